"""SearchByProjection(CurrentFrame, LastFrame) and SearchLocalPoints on the device at the limits of
their routes: the crafted scenes of tests/proj_cases.py (their preconditions are asserted on the CPU
in tests/test_proj_routes.py), the size gates of the list form, non-default image bounds, one
context through every route in turn, ORBHIP_PROJ_DMA, and PredictScale at its steps. Every
comparison is with the oracle and exact (match count, match indices, in_view, level); every test
asserts the route it ran on through orbhip_test_proj_stats."""
import functools

import numpy as np
import pytest

import proj_cases as pc
from helpers import proj_route, proj_stats
from orb_slam3_ros2_amd._lib import Context, OrbHipError, lib
from orb_slam3_ros2_amd.matcher import ORBmatcher, ProjFrame
from orb_slam3_ros2_amd.synthetic import synthetic_projection_scene
from test_proj_routes import frame_of, natural_entries, oracle_last, oracle_local

pytestmark = pytest.mark.gpu

SWITCHES = ("ORBHIP_PROJ_ROUNDS", "ORBHIP_PROJ_TWO", "ORBHIP_PROJ_CAP", "ORBHIP_PROJ_DMA")
# the four forms of tests/test_projection.py and the hipMemcpyAsync upload
FORMS = {"lists": {}, "two": {"ORBHIP_PROJ_TWO": "1"}, "overflow": {"ORBHIP_PROJ_CAP": "2"},
         "rounds": {"ORBHIP_PROJ_ROUNDS": "1"}, "dma": {"ORBHIP_PROJ_DMA": "1"}}


def _set_form(monkeypatch, name):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[name].items():
        monkeypatch.setenv(k, v)
    return name


@pytest.fixture(params=list(FORMS))
def form(request, monkeypatch):
    return _set_form(monkeypatch, request.param)


@pytest.fixture
def default_form(monkeypatch):
    return _set_form(monkeypatch, "lists")


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def want_form(form, max_list, lists_ok=True):
    """The form that must produce the result: rounds only, the rounds after an overflow, the lists."""
    if form == "rounds" or not lists_ok:
        return 2
    return 1 if max_list > (2 if form == "overflow" else 128) else 0


def run_last(ctx, oracle, s, f, ori=False, th=None):
    th = s.get("th_last", 15.0) if th is None else th
    got = ORBmatcher(0.9, ori, ctx=ctx).SearchByProjectionLastFrame(f, s["points"], s["mp_desc"], s["last_octave"],
                                                                    s["last_angle"], th)
    want = oracle_last(oracle, s, f, ori, th)
    assert got[0] == want[0] and np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:10]
    return got, proj_stats(ctx)


def run_local(ctx, oracle, s, f, th=None, nnratio=None):
    th = s.get("th_local", 1.0) if th is None else th
    nnratio = s.get("nnratio", 0.8) if nnratio is None else nnratio
    got = ORBmatcher(nnratio, False, ctx=ctx).SearchLocalPoints(f, s["points"], s["normals"], s["min_dist"],
                                                                s["max_dist"], s["mp_desc"], s["skip"], th=th)
    want = oracle_local(oracle, s, f, th, nnratio)
    assert got[0] == want[0]
    for name, a, b in zip(("match", "in_view", "level"), got[1:], want[1:]):
        assert np.array_equal(a, b), (name, np.nonzero(a != b)[0][:10])
    return got, proj_stats(ctx)


# ---- long chains, walk-order ties ----

@pytest.mark.parametrize("ori", [False, True])
@pytest.mark.parametrize("K", [3, 70, 102])
def test_chain_last(ctx, oracle, form, K, ori):
    """Query i takes keypoint i: K rounds of the fixed point (the owner tables rotate K times, the
    round kernels run in several batches), distance 100 matches and 101 does not. With the
    orientation check three queries of the 70 lie in another rotation bin and are dropped."""
    s = pc.chain(K, rot_outliers=(5, 33, 60) if (ori and K == 70) else ())
    (n, m), st = run_last(ctx, oracle, s, frame_of(s), ori)
    if not (ori and K == 70):
        assert np.array_equal(m, s["expect"])
    else:
        # the rotation filter (k_proj_finish behind the rounds, resolve_body's tail in the list
        # forms) has something to remove: the oracle keeps more without the orientation check
        assert n == 67 < oracle_last(oracle, s, frame_of(s), False, s["th_last"])[0]
    assert st["form"] == want_form(form, K) and st["rounds"] >= K, st
    if st["form"] == 0:
        assert st["entries"] == K * K <= st["ent_cap"]


@pytest.mark.parametrize("hist", ["12-1", "ties"])
def test_rotation_filter_rules(ctx, oracle, form, hist):
    """ComputeThreeMaxima's two rules in k_proj_finish (behind the rounds) and resolve_body's tail
    (the list forms): one keypoint under every query's projection, so each query matches and the
    angles alone decide. A single match beside twelve is dropped (1 < 0.1f * 12); of four equal
    bins the three of lower index stay."""
    from helpers import rot_edge_bins
    bins, kept = rot_edge_bins(hist)
    n = len(bins)
    uv = np.array(pc.LATTICE[:n])
    qd = np.random.default_rng(700 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    s = pc._scene(pc._kps(uv + 0.5, 0), np.stack([pc.flip_low_bits(d, 5) for d in qd]), uv, qd,
                  last_angle=(30.0 * bins).astype(np.float32))
    assert oracle_last(oracle, s, frame_of(s), False)[0] == n
    (gn, gm), st = run_last(ctx, oracle, s, frame_of(s), True)
    assert gn == kept < n
    assert st["form"] == want_form(form, 1), st


@pytest.mark.parametrize("mode,K", [("local", 70), ("ratio", 12)])
def test_chain_local(ctx, oracle, form, mode, K):
    """The same chain through SearchLocalPoints: without a ratio test (best and second never on one
    level), and with queries rejected by it in the middle of the chain, which claim nothing."""
    s = pc.chain(K, mode)
    (n, m, iv, lvl), st = run_local(ctx, oracle, s, frame_of(s))
    assert np.array_equal(m, s["expect"]) and iv.all() and (lvl == pc.LEVEL).all()
    assert st["form"] == want_form(form, K) and st["rounds"] >= (K if mode == "local" else 6), st


@pytest.mark.parametrize("ori", [False, True])
def test_ties(ctx, oracle, form, ori):
    """Every distance equal: query i takes the i-th keypoint in walk order (cell, then index)."""
    s = pc.ties()
    (n, m), st = run_last(ctx, oracle, s, frame_of(s), ori)
    assert n == 40 and np.array_equal(m, s["expect"])
    assert st["form"] == want_form(form, 40) and st["rounds"] >= 40, st


# ---- kRectCap, kProjCap, ent_cap at their values ----

@pytest.mark.parametrize("fm", ["lists", "two"])
@pytest.mark.parametrize("R", [512, 513])
def test_dense_rect(ctx, oracle, monkeypatch, R, fm):
    """512 keypoints in the cell rectangle: listed per wave; 513: the wave tests every keypoint."""
    _set_form(monkeypatch, fm)
    s = pc.dense_rect(R)
    (n, m), st = run_last(ctx, oracle, s, frame_of(s))
    assert n == 40 and np.array_equal(m, s["expect"])
    assert st["form"] == 0 and st["entries"] == 44 * 40 and st["rounds"] >= 40, st


@pytest.mark.parametrize("C,claim,want", [(128, False, 0), (129, False, 1), (129, True, 0)])
def test_list_count(ctx, oracle, default_form, C, claim, want):
    """A list of exactly 128 entries resolves; 129 overflow into the rounds; 129 in the window
    with one claimed are 128 in the list."""
    s = pc.list_count(C, claim)
    (n, m), st = run_last(ctx, oracle, s, frame_of(s))
    assert n == 41 and np.array_equal(m, s["expect"])
    assert st["form"] == want, st
    if want == 0:
        assert st["entries"] == 128 + 40


@pytest.mark.parametrize("fm", ["lists", "two"])
@pytest.mark.parametrize("extra", [0, 1])
def test_entries_at_ent_cap(ctx, oracle, monkeypatch, extra, fm):
    """Exactly ent_cap list entries: the resolve holds them in LDS; one more: it reads them from
    global memory."""
    _set_form(monkeypatch, fm)
    s = pc.entries(extra)
    (n, m), st = run_last(ctx, oracle, s, frame_of(s))
    assert st["form"] == 0 and st["entries"] == s["total"] and st["ent_cap"] == s["ent_cap"], st
    assert (st["entries"] <= st["ent_cap"]) == (extra == 0)


@pytest.mark.parametrize("fm", ["lists", "two"])
def test_entries_natural(ctx, oracle, monkeypatch, fm):
    """An ordinary 2000 x 2000 scene with a wide window: several times ent_cap entries, no list
    above 128."""
    _set_form(monkeypatch, fm)
    s = natural_entries()
    f = frame_of(s)
    total = int(pc.counts_last(s, f)[1].sum())
    (n, m), st = run_last(ctx, oracle, s, f, ori=True)
    assert st["form"] == 0 and st["entries"] == total > st["ent_cap"] == proj_route(2000, 2000)["ent_cap"], st


# ---- the size gates of the list form ----

@functools.lru_cache(maxsize=None)
def _sized(n_kp, n_mp):
    return synthetic_projection_scene(n_kp=n_kp, n_mp=n_mp, seed=n_kp % 97 + n_mp % 89)


@pytest.mark.parametrize("n_kp,n_mp,lists", [(8192, 64, True), (8193, 64, False), (300, 8192, True), (300, 8193, False),
                                             (8192, 6911, True), (8192, 6912, False)])
def test_size_gates(ctx, oracle, default_form, n_kp, n_mp, lists):
    """Each gate of the list form from both sides, both searches. (8192, 6911) leaves the resolve
    no LDS for entries: every one is read from global memory."""
    s = _sized(n_kp, n_mp)
    f = frame_of(s)
    r = proj_route(n_kp, n_mp, int(s["kps"]["octave"].max()))
    assert r["lists"] == lists
    for (got, st) in (run_last(ctx, oracle, s, f, ori=True, th=7.0), run_local(ctx, oracle, s, f, th=1.0)):
        assert got[0] > 0 and st["form"] == (0 if lists else 2), st
        if lists:
            assert st["ent_cap"] == r["ent_cap"] and st["entries"] > 0
            if (n_kp, n_mp) == (8192, 6911):
                assert st["ent_cap"] == 0


@pytest.mark.parametrize("octave,lists", [(15, True), (16, False)])
def test_octave_gate(ctx, oracle, default_form, octave, lists):
    """A keypoint of octave 16 does not fit the list entry's 4 bits: the rounds run."""
    s = synthetic_projection_scene(n_kp=300, n_mp=200, seed=81)
    s["kps"]["octave"][17] = octave
    f = frame_of(s, n_levels=18)
    assert proj_route(300, 200, int(s["kps"]["octave"].max()))["lists"] == lists
    for (got, st) in (run_last(ctx, oracle, s, f, ori=True), run_local(ctx, oracle, s, f, th=3.0)):
        assert got[0] > 0 and st["form"] == (0 if lists else 2), st


def test_largest_frame(ctx, oracle, default_form):
    """65535 keypoints (the rounds: the index fills the key's 16 bits): a query built onto the last
    keypoint takes index 65534. 65536 keypoints are refused."""
    s = synthetic_projection_scene(n_kp=65535, n_mp=64, seed=82)
    last = 65534
    q = s["pose_q"].astype(np.float64)
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    s["kps"]["x"][last], s["kps"]["y"][last], s["kps"]["octave"][last] = 321.0, 243.0, 2
    Xc = np.array([(321.0 - s["cx"]) / s["fx"] * 3.0, (243.0 - s["cy"]) / s["fy"] * 3.0, 3.0])
    s["points"][40] = ((Xc - s["pose_t"].astype(np.float64)) @ R).astype(np.float32)
    s["mp_desc"][40], s["last_octave"][40] = s["desc"][last], 2
    s["claimed"][last] = 0
    f = frame_of(s)
    (n, m), st = run_last(ctx, oracle, s, f, ori=False)
    assert m[40] == last and st["form"] == 2, st
    assert not proj_route(65535, 64)["lists"]
    kps = np.concatenate([s["kps"], s["kps"][:1]])
    big = ProjFrame(kps, np.concatenate([s["desc"], s["desc"][:1]]), s["pose_q"], s["pose_t"], s["fx"], s["fy"],
                    s["cx"], s["cy"])
    with pytest.raises(OrbHipError):
        ORBmatcher(0.9, False, ctx=ctx).SearchByProjectionLastFrame(big, s["points"], s["mp_desc"], s["last_octave"],
                                                                    s["last_angle"], 15.0)
    with pytest.raises(OrbHipError):
        ORBmatcher(0.8, False, ctx=ctx).SearchLocalPoints(big, s["points"], s["normals"], s["min_dist"], s["max_dist"],
                                                          s["mp_desc"], s["skip"])


# ---- image bounds other than [0, 640] x [0, 480] ----

@pytest.mark.parametrize("which", ["kitti", "undistorted"])
def test_bounds(ctx, oracle, form, which):
    """A 1241 x 376 frame, and bounds with a negative minimum as an undistorted frame has: the
    cell sizes follow the bounds."""
    if which == "kitti":
        s = synthetic_projection_scene(n_kp=900, n_mp=700, seed=83, width=1241, height=376)
        f = frame_of(s, width=1241, height=376)
    else:
        s = synthetic_projection_scene(n_kp=900, n_mp=700, seed=84)
        s["kps"]["x"][:40] -= 12.0          # some keypoints left of 0, still on the grid
        s["kps"]["y"][40:80] -= 10.0
        f = frame_of(s, bounds=(-14.5, 652.25, -11.75, 489.5))
    (g, st) = run_last(ctx, oracle, s, f, ori=True)
    cand = pc.counts_last(s, f)[1]
    assert g[0] > 100 and st["form"] == want_form(form, cand.max()), st
    if st["form"] == 0:
        assert st["entries"] == cand.sum()
    (g, st) = run_local(ctx, oracle, s, f, th=3.0)
    cand = pc.window_counts(f, pc.windows_local(f, s["points"], s["normals"], 3.0, g[2], g[3]))[1]
    assert g[0] > 50 and st["form"] == want_form(form, cand.max()), st
    if st["form"] == 0:
        assert st["entries"] == cand.sum()


def test_distance_256(ctx, oracle, form):
    """The only candidate at distance 256: an entry in the list, no match."""
    s = pc.dist256()
    f = frame_of(s)
    (n, m), st = run_last(ctx, oracle, s, f)
    assert n == 5 and np.array_equal(m, s["expect"]) and st["form"] == want_form(form, 1), st
    if st["form"] == 0:
        assert st["entries"] == 6
    (n, m, iv, lvl), st = run_local(ctx, oracle, s, f)
    assert n == 5 and np.array_equal(m, s["expect"]) and st["form"] == want_form(form, 1), st
    if st["form"] == 0:
        assert st["entries"] == 6


def test_no_queries_reports_no_form(ctx, oracle, default_form):
    s = synthetic_projection_scene(n_kp=50, n_mp=0, seed=85)
    n, m = ORBmatcher(0.9, True, ctx=ctx).SearchByProjectionLastFrame(frame_of(s), s["points"], s["mp_desc"],
                                                                     s["last_octave"], s["last_angle"])
    assert n == 0 and m.size == 0 and proj_stats(ctx)["form"] == -1
    fresh = Context()
    try:
        assert proj_stats(fresh) == {"form": -1, "rounds": 0, "entries": 0, "ent_cap": 0}
    finally:
        fresh.close()


# ---- one context through every route ----

def test_one_context_through_every_route(oracle, default_form):
    """Entries in global memory, an overflow into the rounds, the rounds alone, a tiny search, the
    first again, on ONE context (the arrival counter back at 0 after every one-launch search, the
    staging block regrown and reused): each result equals the oracle's and, bit for bit, the same
    call on a fresh context."""
    steps = [(natural_entries(), True, None, 0), (pc.list_count(129), False, None, 1),
             (_sized(8193, 64), True, 7.0, 2), (synthetic_projection_scene(n_kp=8, n_mp=4, seed=60), True, None, 0)]
    steps.append(steps[0])
    shared = Context()
    try:
        for i, (s, ori, th, want) in enumerate(steps):
            f = frame_of(s)
            got, st = run_last(shared, oracle, s, f, ori, th)
            assert st["form"] == want, (i, st)
            if i in (0, 4):
                assert st["entries"] > st["ent_cap"]
            fresh = Context()
            try:
                alone, st2 = run_last(fresh, oracle, s, f, ori, th)
            finally:
                fresh.close()
            assert got[0] == alone[0] and got[1].tobytes() == alone[1].tobytes(), i
            assert (st2["form"], st2["entries"], st2["ent_cap"]) == (st["form"], st["entries"], st["ent_cap"]), i
            gl, stl = run_local(shared, oracle, s, f, th=3.0)
            assert stl["form"] in (0, 2) and (stl["form"] == 2) == (want == 2), (i, stl)
    finally:
        shared.close()


# ---- ORBHIP_PROJ_DMA outside the projection searches ----

def test_dma_upload_outside_the_projection_searches(ctx, oracle, monkeypatch):
    """ORBHIP_PROJ_DMA=1 (read by the staging helper's upload_inputs on every call) under one Fuse
    call of the Fuse parity fixtures, equal to its model (Fuse uploads its block by hipMemcpyAsync
    itself: the switch must leave it alone), and under the callers of upload_inputs other than the
    projection searches: SearchForInitialization and a one-frame PoseOptimization, equal to the
    oracle."""
    import fuse_numpy as F
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.synthetic import synthetic_init_pair, synthetic_pose_problem
    _set_form(monkeypatch, "dma")
    s = F.parity_scene(0)
    gn, gi, gd, gl = ORBmatcher(0.6, True, ctx=ctx).Fuse(s["kfs"], s["points"], s["normals"], s["min_dist"],
                                                        s["max_dist"], s["mp_desc"], s["inv_level_sigma2"], s["th"],
                                                        s["skip"], s["pair_skip"])
    rn, ri, rd, rl = s["expected"][:4]
    assert np.array_equal(gi, ri) and np.array_equal(gd, rd) and np.array_equal(gl, rl) and gn.tolist() == rn.tolist()
    assert (ri >= 0).sum() > 0
    k1, d1, k2, d2, prev = synthetic_init_pair(n1=300, seed=62)
    got = ORBmatcher(0.9, True, ctx=ctx).SearchForInitialization(k1, d1, k2, d2, prev, 100)
    want = oracle.search_for_initialization(k1, d1, k2, d2, prev, 100, 0.9, True)
    assert want[0] > 0 and got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
    prob, _ = synthetic_pose_problem(n=10, outlier_frac=0.2, seed=63)
    r = Optimizer(ctx=ctx).PoseOptimization(prob)
    o = oracle.pose_optimization(prob)
    assert r.n_inliers == o["n_inliers"] and np.array_equal(r.outlier, o["outlier"])
    assert np.abs(r.pose_t - o["pose_t"]).max() <= 1e-4 * max(1.0, float(np.abs(o["pose_t"]).max()))
    # the projection search itself under the same switch reports the list form
    sc = pc.dist256()
    assert run_last(ctx, oracle, sc, frame_of(sc))[1]["form"] == 0


# ---- PredictScale ----

def _sweep(oracle, lo, hi, log_sf, n_levels):
    bad = 0
    chunk = 1 << 24
    for a in range(lo, hi + 1, chunk):
        b = min(a + chunk - 1, hi)
        ref = oracle.predict_scale_range(a, b, log_sf, n_levels)
        r = lib().orbhip_test_predict_scale_sweep(a, b, log_sf, n_levels, ref.ctypes.data)
        assert r >= 0
        bad += r
    return bad


def _bits(x):
    return int(np.float32(x).view(np.uint32))


def test_predict_scale_matches_host_every_float():
    """The device's PredictScale (the one function both isInFrustum and Fuse call) against the
    host's ceil(log(ratio) / logf(1.2f)) clamped to 8 levels, for every float ratio in [0.5, 8)."""
    from oracle import pyoracle
    log_sf = float(np.log(np.float32(1.2)).astype(np.float32))
    bad = _sweep(pyoracle, _bits(0.5), _bits(8.0) - 1, log_sf, 8)
    print(f"PREDICT_SCALE_SWEEP sf=1.2 levels=8 ratios=[0.5,8) mismatches={bad}")
    assert bad == 0


def test_predict_scale_matches_host_at_powers_of_two():
    """Scale factor 2.0, 8 levels: 4096 ulps either side of every step 2^k, k = 0..7."""
    from oracle import pyoracle
    log_sf = float(np.log(np.float32(2.0)).astype(np.float32))
    bad = 0
    for k in range(8):
        c = _bits(2.0 ** k)
        bad += _sweep(pyoracle, c - 4096, c + 4096, log_sf, 8)
    print(f"PREDICT_SCALE_SWEEP sf=2.0 levels=8 steps=2^0..2^7 +-4096ulp mismatches={bad}")
    assert bad == 0


def test_predict_scale_matches_host_past_16_levels():
    """Scale factor 1.1, 24 levels (the first 16 steps travel in the kernel arguments, the others
    are read from memory): 4096 ulps either side of every step."""
    from oracle import pyoracle
    log_sf = float(np.log(np.float32(1.1)).astype(np.float32))
    thr = np.zeros(24, np.float32)
    assert lib().orbhip_test_level_thresholds(log_sf, 24, thr.ctypes.data) == 0
    bad = sum(_sweep(pyoracle, _bits(t) - 4096, _bits(t) + 4096, log_sf, 24) for t in thr[1:])
    print(f"PREDICT_SCALE_SWEEP sf=1.1 levels=24 steps +-4096ulp mismatches={bad}")
    assert bad == 0


@pytest.mark.parametrize("fm", ["lists", "rounds"])
def test_levels_at_the_steps(ctx, oracle, monkeypatch, fm):
    """SearchLocalPoints with max_dist / dist within a few ulps of every step 1.2^k, both sides
    (tests/test_proj_routes.py asserts that the oracle's levels take both values at each k)."""
    _set_form(monkeypatch, fm)
    s = pc.scale_steps()
    f = frame_of(s, n_levels=pc.STEP_LEVELS)
    (n, m, iv, lvl), st = run_local(ctx, oracle, s, f)
    assert iv.all() and st["form"] == (0 if fm == "lists" else 2), st
