"""orbhip_search_by_projection_sim3 and orbhip_fuse_sim3 on the GPU against the numpy restatement
(tests/sim3_numpy.py): every output must be EQUAL, for every point, with no tolerance. The scenes
keep PredictScale's ceil 1e-3 away from a step (tests/test_sim3.py checks that on the CPU), which is
all that separates the device's logf from numpy's. Outputs are pre-filled with a poison value."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, FrameC, LocalPointsC, OrbHipError, lib, ptr
from orb_slam3_ros2_amd.matcher import ORBmatcher, ProjFrame
from orb_slam3_ros2_amd.synthetic import synthetic_fuse_scene, synthetic_sim3_scene

import fuse_numpy as F
import sim3_numpy as S

pytestmark = pytest.mark.gpu
POISON = -7


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _points_c(s):
    n = s["points"].shape[0]
    sk = None if s["skip"] is None else np.ascontiguousarray(s["skip"], np.uint8)
    arrs = [np.ascontiguousarray(s[k]) for k in ("points", "normals", "min_dist", "max_dist", "mp_desc")] + [sk]
    return n, LocalPointsC(n, *[ptr(a) for a in arrs]), arrs


# ---- SearchByProjection with a Sim3 ----

def _mirror(ctx, s):
    return ORBmatcher(0.6, True, ctx=ctx).SearchByProjectionSim3(s["kf"], s["points"], s["normals"], s["min_dist"],
                                                                 s["max_dist"], s["mp_desc"], s["th"], s["ratio"],
                                                                 s["skip"])


def _raw(ctx, s, want_dist=True, want_level=True, ratio=None):
    """The C entry point itself: (return value, match, match_dist or None, level or None)."""
    n, lc, keep = _points_c(s)
    fc = s["kf"].to_c()
    match = np.full(n, POISON, np.int32)
    dist = np.full(n, POISON, np.int32) if want_dist else None
    lvl = np.full(n, POISON, np.int32) if want_level else None
    rc = lib().orbhip_search_by_projection_sim3(ctx.handle, ctypes.byref(fc), ctypes.byref(lc), s["th"],
                                                s["ratio"] if ratio is None else ratio, ptr(match), ptr(dist), ptr(lvl))
    return rc, match, dist, lvl


def _assert_search_equal(got, want):
    assert got[0] == want[0] == int((got[1] >= 0).sum())
    for name, g, r in zip(("match", "match_dist", "level"), got[1:4], want[1:4]):
        bad = np.nonzero(g != r)[0]
        assert bad.size == 0, f"{name}: {len(bad)} points differ, first {bad[:5].tolist()}: gpu {g[bad[:5]].tolist()} " \
                              f"restatement {r[bad[:5]].tolist()}"


@pytest.mark.parametrize("k", range(len(S.PARITY_SCENES)))
def test_parity_scene_set(ctx, k):
    """n_kp = 300, n_mp = 400 at upstream's (th, ratioHamming) pairs: the scenes whose conditions
    tests/test_sim3.py asserts (points that lose their first choice, that get a later one, that end
    with none; keypoints claimed at call time; every gate)."""
    s = S.parity_scene(k)
    want = s["expected"]
    _assert_search_equal(_mirror(ctx, s), want)
    _assert_search_equal(_raw(ctx, s), want)
    # the optional outputs may be NULL
    for want_dist, want_level in ((False, False), (True, False), (False, True)):
        rc, match, dist, lvl = _raw(ctx, s, want_dist, want_level)
        assert rc == want[0] and np.array_equal(match, want[1])
        assert dist is None or np.array_equal(dist, want[2])
        assert lvl is None or np.array_equal(lvl, want[3])


@pytest.mark.parametrize("n_mp", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_point_count_edges(ctx, n_mp):
    """Points at the wave and tile boundaries (four lanes per point) against keyframes of 1, 63, 64,
    65 and 257 keypoints: five SearchByProjection calls, one Fuse call of five keyframes."""
    f = synthetic_fuse_scene([1, 63, 64, 65, 257], (3 * n_mp + 3) // 4, 5, seed=100 + n_mp)
    matched = 0
    for b, n_kp in enumerate((1, 63, 64, 65, 257)):
        s = synthetic_sim3_scene(n_kp, n_mp, seed=100 + n_mp + b, th=5.0, ratio=1.0, n_claimed=n_kp // 8)
        assert s["kf"].kps.shape[0] == n_kp and s["points"].shape[0] == n_mp
        want = S.search_scene(s)
        _assert_search_equal(_raw(ctx, s), want)
        matched += want[0]
    if n_mp >= 63:
        assert matched > 0
    want = S.fuse_sim3(f["kfs"], f["points"], f["normals"], f["min_dist"], f["max_dist"], f["mp_desc"], 4.0, f["skip"],
                       f["pair_skip"])
    _assert_fuse_equal(_fuse_mirror(ctx, f, th=4.0), want)


@pytest.mark.parametrize("claimed", [False, True])
def test_chain_deeper_than_the_stored_lists(ctx, claimed):
    """300 keypoints of one descriptor in one grid cell, 320 points with that descriptor projecting
    into it: every point's list holds every free keypoint at distance 0, point m must get the m-th
    free index, the points past the last free keypoint nothing. The chain is 300 (150) deep: far past
    the stored list capacity, and the resolve has no round cap below (points with a list) + 1."""
    cap = lib().orbhip_test_sim3_list_cap()
    free = np.arange(0, 300, 2) if claimed else np.arange(300)
    assert 1 <= cap < len(free) // 4
    s = S.chain_scene(300, 320, every_second_claimed=claimed)
    want = np.full(320, -1, np.int32)
    want[:len(free)] = free
    rc, match, dist, lvl = _raw(ctx, s)
    assert match.tolist() == want.tolist() and rc == len(free)
    assert (dist[:len(free)] == 0).all() and (dist[len(free):] == 256).all() and (lvl == 7).all()
    _assert_search_equal(_mirror(ctx, s), S.search_scene(s))


def test_lists_longer_than_stored_with_distinct_distances_and_cells(ctx):
    """48 points that all see the same ~40 free keypoints over 19 grid cells, at distinct distances:
    most points end up far past the stored capacity of their list, where the resolve walks the
    window again for the next key."""
    s = S.cluster_scene()
    lists, _ = S.lists_of_scene(s)
    pos = S.resolve_sorted(lists)[3]
    assert pos.max() >= 3 * lib().orbhip_test_sim3_list_cap() and (pos < 0).sum() >= 3
    want = S.search_scene(s)
    _assert_search_equal(_raw(ctx, s), want)
    _assert_search_equal(_mirror(ctx, s), want)


def test_determinism(ctx):
    s = S.parity_scene(0)
    a, b = _raw(ctx, s), _raw(ctx, s)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))
    f = F.parity_scene(0)
    a, b = _fuse_raw(ctx, f), _fuse_raw(ctx, f)
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


# ---- Fuse with a Sim3 ----

def _fuse_mirror(ctx, s, **over):
    a = dict(s, **over)
    return ORBmatcher(0.6, True, ctx=ctx).FuseSim3(a["kfs"], a["points"], a["normals"], a["min_dist"], a["max_dist"],
                                                   a["mp_desc"], a["th"], a["skip"], a["pair_skip"])


def _fuse_raw(ctx, s, pair_skip="scene", th=4.0, kfs=None):
    kfs = list(s["kfs"] if kfs is None else kfs)
    B = len(kfs)
    n, lc, keep = _points_c(s)
    arr = (FrameC * max(B, 1))(*[k.to_c() for k in kfs])
    if isinstance(pair_skip, str):
        pair_skip = s["pair_skip"]
    ps = None if pair_skip is None else np.ascontiguousarray(pair_skip, np.uint8)
    nf = np.full(B, POISON, np.int32)
    idx = np.full((B, n), POISON, np.int32)
    dist = np.full((B, n), POISON, np.int32)
    lvl = np.full((B, n), POISON, np.int32)
    rc = lib().orbhip_fuse_sim3(ctx.handle, arr, B, ctypes.byref(lc), ptr(ps), th, ptr(idx), ptr(dist), ptr(lvl), ptr(nf))
    return rc, nf, idx, dist, lvl


def _assert_fuse_equal(got, want):
    for name, g, r in zip(("nfused", "best_idx", "best_dist", "level"), got, want[:4]):
        assert g.shape == r.shape
        bad = np.argwhere(g != r)
        assert bad.size == 0, f"{name}: {len(bad)} entries differ, first {bad[:5].tolist()}"
    assert got[0].tolist() == (got[1] >= 0).sum(1).tolist()


@pytest.mark.parametrize("k", range(len(F.PARITY_SCENES)))
def test_fuse_sim3_parity_and_equality_with_fuse_at_zero_inv_level_sigma2(ctx, k):
    """B = 3 at th = 4 (SearchAndFuse), pair_skip given and NULL: equal to the restatement, through
    the mirror and the bare C call, and to orbhip_fuse called with an all-zero inv_level_sigma2."""
    s = F.parity_scene(k)
    mt = ORBmatcher(0.6, True, ctx=ctx)
    for ps in (s["pair_skip"], None):
        want = S.fuse_sim3(s["kfs"], s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], 4.0,
                           s["skip"], ps)
        assert want[0].min() > 50
        _assert_fuse_equal(_fuse_mirror(ctx, s, th=4.0, pair_skip=ps), want)
        rc, nf, idx, dist, lvl = _fuse_raw(ctx, s, pair_skip="scene" if ps is not None else None)
        assert rc == int(want[0].sum())
        _assert_fuse_equal((nf, idx, dist, lvl), want)
        zero = mt.Fuse(s["kfs"], s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"],
                       np.zeros(8, np.float32), 4.0, s["skip"], ps)
        _assert_fuse_equal(zero, want)


def test_search_equals_fuse_sim3_where_no_best_keypoint_is_shared(ctx):
    """Without contention and with nothing claimed the greedy pass is the per-point minimum: at ratio
    1.0 (thr = 50 = TH_LOW) match equals FuseSim3's best_idx for one keyframe."""
    s = synthetic_fuse_scene(300, 300, 1, seed=7, th=4.0)
    want = S.fuse_sim3(s["kfs"], s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], 4.0, s["skip"])
    first = want[1][0]
    shared = {int(j) for j in first[first >= 0] if (first == j).sum() > 1}
    skip = np.array(s["skip"], np.uint8)
    for j in shared:                                       # keep the first point of every shared keypoint only
        skip[np.nonzero(first == j)[0][1:]] = 1
    want = S.fuse_sim3(s["kfs"], s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], 4.0, skip)
    got = want[1][0][want[1][0] >= 0]
    assert len(got) > 100 and len(set(got.tolist())) == len(got)
    mt = ORBmatcher(0.6, True, ctx=ctx)
    kf = s["kfs"][0]
    assert kf.claimed is None
    nf, idx, dist, lvl = mt.FuseSim3([kf], s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], 4.0, skip)
    nm, match, mdist, mlvl = mt.SearchByProjectionSim3(kf, s["points"], s["normals"], s["min_dist"], s["max_dist"],
                                                       s["mp_desc"], 4.0, 1.0, skip)
    _assert_fuse_equal((nf, idx, dist, lvl), want)
    assert nm == nf[0] and np.array_equal(match, idx[0]) and np.array_equal(mlvl, lvl[0])
    assert np.array_equal(mdist[match >= 0], dist[0][match >= 0]) and (mdist[match < 0] == 256).all()


def test_one_staging_block_across_fuse_and_sim3_calls():
    """Fuse, Fuse with a Sim3 and the Sim3 projection search stage into ONE block per context: Fuse at
    B = 1, 3 points, 5 keypoints; SearchByProjectionSim3 at 200 points x 300 keypoints (the block
    grows); FuseSim3 at B = 3, 40 points, 60 keypoints (the block is reused, larger than needed); the
    first Fuse call again. Every result equals the restatement and the same call on a fresh context."""
    small = synthetic_fuse_scene(5, 3, 1, seed=31)
    big = synthetic_sim3_scene(300, 200, seed=32, th=4.0, ratio=1.0)
    mid = synthetic_fuse_scene(60, 40, 3, seed=33)
    assert small["points"].shape[0] == 3 and [k.kps.shape[0] for k in small["kfs"]] == [5]
    assert big["points"].shape[0] == 200 and big["kf"].kps.shape[0] == 300
    want_small = F.fuse_scene(dict(small, ratios=None))[:4]
    want_big = S.search_scene(big)
    want_mid = S.fuse_sim3(mid["kfs"], mid["points"], mid["normals"], mid["min_dist"], mid["max_dist"], mid["mp_desc"],
                           4.0, mid["skip"], mid["pair_skip"])[:4]
    assert want_big[0] > 20 and want_mid[0].sum() > 0                  # not vacuous

    def fuse(c):
        s = small
        return ORBmatcher(0.6, True, ctx=c).Fuse(s["kfs"], s["points"], s["normals"], s["min_dist"], s["max_dist"],
                                                 s["mp_desc"], s["inv_level_sigma2"], s["th"], s["skip"], s["pair_skip"])

    steps = [(fuse, want_small, _assert_fuse_equal),
             (lambda c: _mirror(c, big), want_big, _assert_search_equal),
             (lambda c: _fuse_mirror(c, mid, th=4.0), want_mid, _assert_fuse_equal),
             (fuse, want_small, _assert_fuse_equal)]
    shared = Context()
    try:
        for call, want, check in steps:
            got = call(shared)
            check(got, want)
            fresh = Context()
            try:
                check(call(fresh), got)
            finally:
                fresh.close()
    finally:
        shared.close()


# ---- arguments ----

def _blank_like(kf, n=0, **kw):
    return ProjFrame(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx,
                     kf.cy, **kw)


def _blank_points(n):
    return dict(points=np.zeros((n, 3), np.float32), normals=np.zeros((n, 3), np.float32),
                min_dist=np.ones(n, np.float32), max_dist=np.ones(n, np.float32), mp_desc=np.zeros((n, 32), np.uint8),
                skip=None, pair_skip=None)


def test_envelope_and_argument_errors(ctx):
    s = synthetic_fuse_scene(40, 30, 2, seed=400)
    kf = s["kfs"][0]
    UNSUPPORTED, ARG = -5, -1

    def fuse(kfs, n=None):
        a = dict(s, **(_blank_points(n) if n is not None else {}))
        return _fuse_raw(ctx, a, kfs=kfs)

    def search(kf, n=None, ratio=1.5):
        a = dict(s, kf=kf, th=3.0, ratio=ratio, **(_blank_points(n) if n is not None else {}))
        return _raw(ctx, a)

    many_levels = _blank_like(kf, 3, n_levels=257)
    assert fuse([kf] * 65, 30)[0] == UNSUPPORTED
    assert fuse([kf], 65537)[0] == UNSUPPORTED and search(kf, 65537)[0] == UNSUPPORTED
    assert fuse([many_levels], 30)[0] == UNSUPPORTED and search(many_levels, 30)[0] == UNSUPPORTED
    assert fuse([_blank_like(kf, 65536)], 30)[0] == UNSUPPORTED and search(_blank_like(kf, 65536), 30)[0] == UNSUPPORTED
    for octave in (8, -1):
        bad = _blank_like(kf, 3)
        bad.kps["octave"][1] = octave
        assert fuse([kf, bad], 30)[0] == ARG and search(bad, 30)[0] == ARG
    for ratio in (0.0, -1.0, float("nan"), float("inf")):
        rc, match, _, _ = search(kf, 30, ratio=ratio)
        assert rc == ARG and (match == POISON).all()
    other_sf = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, scale_factor=1.25)
    other_nl = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, n_levels=7)
    for other in (other_sf, other_nl):
        assert fuse([kf, other], 30)[0] == ARG
    # B = 0 or n = 0 returns 0 and writes nothing past nfused
    rc, nf, idx, dist, lvl = fuse([], 30)
    assert rc == 0 and (idx == POISON).all()
    rc, nf, idx, dist, lvl = fuse([kf, kf], 0)
    assert rc == 0 and nf.tolist() == [0, 0]
    rc, nf, idx, dist, lvl = _fuse_raw(ctx, dict(s, **_blank_points(30)), kfs=[kf, kf])
    assert rc == 0 and nf.tolist() == [0, 0] and not (idx == POISON).any()      # (a real call does write)
    assert search(kf, 0)[0] == 0
    # the envelope itself is accepted
    rc, nf, idx, _, _ = fuse([kf] * 64, 30)
    assert rc >= 0 and not (nf == POISON).any() and not (idx == POISON).any()
    with pytest.raises(OrbHipError):
        ORBmatcher(0.6, True, ctx=ctx).SearchByProjectionSim3(kf, s["points"], s["normals"], s["min_dist"],
                                                              s["max_dist"], s["mp_desc"], 3.0, 0.0)
