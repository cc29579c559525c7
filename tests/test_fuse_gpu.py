"""orbhip_fuse on the GPU against the numpy restatement (tests/fuse_numpy.py): best_idx, best_dist,
level, nfused and the return value must be EQUAL, for every pair, with no tolerance. The scenes keep
PredictScale's ceil 1e-3 away from a step (tests/test_fuse.py checks that on the CPU), which is all
that separates the device's logf from numpy's; every other operation is one IEEE fp32 operation on
both sides."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, FrameC, LocalPointsC, OrbHipError, lib, ptr
from orb_slam3_ros2_amd.matcher import ORBmatcher, ProjFrame
from orb_slam3_ros2_amd.synthetic import _flip_bits, synthetic_fuse_scene, synthetic_projection_scene

import fuse_numpy as F

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _library(ctx, s, **over):
    a = dict(s, **over)
    return ORBmatcher(0.6, True, ctx=ctx).Fuse(a["kfs"], a["points"], a["normals"], a["min_dist"], a["max_dist"],
                                               a["mp_desc"], a["inv_level_sigma2"], a["th"], a["skip"], a["pair_skip"])


def _assert_equal(got, want):
    gn, gi, gd, gl = got
    rn, ri, rd, rl = want[:4]
    assert gi.shape == ri.shape and gn.shape == rn.shape
    for name, g, r in (("best_idx", gi, ri), ("best_dist", gd, rd), ("level", gl, rl)):
        bad = np.argwhere(g != r)
        assert bad.size == 0, f"{name}: {len(bad)} pairs differ, first (kf, point) {bad[:5].tolist()}: " \
                              f"gpu {g[tuple(bad[:5].T)].tolist()} restatement {r[tuple(bad[:5].T)].tolist()}"
    assert gn.tolist() == rn.tolist() == (gi >= 0).sum(1).tolist()


def _parity(ctx, s, **over):
    """Runs both, asserts equality, returns the restatement's (nfused, best_idx, best_dist, level, counters)."""
    want = s["expected"] if "expected" in s and not over else F.fuse_scene(dict(s, ratios=None), **over)
    _assert_equal(_library(ctx, s, **over), want)
    return want


def _raw(ctx, s, pair_skip="scene", want_dist=True, want_level=True):
    """The C entry point itself: (return value, nfused, best_idx, best_dist or None, level or None)."""
    kfs = list(s["kfs"])
    B, n = len(kfs), s["points"].shape[0]
    arr = (FrameC * max(B, 1))(*[k.to_c() for k in kfs])
    sk = np.ascontiguousarray(s["skip"], np.uint8)
    lc = LocalPointsC(n, ptr(s["points"]), ptr(s["normals"]), ptr(s["min_dist"]), ptr(s["max_dist"]),
                      ptr(s["mp_desc"]), ptr(sk))
    ps = np.ascontiguousarray(s["pair_skip"], np.uint8) if isinstance(pair_skip, str) else pair_skip
    nf = np.full(B, -7, np.int32)
    idx = np.full((B, n), -7, np.int32)
    dist = np.full((B, n), -7, np.int32) if want_dist else None
    lvl = np.full((B, n), -7, np.int32) if want_level else None
    rc = lib().orbhip_fuse(ctx.handle, arr, B, ctypes.byref(lc), ptr(ps), ptr(s["inv_level_sigma2"]), s["th"],
                           ptr(idx), ptr(dist), ptr(lvl), ptr(nf))
    return rc, nf, idx, dist, lvl


@pytest.mark.parametrize("k", range(len(F.PARITY_SCENES)))
def test_parity_scene_set(ctx, k):
    """n_kp = 300, n_mp = 300, B = 3: the scenes whose conditions tests/test_fuse.py asserts (every
    gate fires, both tie kinds, levels 0..7)."""
    s = F.parity_scene(k)
    rn = _parity(ctx, s)[0]
    assert (rn * 3 >= 300).all()
    rc, nf, idx, dist, lvl = _raw(ctx, s)
    assert rc == int(rn.sum())                              # the return value
    _assert_equal((nf, idx, dist, lvl), s["expected"])


@pytest.mark.parametrize("n_mp", [1, 15, 16, 17, 63, 64, 65, 255, 256, 257])
def test_point_count_edges(ctx, n_mp):
    """Points at the wave and tile boundaries (four lanes per point: a wave holds 16 points, a
    work-group 64; 256 is a work-group of the lane-per-point form) against keyframes of 1, 63, 64, 65
    and 257 keypoints, the five as five keyframes of one call."""
    s = synthetic_fuse_scene([1, 63, 64, 65, 257], n_mp, 5, seed=100 + n_mp)
    assert [k.kps.shape[0] for k in s["kfs"]] == [1, 63, 64, 65, 257] and s["points"].shape[0] == n_mp
    rn = _parity(ctx, s)[0]
    if n_mp >= 63:
        assert rn[1:].min() > 0          # not vacuous: every keyframe of >= 63 keypoints fuses something


def _cell_scene(n_kp=300, n_mp=48, seed=3):
    """Every keypoint in ONE grid cell (px 32, py 24) of a keyframe at the identity pose, the points
    projecting into and around it; descriptors planted with few flipped bits, several equal."""
    rng = np.random.Generator(np.random.PCG64(seed))
    pts = [F.make_point(rng.uniform(312, 328), rng.uniform(232, 248), rng.uniform(2, 5), int(rng.integers(0, 8)))
           for _ in range(n_mp)]
    mp_desc = rng.integers(0, 256, (n_mp, 32), dtype=np.uint8)
    kps, descs = [], []
    for i in range(n_kp):
        m = int(rng.integers(0, n_mp))
        kps.append((rng.uniform(315.1, 324.9), rng.uniform(235.1, 244.9), int(rng.integers(0, 8))))
        descs.append(_flip_bits(rng, mp_desc[m], int(rng.choice([0, 5, 5, 30, 60]))))
    kf = F.make_keyframe(kps, descs)
    assert list(F.Grid(kf).cells) == [(32, 24)]
    return dict(kfs=[kf], points=np.stack([p["P"] for p in pts]), normals=np.stack([p["normal"] for p in pts]),
                min_dist=np.array([p["min_dist"] for p in pts], np.float32),
                max_dist=np.array([p["max_dist"] for p in pts], np.float32), mp_desc=mp_desc, skip=None,
                pair_skip=None, inv_level_sigma2=F.parity_scene(0)["inv_level_sigma2"], th=3.0)


def test_one_cell_holding_300_keypoints(ctx):
    s = _cell_scene()
    rn, _, _, _, cnt = _parity(ctx, s)
    assert rn[0] >= 10 and cnt["tie_index"] > 0 and cnt["cand_chi2"] > 0 and cnt["cand_level_low"] > 0


def _blank_like(kf, n=0):
    return ProjFrame(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx,
                     kf.cy)


def test_empty_keyframe_between_two(ctx):
    s = F.parity_scene(1)
    kfs = [s["kfs"][0], _blank_like(s["kfs"][1]), s["kfs"][2]]
    rn, ri, rd, _, _ = _parity(ctx, s, kfs=kfs)
    assert rn[1] == 0 and (ri[1] == -1).all() and (rd[1] == 256).all() and rn[0] > 0 and rn[2] > 0
    e = s["expected"]
    assert np.array_equal(ri[0], e[1][0]) and np.array_equal(ri[2], e[1][2])     # the neighbours are unaffected


def test_keyframe_with_every_keypoint_outside_the_grid(ctx):
    """PosInGrid's round puts x >= 635 in column 64: such keypoints are in no cell."""
    s = F.parity_scene(2)
    src = s["kfs"][1]
    kps = src.kps.copy()
    kps["x"] = np.float32(635.5) + (np.arange(kps.shape[0]) % 40).astype(np.float32) * np.float32(0.1)
    out = ProjFrame(kps, src.desc, src.pose_q, src.pose_t, src.fx, src.fy, src.cx, src.cy)
    assert F.Grid(out).cells == {}
    rn, ri, rd, rl, _ = _parity(ctx, s, kfs=[s["kfs"][0], out, s["kfs"][2]])
    assert rn[1] == 0 and (rd[1] == 256).all() and (rl[1] >= 0).any() and rn[0] > 0 and rn[2] > 0


@pytest.mark.parametrize("B,n_kp,n_mp", [(1, 200, 150), (2, 200, 150), (64, 40, 60)])
def test_batch_sizes(ctx, B, n_kp, n_mp):
    s = synthetic_fuse_scene(n_kp, n_mp, B, seed=200 + B)
    rn = _parity(ctx, s)[0]
    assert rn.shape == (B,) and (rn > 0).all()


def test_null_pair_skip_equals_zeros_and_optional_outputs(ctx):
    s = F.parity_scene(0)
    B, n = 3, s["points"].shape[0]
    none = _raw(ctx, s, pair_skip=None)
    zeros = _raw(ctx, s, pair_skip=np.zeros((B, n), np.uint8))
    assert none[0] == zeros[0] > 0
    for a, b in zip(none[1:], zeros[1:]):
        assert np.array_equal(a, b)
    _assert_equal(none[1:], F.fuse_scene(dict(s, ratios=None), pair_skip=None))
    # best_dist and level are optional: best_idx, nfused and the return value do not depend on them
    full = _raw(ctx, s)
    for want_dist, want_level in ((False, False), (True, False), (False, True)):
        part = _raw(ctx, s, want_dist=want_dist, want_level=want_level)
        assert part[0] == full[0] and np.array_equal(part[1], full[1]) and np.array_equal(part[2], full[2])
        if want_dist:
            assert np.array_equal(part[3], full[3])
        if want_level:
            assert np.array_equal(part[4], full[4])


@pytest.fixture(scope="module")
def second_pass_scene():
    """B = 1, n_mp = 4097, n_kp = 2048 (SearchInNeighbors' second pass: every neighbour's points
    against the current keyframe). The last point is made to fuse into the last keypoint."""
    s = synthetic_fuse_scene(2048, 4097, 1, seed=300)
    _, idx, _, _, _ = F.fuse_scene(dict(s, ratios=None))
    m = int(np.nonzero((idx[0] >= 0) & (s["kind"] == "plain"))[0][0])    # an accepted point and its keypoint
    j = int(idx[0, m])
    kf = s["kfs"][0]
    last_m, last_j = 4096, 2047
    for a in (s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"]):
        a[[m, last_m]] = a[[last_m, m]]
    s["pair_skip"][:, [m, last_m]] = s["pair_skip"][:, [last_m, m]]
    s["skip"][last_m] = 0
    s["pair_skip"][0, last_m] = 0
    kps, desc = kf.kps.copy(), kf.desc.copy()
    kps[[j, last_j]] = kps[[last_j, j]]
    desc[[j, last_j]] = desc[[last_j, j]]
    s["kfs"] = [ProjFrame(kps, desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy)]
    return s


def test_second_pass_shape_with_the_last_indices_matched(ctx, second_pass_scene):
    s = second_pass_scene
    assert s["points"].shape[0] == 4097 and s["kfs"][0].kps.shape[0] == 2048
    rn, ri, _, _, _ = _parity(ctx, s)
    assert ri[0, 4096] == 2047 and rn[0] > 1000


def test_envelope_and_argument_errors(ctx):
    s = synthetic_fuse_scene(40, 30, 2, seed=400)
    mt = ORBmatcher(0.6, True, ctx=ctx)
    kf = s["kfs"][0]

    def call(kfs, n=None, **over):
        a = dict(s, **over)
        if n is not None:      # n blank points
            a.update(points=np.zeros((n, 3), np.float32), normals=np.zeros((n, 3), np.float32),
                     min_dist=np.ones(n, np.float32), max_dist=np.ones(n, np.float32),
                     mp_desc=np.zeros((n, 32), np.uint8), skip=None, pair_skip=None)
        return mt.Fuse(kfs, a["points"], a["normals"], a["min_dist"], a["max_dist"], a["mp_desc"],
                       a["inv_level_sigma2"], a["th"], a["skip"], a["pair_skip"])

    for kfs, n in (([kf] * 65, 30), ([kf], 65537), ([_blank_like(kf, 65536)], 30)):
        with pytest.raises(OrbHipError) as e:
            call(kfs, n)
        assert e.value.code == -5          # ORBHIP_ERR_UNSUPPORTED
    # an octave out of range, on either side of it, in any keyframe of the call
    for octave in (8, -1):
        bad = _blank_like(kf, 3)
        bad.kps["octave"][1] = octave
        for kfs in ([bad], [kf, bad]):
            with pytest.raises(OrbHipError) as e:
                call(kfs, 30)
            assert e.value.code == -1      # ORBHIP_ERR_ARG
    # keyframes of one call share the scale pyramid
    other_sf = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, scale_factor=1.25)
    other_nl = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, n_levels=7)
    other_log = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy)
    other_log.log_scale_factor = kf.log_scale_factor * 1.01
    for other in (other_sf, other_nl, other_log):
        with pytest.raises(OrbHipError) as e:
            call([kf, other], 30)
        assert e.value.code == -1
    # B = 0 and n = 0 return 0
    nf, idx, dist, lvl = call([], 30)
    assert nf.shape == (0,) and idx.shape == (0, 30)
    nf, idx, dist, lvl = call([kf, kf], 0)
    assert nf.tolist() == [0, 0] and idx.shape == (2, 0)
    rc, nf, _, _, _ = _raw(ctx, dict(s, points=np.zeros((0, 3), np.float32), skip=np.zeros(0, np.uint8)), pair_skip=None)
    assert rc == 0 and nf.tolist() == [0, 0]
    rc, _, _, _, _ = _raw(ctx, dict(s, kfs=[]), pair_skip=None)
    assert rc == 0
    # the envelope itself is accepted
    nf, idx, _, _ = call([kf] * 64, 30)
    assert nf.shape == (64,) and idx.shape == (64, 30)


def test_repeatability_and_a_search_local_points_call_between(ctx):
    """Two identical calls on one context give identical outputs, with calls of other sizes and a
    SearchLocalPoints call between them; that call returns what it returns on a context Fuse never
    ran on."""
    big, small = F.parity_scene(0), synthetic_fuse_scene(65, 33, 1, seed=500)
    p = synthetic_projection_scene(400, 350, seed=11)
    frame = ProjFrame(p["kps"], p["desc"], p["pose_q"], p["pose_t"], p["fx"], p["fy"], p["cx"], p["cy"],
                      claimed=p["claimed"])

    def local(c):
        return ORBmatcher(0.8, True, ctx=c).SearchLocalPoints(frame, p["points"], p["normals"], p["min_dist"],
                                                              p["max_dist"], p["mp_desc"], p["skip"])
    fresh = Context()
    want_local = local(fresh)
    fresh.close()
    first = _library(ctx, big)
    again = _library(ctx, big)
    _library(ctx, small)
    got_local = local(ctx)
    third = _library(ctx, big)
    for other in (again, third):
        for a, b in zip(first, other):
            assert np.array_equal(a, b)
    _assert_equal(first, big["expected"])
    assert got_local[0] == want_local[0] > 0
    for a, b in zip(got_local[1:], want_local[1:]):
        assert np.array_equal(a, b)
    _assert_equal(_library(ctx, small), F.fuse_scene(dict(small, ratios=None)))
