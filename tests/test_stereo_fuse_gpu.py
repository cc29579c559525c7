"""orbhip_fuse_stereo on the GPU against the numpy restatement (tests/stereo_fuse_numpy.py):
best_idx, best_dist, level, nfused and the return value must be EQUAL, for every pair, with no
tolerance and no pair left out. The scenes keep PredictScale's ceil 1e-3 away from a step
(tests/test_stereo_fuse.py checks that on the CPU), which is all that separates the device's logf
from numpy's; every other operation is one IEEE fp32 operation on both sides."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, LocalPointsC, OrbHipError, StereoViewC, lib, ptr
from orb_slam3_ros2_amd.matcher import ORBmatcher, ProjFrame
from orb_slam3_ros2_amd.synthetic import synthetic_fuse_scene, synthetic_stereo_fuse_scene

import fuse_numpy as F
import stereo_fuse_numpy as SF

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _library(ctx, s, **over):
    """ORBmatcher.Fuse: it dispatches on the keyframes' u_right."""
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
    want = s["expected"] if "expected" in s and not over else SF.fuse_stereo_scene(dict(s, ratios=None), **over)
    _assert_equal(_library(ctx, s, **over), want)
    return want


def _raw(ctx, s, pair_skip="scene", want_dist=True, want_level=True, edit=None):
    """The C entry point itself: (return value, nfused, best_idx, best_dist or None, level or None).
    edit(views): changes the orbhip_stereo_view array before the call."""
    kfs = list(s["kfs"])
    B, n = len(kfs), s["points"].shape[0]
    views = (StereoViewC * max(B, 1))(*[k.to_c_stereo() for k in kfs])
    if edit:
        edit(views)
    sk = None if s["skip"] is None else np.ascontiguousarray(s["skip"], np.uint8)
    lc = LocalPointsC(n, ptr(s["points"]), ptr(s["normals"]), ptr(s["min_dist"]), ptr(s["max_dist"]),
                      ptr(s["mp_desc"]), ptr(sk))
    ps = np.ascontiguousarray(s["pair_skip"], np.uint8) if isinstance(pair_skip, str) else pair_skip
    nf = np.full(B, -7, np.int32)
    idx = np.full((B, n), -7, np.int32)
    dist = np.full((B, n), -7, np.int32) if want_dist else None
    lvl = np.full((B, n), -7, np.int32) if want_level else None
    rc = lib().orbhip_fuse_stereo(ctx.handle, views, B, ctypes.byref(lc), ptr(ps), ptr(s["inv_level_sigma2"]), s["th"],
                                  ptr(idx), ptr(dist), ptr(lvl), ptr(nf))
    return rc, nf, idx, dist, lvl


def _stage_launches(ctx, call):
    """How many times `call` launched the Fuse kernels (profile stage 8)."""
    L = lib()
    assert L.orbhip_profile_stage(ctx.handle, 8) == 0
    try:
        out = call()
    except OrbHipError as err:
        out = err
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(ctx.handle, 0) == 0
    return out, cnt.value


@pytest.mark.parametrize("k", range(len(SF.PARITY_SCENES)))
def test_parity_scene_set(ctx, k):
    """n_kp = 300, n_mp = 300, B = 3: the scenes whose conditions tests/test_stereo_fuse.py asserts,
    through the mirror and the bare C call. The monocular entry point on the same keyframes without
    u_right gives the monocular restatement, which differs."""
    s = SF.parity_scene(k)
    rn = _parity(ctx, s)[0]
    assert (rn * 4 >= 300).all()
    rc, nf, idx, dist, lvl = _raw(ctx, s)
    assert rc == int(rn.sum())
    _assert_equal((nf, idx, dist, lvl), s["expected"])
    mono = _library(ctx, s, kfs=s["mono_kfs"])
    _assert_equal(mono, F.fuse_scene(dict(s, ratios=None), kfs=s["mono_kfs"]))
    assert not np.array_equal(mono[1], idx)


CASES = SF.direct_cases()


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_direct_case(ctx, c):
    """Every direct case of tests/test_stereo_fuse.py on the device, under both rules."""
    mt = ORBmatcher(0.6, True, ctx=ctx)
    inv_s2 = F.parity_scene(0)["inv_level_sigma2"]
    nf, idx, dist, lvl = mt.Fuse([c["kf"]], *SF.direct_args(c), inv_s2, 3.0)
    assert (int(idx[0, 0]), int(dist[0, 0]), int(lvl[0, 0])) == c["want"] + (c["octave"],)
    assert nf.tolist() == [int(c["want"][0] == 0)]
    nf, idx, dist, lvl = mt.Fuse([SF.mono_keyframe(c["kf"])], *SF.direct_args(c), inv_s2, 3.0)
    assert (int(idx[0, 0]), int(dist[0, 0])) == c["mono"]


@pytest.mark.parametrize("n_mp", [1, 63, 64, 65, 257])
def test_point_count_edges(ctx, n_mp):
    """mps->n at the tile of 64 points against keyframes of 1, 63, 64, 65 and 257 keypoints, the five
    as five keyframes of one call."""
    s = synthetic_stereo_fuse_scene([1, 63, 64, 65, 257], n_mp, 5, seed=100 + n_mp)
    assert [k.kps.shape[0] for k in s["kfs"]] == [1, 63, 64, 65, 257] and s["points"].shape[0] == n_mp
    rn, _, _, _, cnt = _parity(ctx, s)
    if n_mp >= 63:
        assert rn[1:].min() > 0 and cnt["cand_stereo"] > 0 and cnt["cand_mono"] > 0


@pytest.mark.parametrize("B,n_kp,n_mp", [(1, 200, 150), (2, 200, 150), (64, 40, 60)])
def test_batch_sizes(ctx, B, n_kp, n_mp):
    s = synthetic_stereo_fuse_scene(n_kp, n_mp, B, seed=200 + B)
    rn, _, _, _, cnt = _parity(ctx, s)
    assert rn.shape == (B,) and (rn > 0).all() and cnt["cand_stereo"] > 0


def _blank_like(kf, n=0, **stereo):
    a = dict(u_right=np.full(n, -1.0, f32), bf=kf.bf, b=kf.b)
    a.update(stereo)
    return ProjFrame(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx,
                     kf.cy, **a)


def test_keyframe_with_no_keypoints_between_two(ctx):
    s = SF.parity_scene(1)
    kfs = [s["kfs"][0], _blank_like(s["kfs"][1]), s["kfs"][2]]
    rn, ri, rd, _, _ = _parity(ctx, s, kfs=kfs)
    assert rn[1] == 0 and (ri[1] == -1).all() and (rd[1] == 256).all() and rn[0] > 0 and rn[2] > 0
    e = s["expected"]
    assert np.array_equal(ri[0], e[1][0]) and np.array_equal(ri[2], e[1][2])     # the neighbours are unaffected


# ---- reduction on the device ----

def test_every_ur_minus_one_equals_the_monocular_entry_point(ctx):
    """orbhip_fuse_stereo with every u_right = -1 returns exactly what orbhip_fuse returns."""
    s = F.parity_scene(0)
    mono = _library(ctx, s)
    kfs = [SF.stereo_keyframe(kf, np.full(kf.kps.shape[0], -1.0, f32), 30.0, 1e-6) for kf in s["kfs"]]
    stereo = _library(ctx, s, kfs=kfs)
    for a, b in zip(mono, stereo):
        assert np.array_equal(a, b)
    _assert_equal(stereo, s["expected"])
    rc, nf, idx, dist, lvl = _raw(ctx, dict(s, kfs=kfs))
    assert rc == int(mono[0].sum()) > 0
    _assert_equal((nf, idx, dist, lvl), s["expected"])


def test_monocular_calls_around_stereo_calls_on_one_context(ctx):
    """The staging block is shared: orbhip_fuse before, between and after stereo calls of other sizes
    returns what it returns on a fresh context, and so does the stereo call."""
    big, small = F.parity_scene(0), synthetic_fuse_scene(65, 33, 1, seed=500)
    st_big, st_small = SF.parity_scene(2), synthetic_stereo_fuse_scene(70, 500, 2, seed=501)
    fresh = Context()
    want = [_library(fresh, x) for x in (big, small, st_big, st_small)]
    fresh.close()
    order = [0, 2, 1, 3, 0, 3, 2, 1]
    for i in order:
        got = _library(ctx, (big, small, st_big, st_small)[i])
        for a, b in zip(got, want[i]):
            assert np.array_equal(a, b), i
    _assert_equal(want[0], big["expected"])
    _assert_equal(want[2], st_big["expected"])


# ---- errors, envelope, optional outputs ----

def test_errors_before_any_launch(ctx):
    s = synthetic_stereo_fuse_scene(40, 30, 2, seed=400)
    kf = s["kfs"][0]

    def null_ur(v):
        v[1].u_right = None

    def bf_zero(v):
        v[0].bf = 0.0

    def bf_negative(v):
        v[1].bf = -1.0

    def bf_nan(v):
        v[0].bf = float("nan")

    def b_zero(v):
        v[1].b = 0.0

    def b_negative(v):
        v[0].b = -0.08

    for edit in (null_ur, bf_zero, bf_negative, bf_nan, b_zero, b_negative):
        out, launches = _stage_launches(ctx, lambda: _raw(ctx, s, edit=edit))
        assert out[0] == -1 and launches == 0, edit.__name__          # ORBHIP_ERR_ARG
        assert (out[2] == -7).all()                                    # nothing was written
    # a null u_right is fine for a keyframe without keypoints
    out, launches = _stage_launches(ctx, lambda: _raw(ctx, dict(s, kfs=[kf, _blank_like(kf)]), pair_skip=None,
                                                      edit=null_ur))
    assert out[0] >= 0 and launches == 1

    def blank_points(n):
        return dict(points=np.zeros((n, 3), f32), normals=np.zeros((n, 3), f32), min_dist=np.ones(n, f32),
                    max_dist=np.ones(n, f32), mp_desc=np.zeros((n, 32), np.uint8), skip=None, pair_skip=None)
    mt = ORBmatcher(0.6, True, ctx=ctx)

    def call(kfs, n):
        a = dict(s, **blank_points(n))
        return mt.Fuse(kfs, a["points"], a["normals"], a["min_dist"], a["max_dist"], a["mp_desc"],
                       a["inv_level_sigma2"], a["th"], a["skip"], a["pair_skip"])
    # the envelope of orbhip_fuse
    for kfs, n in (([kf] * 65, 30), ([kf], 65537), ([_blank_like(kf, 65536)], 30)):
        err, launches = _stage_launches(ctx, lambda: call(kfs, n))
        assert isinstance(err, OrbHipError) and err.code == -5 and launches == 0      # ORBHIP_ERR_UNSUPPORTED
    for octave in (8, -1):
        bad = _blank_like(kf, 3)
        bad.kps["octave"][1] = octave
        err, launches = _stage_launches(ctx, lambda: call([kf, bad], 30))
        assert isinstance(err, OrbHipError) and err.code == -1 and launches == 0
    other_nl = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, n_levels=7,
                         u_right=kf.u_right, bf=kf.bf, b=kf.b)
    err, launches = _stage_launches(ctx, lambda: call([kf, other_nl], 30))
    assert isinstance(err, OrbHipError) and err.code == -1 and launches == 0
    # B = 0 and n = 0 return 0 without a launch; the envelope itself is accepted
    out, launches = _stage_launches(ctx, lambda: _raw(ctx, dict(s, kfs=[]), pair_skip=None))
    assert out[0] == 0 and launches == 0
    out, launches = _stage_launches(ctx, lambda: _raw(ctx, dict(s, **blank_points(0)), pair_skip=None))
    assert out[0] == 0 and out[1].tolist() == [0, 0] and launches == 0
    (nf, idx, _, _), launches = _stage_launches(ctx, lambda: call([kf] * 64, 30))
    assert nf.shape == (64,) and idx.shape == (64, 30) and launches == 1


def test_null_pair_skip_equals_zeros_and_optional_outputs(ctx):
    s = SF.parity_scene(0)
    B, n = 3, s["points"].shape[0]
    none = _raw(ctx, s, pair_skip=None)
    zeros = _raw(ctx, s, pair_skip=np.zeros((B, n), np.uint8))
    assert none[0] == zeros[0] > 0
    for a, b in zip(none[1:], zeros[1:]):
        assert np.array_equal(a, b)
    _assert_equal(none[1:], SF.fuse_stereo_scene(dict(s, ratios=None), pair_skip=None))
    # best_dist and level are optional: best_idx, nfused and the return value do not depend on them
    full = _raw(ctx, s)
    for want_dist, want_level in ((False, False), (True, False), (False, True)):
        part = _raw(ctx, s, want_dist=want_dist, want_level=want_level)
        assert part[0] == full[0] and np.array_equal(part[1], full[1]) and np.array_equal(part[2], full[2])
        if want_dist:
            assert np.array_equal(part[3], full[3])
        if want_level:
            assert np.array_equal(part[4], full[4])
