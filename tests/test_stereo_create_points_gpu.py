"""orbhip_search_for_triangulation_stereo, orbhip_create_new_map_points_stereo and
orbhip_triangulate_matches_stereo on the GPU against the numpy restatement
(tests/stereo_create_points_numpy.py): every output must be EQUAL, the points as raw 32-bit
patterns, `source` included, no pair left out (no operation of the rule is not bit-pinned). The
restatement's search is fed the library's own F12 and epipole, as in tests/test_create_points_gpu.py."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, NewPointsC, OrbHipError, TriParamsC, TriStereoKeyFrameC, lib, ptr
from orb_slam3_ros2_amd.matcher import NewPoints, ORBmatcher, TriKeyFrame
from orb_slam3_ros2_amd.synthetic import synthetic_stereo_new_points_scene

import create_points_numpy as C
import stereo_create_points_numpy as S
import test_create_points as P
import test_stereo_create_points as SP
from test_create_points_gpu import assert_same as assert_same_mono, bits

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def assert_same(r, e, what=""):
    assert_same_mono(r, e, what)
    if r.source is not None:
        bad = np.argwhere(r.source != e.source)
        assert bad.size == 0, f"{what}: source differs at {bad[:5].tolist()}"


def restate(s, ori):
    kf1, nbrs = s["kf1"], s["neighbours"]
    geoms = [kf1.geometry(k) for k in nbrs]
    return S.create_new_map_points(kf1, nbrs, s["scale_factors"], s["level_sigma2"], ori,
                                   far=s.get("far_threshold", 0.0), geoms=geoms)


def library(ctx, s, ori, diagnostics=True, mono=False):
    kf1, nbrs = (s["mono_kf1"], s["mono_neighbours"]) if mono else (s["kf1"], s["neighbours"])
    return ORBmatcher(0.6, bool(ori), ctx=ctx).CreateNewMapPoints(
        kf1, nbrs, s["scale_factors"], s["level_sigma2"], far_threshold=s.get("far_threshold", 0.0),
        diagnostics=diagnostics)


def from_matches(ctx, s, match12, diagnostics=True):
    return ORBmatcher(0.6, False, ctx=ctx).TriangulateMatches(
        s["kf1"], s["neighbours"], match12, s["scale_factors"], s["level_sigma2"],
        far_threshold=s.get("far_threshold", 0.0), diagnostics=diagnostics)


def search(ctx, s, ori, mono=False):
    kf1, nbrs = (s["mono_kf1"], s["mono_neighbours"]) if mono else (s["kf1"], s["neighbours"])
    return ORBmatcher(0.6, bool(ori), ctx=ctx).SearchForTriangulation(kf1, nbrs, s["scale_factors"], s["level_sigma2"])


def _stage_launches(ctx, call, stage):
    L = lib()
    assert L.orbhip_profile_stage(ctx.handle, stage) == 0
    try:
        out = call()
    except OrbHipError as err:
        out = err
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(ctx.handle, 0) == 0
    return out, cnt.value


ORI = pytest.mark.parametrize("ori", [0, 1])


@ORI
@pytest.mark.parametrize("k", range(len(SP.PARITY_SEEDS)))
def test_parity_scene_set(ctx, k, ori):
    """The scenes whose conditions tests/test_stereo_create_points.py asserts: the fused call, the
    triangulation alone fed the restatement's matches, and the search alone."""
    s = SP.parity_scene(k)
    e = restate(s, ori)
    assert e.n >= 50 and e.gated.tolist() == [0, 1, 0, 0]
    assert_same(library(ctx, s, ori), e, "fused")
    e2 = S.from_matches(s["kf1"], s["neighbours"], e.match12, s["scale_factors"], s["level_sigma2"],
                        far=s["far_threshold"])
    assert np.array_equal(e2.status, e.status) and np.array_equal(e2.source, e.source)
    assert_same(from_matches(ctx, s, e.match12), e2, "from matches")
    # the search alone does not gate: the gated neighbour's row is searched too
    geoms = [s["kf1"].geometry(x) for x in s["neighbours"]]
    nm, m12, _ = S.search_for_triangulation(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], ori, geoms)
    gn, gm = search(ctx, s, ori)
    assert gn.tolist() == nm.tolist() and np.array_equal(gm, m12)
    assert np.array_equal(m12[[0, 2, 3]], e.match12[[0, 2, 3]])
    # and it differs from the monocular search on the same keyframes (the epipole exclusion)
    assert not np.array_equal(search(ctx, s, ori, mono=True)[1], gm)


@pytest.mark.parametrize("name", list(SP.DIRECT))
def test_direct_cases(ctx, name):
    """Every CPU direct case through orbhip_triangulate_matches_stereo on one pair."""
    k1, k2, want, source, mono, kw = SP.DIRECT[name]
    r = ORBmatcher(0.6, False, ctx=ctx).TriangulateMatches(k1, [k2], np.zeros((1, 1), np.int32), SP.SF, SP.S2,
                                                          diagnostics=True, **kw)
    e_st, e_x, e_src, _ = SP.run_direct(name)
    assert (int(r.status[0, 0]), int(r.source[0, 0])) == (e_st, e_src) == (want, source)
    assert np.array_equal(bits(r.x3d_all[0, 0]), bits(e_x))
    assert r.n == int(want == 1)
    m = ORBmatcher(0.6, False, ctx=ctx).TriangulateMatches(S.without_stereo(k1), [S.without_stereo(k2)],
                                                          np.zeros((1, 1), np.int32), SP.SF, SP.S2, diagnostics=True, **kw)
    assert int(m.status[0, 0]) == mono and m.source is None


def test_epipole_radius_pair_and_mb_gate(ctx):
    Pt, c2 = np.array([0.004, 0.002, 4.0]), (0.0, 0.0, 0.5)
    p1, p2 = P.proj(Pt), P.proj(Pt, c=c2)
    k1m, k2m = P.keyframe([p1], [0]), P.keyframe([p2], [0], t=P.pose_t(P.IDENT, c2))
    mt = ORBmatcher(0.6, False, ctx=ctx)
    assert mt.SearchForTriangulation(k1m, [k2m], SP.SF, SP.S2)[0].tolist() == [0]
    k1 = S.with_stereo(k1m, [SP.right(p1, 4.0)], [4.0], SP.BF, SP.B_ST)
    for k2 in (S.all_mono(k2m, SP.BF, SP.B_ST), S.with_stereo(k2m, [SP.right(p2, 3.5)], [3.5], SP.BF, SP.B_ST)):
        nm, m = mt.SearchForTriangulation(k1, [k2], SP.SF, SP.S2)
        assert nm.tolist() == [1] and m.tolist() == [[0]]
    nm, m = mt.SearchForTriangulation(S.all_mono(k1m, SP.BF, SP.B_ST), [k2], SP.SF, SP.S2)     # feature 2 alone is stereo
    assert nm.tolist() == [1]
    assert mt.SearchForTriangulation(S.all_mono(k1m), [S.all_mono(k2m)], SP.SF, SP.S2)[0].tolist() == [0]
    # the mb gate on both sides of baseline == b (0.5 exactly)
    for b, gated in ((0.5, 0), (float(np.nextafter(f32(0.5), f32(1))), 1), (float(np.nextafter(f32(0.5), f32(0))), 0)):
        r = mt.CreateNewMapPoints(k1, [S.with_stereo(k2m, [-1.0], [-1.0], SP.BF, b)], SP.SF, SP.S2, diagnostics=True)
        assert r.gated.tolist() == [gated] and r.nmatches.tolist() == [1 - gated]


@ORI
@pytest.mark.parametrize("n1", [1, 63, 64, 65, 257])
def test_size_edges(ctx, n1, ori):
    """n1 x n2 over 1, 63, 64, 65, 257 (the five n2 as five neighbours of one call, a gated one among them)."""
    s = synthetic_stereo_new_points_scene(n1, 5, seed=10 + n1, n_nodes=2, n2=[1, 63, 64, 65, 257])
    assert [k.n for k in s["neighbours"]] == [1, 1, 63, 64, 65, 257] and s["kf1"].n == n1
    e = restate(s, ori)
    assert_same(library(ctx, s, ori), e)
    if n1 >= 63:
        assert e.n > 0 and (e.source > 1).any()


@pytest.mark.parametrize("B", [1, 2, 64])
def test_batch_sizes(ctx, B):
    s = synthetic_stereo_new_points_scene(40, B, seed=30 + B, n_nodes=2, gated_at=None if B == 64 else 0)
    assert len(s["neighbours"]) == (64 if B == 64 else B + 1)
    e = restate(s, 0)
    assert e.n > 0
    assert_same(library(ctx, s, 0), e)


def test_every_neighbour_gated(ctx):
    s = dict(SP.parity_scene(0))
    s["neighbours"] = [S.with_stereo(k, k.u_right, k.depth, k.bf, 10.0) for k in s["neighbours"]]
    r, launches = _stage_launches(ctx, lambda: library(ctx, s, 0), 10)
    assert launches == 0 and r.n == 0
    assert r.gated.tolist() == [1, 1, 1, 1] and not r.status.any() and (r.match12 == -1).all() and not r.source.any()
    _, launches = _stage_launches(ctx, lambda: library(ctx, SP.parity_scene(0), 0), 10)
    assert launches == 1


# ---- reduction on the device ----
def test_no_stereo_feature_equals_the_monocular_entry_points(ctx):
    """Every u_right = -1 and a tiny b: exactly what the monocular entry points return (no median_depth)."""
    s = P.parity_scene(0)
    st = dict(s, kf1=S.all_mono(s["kf1"]), neighbours=[S.all_mono(k) for k in s["neighbours"]])
    mt = ORBmatcher(0.6, True, ctx=ctx)
    a = mt.CreateNewMapPoints(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"],
                              far_threshold=s["far_threshold"], diagnostics=True)
    b = library(ctx, st, 1)
    assert a.n == b.n > 0 and not b.gated.any()
    assert_same_mono(b, a, "fused")
    assert np.array_equal(b.source, ((a.status == 1) | (a.status >= 4)).astype(np.uint8))
    sa = mt.SearchForTriangulation(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"])
    sb = mt.SearchForTriangulation(st["kf1"], st["neighbours"], s["scale_factors"], s["level_sigma2"])
    assert sa[0].tolist() == sb[0].tolist() and np.array_equal(sa[1], sb[1])
    ta = mt.TriangulateMatches(s["kf1"], s["neighbours"], a.match12, s["scale_factors"], s["level_sigma2"],
                               far_threshold=s["far_threshold"], diagnostics=True)
    tb = from_matches(ctx, dict(st, far_threshold=s["far_threshold"]), a.match12)
    assert_same_mono(tb, ta, "from matches")


def test_monocular_calls_around_stereo_calls_on_one_context(ctx):
    """The staging block is shared: the monocular entry points before, between and after stereo
    calls return what they return on a fresh context."""
    s, st = P.parity_scene(2), SP.parity_scene(1)
    small = synthetic_stereo_new_points_scene(65, 1, seed=27, n_nodes=2)

    def mono(c):
        mt = ORBmatcher(0.6, True, ctx=c)
        a = mt.CreateNewMapPoints(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], s["median_depth"],
                                  far_threshold=s["far_threshold"], diagnostics=True)
        return a, mt.SearchForTriangulation(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"])
    fresh = Context()
    want, want_search = mono(fresh)
    want_st = library(fresh, st, 0)
    fresh.close()
    first = mono(ctx)
    got_st = library(ctx, st, 0)
    library(ctx, small, 1)
    search(ctx, st, 1)
    second = mono(ctx)
    from_matches(ctx, st, got_st.match12)
    third = mono(ctx)
    for a, sr in (first, second, third):
        assert_same_mono(a, want)
        assert sr[0].tolist() == want_search[0].tolist() and np.array_equal(sr[1], want_search[1])
    assert_same(got_st, want_st)
    assert_same(library(ctx, st, 0), want_st)


# ---- errors, envelope, optional outputs ----
def _raw_create(ctx, s, edit=None, what="create", match12=None):
    """The C entry points themselves, with the orbhip_tri_stereo_keyframe structs editable."""
    kf1, nbrs = s["kf1"], list(s["neighbours"])
    B, n1 = len(nbrs), kf1.n
    sf, s2 = np.ascontiguousarray(s["scale_factors"], f32), np.ascontiguousarray(s["level_sigma2"], f32)
    arr = (TriStereoKeyFrameC * max(B, 1))(*[k.to_c_stereo() for k in nbrs])
    c1 = kf1.to_c_stereo()
    if edit:
        edit(c1, arr)
    r = NewPoints(B, n1, True, True)
    out = NewPointsC(ptr(r.match12), ptr(r.nmatches), ptr(r.gated), ptr(r.status), ptr(r.x3d_all), ptr(r.first),
                     ptr(r.nnew), ptr(r._nbr), ptr(r._idx1), ptr(r._idx2), ptr(r._x3d))
    prm = TriParamsC(0.9998, float(f32(1.5) * sf[1]), 0.0)
    if what == "search":
        nm, m = np.zeros(B, np.int32), np.full((B, n1), -1, np.int32)
        return lib().orbhip_search_for_triangulation_stereo(ctx.handle, ctypes.byref(c1), arr, B, ptr(sf), ptr(s2),
                                                            sf.shape[0], 0, ptr(m), ptr(nm))
    if what == "matches":
        return lib().orbhip_triangulate_matches_stereo(ctx.handle, ctypes.byref(c1), arr, B, ptr(match12), ptr(sf),
                                                       ptr(s2), sf.shape[0], ctypes.byref(prm), ctypes.byref(out),
                                                       ptr(r.source))
    return lib().orbhip_create_new_map_points_stereo(ctx.handle, ctypes.byref(c1), arr, B, ptr(sf), ptr(s2), sf.shape[0],
                                                     0, ctypes.byref(prm), ctypes.byref(out), ptr(r.source))


def test_errors_before_any_launch(ctx):
    s = synthetic_stereo_new_points_scene(40, 1, seed=26, n_nodes=2, gated_at=None)
    k1, k2, sf, s2 = s["kf1"], s["neighbours"][0], s["scale_factors"], s["level_sigma2"]
    none = np.full((1, k1.n), -1, np.int32)

    def null_ur1(c1, arr):
        c1.u_right = None

    def null_depth2(c1, arr):
        arr[0].depth = None

    def bf_zero(c1, arr):
        arr[0].bf = 0.0

    def b_negative(c1, arr):
        c1.b = -0.08

    def b_nan(c1, arr):
        arr[0].b = float("nan")

    for edit in (null_ur1, null_depth2, bf_zero, b_negative, b_nan):
        for what, stage in (("create", 7), ("create", 10), ("search", 7), ("matches", 10)):
            rc, launches = _stage_launches(ctx, lambda: _raw_create(ctx, s, edit, what, none), stage)
            assert rc == -1 and launches == 0, (edit.__name__, what)
    mt = ORBmatcher(0.6, False, ctx=ctx)

    def blank(n):
        return TriKeyFrame(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.ones(n),
                           np.zeros(n, np.uint8), k2.pose_q, k2.pose_t, k2.fx, k2.fy, k2.cx, k2.cy,
                           u_right=np.full(n, -1.0, f32), depth=np.full(n, -1.0, f32), bf=k2.bf, b=k2.b)
    bad = blank(3)
    bad.kps["octave"][1] = len(sf)
    past = none.copy()
    past[0, 5] = k2.n
    calls = [(-5, lambda: mt.CreateNewMapPoints(blank(2049), [k2], sf, s2)),
             (-5, lambda: mt.CreateNewMapPoints(k1, [k2, blank(2049)], sf, s2)),
             (-5, lambda: mt.CreateNewMapPoints(k1, [k2] * 65, sf, s2)),
             (-5, lambda: mt.SearchForTriangulation(k1, [k2] * 65, sf, s2)),
             (-5, lambda: mt.TriangulateMatches(k1, [k2] * 65, np.full((65, k1.n), -1, np.int32), sf, s2)),
             (-1, lambda: mt.CreateNewMapPoints(k1, [k2, bad], sf, s2)),
             (-1, lambda: mt.SearchForTriangulation(bad, [k2], sf, s2)),
             (-1, lambda: mt.TriangulateMatches(k1, [k2], past, sf, s2))]
    for code, call in calls:
        for stage in (7, 10):
            err, launches = _stage_launches(ctx, call, stage)
            assert isinstance(err, OrbHipError) and err.code == code and launches == 0
    r = mt.CreateNewMapPoints(blank(2048), [k2] * 64, sf, s2)     # the envelope itself
    assert r.n == 0 and r.first.shape == (2048,)
    assert mt.CreateNewMapPoints(k1, [], sf, s2).n == 0 and mt.CreateNewMapPoints(blank(0), [k2], sf, s2).n == 0


def test_optional_outputs(ctx):
    s = SP.parity_scene(1)
    full, lean = library(ctx, s, 0), library(ctx, s, 0, diagnostics=False)
    assert lean.status is None and lean.match12 is None and lean.x3d_all is None and lean.source is None
    assert lean.n == full.n > 0 and lean.first.tolist() == full.first.tolist()
    assert lean.nnew.tolist() == full.nnew.tolist() and lean.nmatches.tolist() == full.nmatches.tolist()
    assert lean.new_nbr.tolist() == full.new_nbr.tolist() and lean.new_idx1.tolist() == full.new_idx1.tolist()
    assert lean.new_idx2.tolist() == full.new_idx2.tolist() and np.array_equal(bits(lean.new_x3d), bits(full.new_x3d))
    a, b = from_matches(ctx, s, full.match12), from_matches(ctx, s, full.match12, diagnostics=False)
    assert a.n == b.n > 0 and np.array_equal(bits(a.new_x3d), bits(b.new_x3d))
