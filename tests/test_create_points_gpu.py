"""orbhip_create_new_map_points and orbhip_triangulate_matches on the GPU against the numpy
restatement (tests/create_points_numpy.py): every output must be EQUAL, the points as raw 32-bit
patterns. The restatement's search is fed the library's own F12 and epipole, as in
tests/test_triangulation_gpu.py."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, OrbHipError, lib
from orb_slam3_ros2_amd.matcher import ORBmatcher, TriKeyFrame
from orb_slam3_ros2_amd.synthetic import (orb_scale_tables, synthetic_new_points_scene,
                                          synthetic_triangulation_scene)

import create_points_numpy as C
import test_create_points as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def assert_same(r, e, what=""):
    """Library result r against restatement result e (diagnostics compared when r has them)."""
    assert r.gated.tolist() == e.gated.tolist(), what
    assert r.nmatches.tolist() == e.nmatches.tolist(), what
    if r.status is not None:
        assert np.array_equal(r.match12, e.match12), what
        bad = np.argwhere(r.status != e.status)
        assert bad.size == 0, f"{what}: status differs at {bad[:5].tolist()}: gpu " \
                              f"{r.status[tuple(bad[:5].T)].tolist()} restatement {e.status[tuple(bad[:5].T)].tolist()}"
        reached = (e.status == 1) | (e.status >= 5)
        assert np.array_equal(bits(r.x3d_all)[reached], bits(e.x3d_all)[reached]), what
        assert not r.x3d_all[~reached].any(), what
    assert r.first.tolist() == e.first.tolist(), what
    assert r.nnew.tolist() == e.nnew.tolist(), what
    assert r.n == e.n, what
    assert r.new_nbr.tolist() == e.new_nbr.tolist() and r.new_idx1.tolist() == e.new_idx1.tolist(), what
    assert r.new_idx2.tolist() == e.new_idx2.tolist(), what
    assert np.array_equal(bits(r.new_x3d), bits(e.new_x3d)), what
    assert (r._nbr[r.n:] == -1).all() and (r._idx1[r.n:] == -1).all() and not r._x3d[r.n:].any(), what


def restate(s, ori, **kw):
    kf1, nbrs = s["kf1"], s["neighbours"]
    geoms = [kf1.geometry(k) for k in nbrs]
    return C.create_new_map_points(kf1, nbrs, s["scale_factors"], s["level_sigma2"], ori, s.get("median_depth"),
                                   far=s.get("far_threshold", 0.0), geoms=geoms, **kw)


def library(ctx, s, ori, diagnostics=True):
    return ORBmatcher(0.6, bool(ori), ctx=ctx).CreateNewMapPoints(
        s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], s.get("median_depth"),
        far_threshold=s.get("far_threshold", 0.0), diagnostics=diagnostics)


def from_matches(ctx, s, match12, diagnostics=True):
    return ORBmatcher(0.6, False, ctx=ctx).TriangulateMatches(
        s["kf1"], s["neighbours"], match12, s["scale_factors"], s["level_sigma2"],
        far_threshold=s.get("far_threshold", 0.0), diagnostics=diagnostics)


ORI = pytest.mark.parametrize("ori", [0, 1])


@ORI
@pytest.mark.parametrize("k", range(len(P.PARITY_SEEDS)))
def test_parity_scene_set(ctx, k, ori):
    """The scenes whose Conditions tests/test_create_points.py asserts; the fused call, then the
    triangulation alone fed the restatement's matches (no gating there: the gated row is empty)."""
    s = P.parity_scene(k)
    e = restate(s, ori)
    assert e.n >= 50 and e.gated.tolist() == [0, 1, 0, 0]
    assert_same(library(ctx, s, ori), e, "fused")
    e2 = C.from_matches(s["kf1"], s["neighbours"], e.match12, s["scale_factors"], s["level_sigma2"],
                        far=s["far_threshold"])
    assert np.array_equal(e2.status, e.status)
    assert_same(from_matches(ctx, s, e.match12), e2, "from matches")


@pytest.mark.parametrize("name", list(P.DIRECT))
def test_direct_cases(ctx, name):
    """Every status, 4, 8 and 9 included, through orbhip_triangulate_matches on one pair."""
    k1, k2, want, kw = P.DIRECT[name]
    e_st, e_x = C.triangulate_pair(C.Camera(k1), C.Camera(k2), k1.kps[0], k2.kps[0], P.SF, P.S2, **kw)
    r = ORBmatcher(0.6, False, ctx=ctx).TriangulateMatches(
        k1, [k2], np.zeros((1, 1), np.int32), P.SF, P.S2, cos_parallax_max=kw.get("cos_max", 0.9998),
        far_threshold=kw.get("far", 0.0), diagnostics=True)
    assert int(r.status[0, 0]) == e_st and e_st in want
    assert np.array_equal(bits(r.x3d_all[0, 0]), bits(e_x))
    assert r.n == int(e_st == 1) and r.nmatches.tolist() == [1]


@ORI
@pytest.mark.parametrize("n1", [1, 63, 64, 65, 257])
def test_size_edges(ctx, n1, ori):
    """n1 x n2 over 1, 63, 64, 65, 257 (the five n2 as five neighbours of one call, a gated one among them)."""
    s = synthetic_new_points_scene(n1, 5, seed=10 + n1, n_nodes=2, n2=[1, 63, 64, 65, 257])
    assert [k.n for k in s["neighbours"]] == [1, 1, 63, 64, 65, 257] and s["kf1"].n == n1
    e = restate(s, ori)
    assert_same(library(ctx, s, ori), e)
    if n1 >= 63:
        assert e.n > 0


@pytest.mark.parametrize("B", [1, 2, 64])
def test_batch_sizes(ctx, B):
    s = synthetic_new_points_scene(40, B, seed=30 + B, n_nodes=2, gated_at=None if B == 64 else 0)
    assert len(s["neighbours"]) == (64 if B == 64 else B + 1)
    e = restate(s, 0)
    assert e.n > 0
    assert_same(library(ctx, s, 0), e)


def _stage_launches(ctx, call):
    """How many times `call` launched the triangulation kernels (profile stage 10)."""
    L = lib()
    assert L.orbhip_profile_stage(ctx.handle, 10) == 0
    try:
        out = call()
    except OrbHipError as err:
        out = err
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(ctx.handle, 0) == 0
    return out, cnt.value


def test_every_neighbour_gated(ctx):
    s = dict(P.parity_scene(0))
    s["median_depth"] = np.full(4, 1e6, np.float32)
    r, launches = _stage_launches(ctx, lambda: library(ctx, s, 0))
    assert launches == 0 and r.n == 0
    assert r.gated.tolist() == [1, 1, 1, 1] and not r.status.any() and (r.match12 == -1).all() and (r.first == -1).all()
    assert_same(r, restate(s, 0))
    _, launches = _stage_launches(ctx, lambda: library(ctx, P.parity_scene(0), 0))
    assert launches == 1                      # the counter does count a call that launches


def test_no_match_at_all(ctx):
    s = synthetic_triangulation_scene(100, 2, seed=22, n_nodes=3, mp_frac=1.0)
    r = library(ctx, s, 0)
    assert r.n == 0 and r.nmatches.tolist() == [0, 0] and not r.status.any() and r.new_nbr.size == 0
    assert_same(r, restate(s, 0))


# ---- the scan of the claim: list positions 255 / 256 / 257 / 1025, inside a neighbour and at a change ----
SPLITS = {255: [(85, 85, 85), (255, 0, 0)], 256: [(100, 100, 56), (256, 0, 0), (64, 192, 0)],
          257: [(256, 1, 0), (100, 100, 57)], 1025: [(1024, 1, 0), (400, 400, 225), (256, 256, 513)]}


@pytest.fixture(scope="module")
def grid_scene():
    """1100 points 4 m in front of KF1, seen exactly by three neighbours 0.3-0.5 m to the side:
    feature i of every keyframe is point i, all at octave 0 (every identity match is accepted); the
    neighbours' last 40 features are at octave 5 instead (their matches fail the scale ratio)."""
    n = 1100
    rng = np.random.default_rng(3)
    pts = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(3.5, 4.5, n)], 1)
    sf, s2 = orb_scale_tables()
    kf1 = P.keyframe([P.proj(p) for p in pts], np.zeros(n, np.int32))
    nbrs = []
    for c in ((0.3, 0.0, 0.0), (-0.4, 0.1, 0.0), (0.1, 0.5, 0.05)):
        octs = np.zeros(n, np.int32)
        octs[-40:] = 5
        nbrs.append(P.keyframe([P.proj(p, c=c) for p in pts], octs, t=P.pose_t(P.IDENT, c)))
    return dict(kf1=kf1, neighbours=nbrs, scale_factors=sf, level_sigma2=s2, perm=rng.permutation(n - 40))


@pytest.mark.parametrize("K,split", [(K, sp) for K, sps in SPLITS.items() for sp in sps])
def test_scan_edges(ctx, grid_scene, K, split):
    s = grid_scene
    n, perm = s["kf1"].n, s["perm"]
    m = np.full((3, n), -1, np.int32)
    at = 0
    for b, cnt in enumerate(split):
        ids = perm[at:at + cnt]
        m[b, ids] = ids                      # accepted, interleaved over idx1
        m[b, n - 40 + 10 * b:n - 40 + 10 * b + 10] = np.arange(n - 40 + 10 * b, n - 30 + 10 * b)   # scale ratio
        at += cnt
    assert at == K
    r = from_matches(ctx, s, m)
    assert r.n == K and r.nnew.tolist() == list(split)
    assert int((r.status == 1).sum()) == K and int((r.status == 11).sum()) == 30
    assert r.new_nbr.tolist() == sorted(r.new_nbr.tolist())
    for b in range(3):
        assert r.new_idx1[r.new_nbr == b].tolist() == sorted(perm[sum(split[:b]):sum(split[:b + 1])].tolist())
    assert r.new_idx2.tolist() == r.new_idx1.tolist()
    if K == 257 or split == (64, 192, 0):    # the restatement on the two smallest layouts (1 ms per pair)
        assert_same(r, C.from_matches(s["kf1"], s["neighbours"], m, s["scale_factors"], s["level_sigma2"]))


def test_optional_outputs(ctx):
    s = P.parity_scene(1)
    full, lean = library(ctx, s, 0), library(ctx, s, 0, diagnostics=False)
    assert lean.status is None and lean.match12 is None and lean.x3d_all is None
    assert lean.n == full.n > 0 and lean.first.tolist() == full.first.tolist()
    assert lean.nnew.tolist() == full.nnew.tolist() and lean.nmatches.tolist() == full.nmatches.tolist()
    assert lean.new_nbr.tolist() == full.new_nbr.tolist() and lean.new_idx1.tolist() == full.new_idx1.tolist()
    assert lean.new_idx2.tolist() == full.new_idx2.tolist() and np.array_equal(bits(lean.new_x3d), bits(full.new_x3d))
    m = full.match12
    a, b = from_matches(ctx, s, m), from_matches(ctx, s, m, diagnostics=False)
    assert a.n == b.n > 0 and np.array_equal(bits(a.new_x3d), bits(b.new_x3d))
    assert a.new_idx1.tolist() == b.new_idx1.tolist() and a.new_nbr.tolist() == b.new_nbr.tolist()


def test_errors_before_any_launch(ctx):
    s = synthetic_triangulation_scene(40, 1, seed=26, n_nodes=2)
    k1, k2, sf, s2 = s["kf1"], s["neighbours"][0], s["scale_factors"], s["level_sigma2"]
    mt = ORBmatcher(0.6, False, ctx=ctx)

    def blank(n):
        return TriKeyFrame(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.ones(n),
                           np.zeros(n, np.uint8), k2.pose_q, k2.pose_t, k2.fx, k2.fy, k2.cx, k2.cy)
    bad = blank(3)
    bad.kps["octave"][1] = len(sf)
    none = np.full((1, k1.n), -1, np.int32)
    past = none.copy()
    past[0, 5] = k2.n
    below = none.copy()
    below[0, 7] = -2
    calls = [(-5, lambda: mt.CreateNewMapPoints(blank(2049), [k2], sf, s2)),
             (-5, lambda: mt.CreateNewMapPoints(k1, [k2, blank(2049)], sf, s2)),
             (-5, lambda: mt.CreateNewMapPoints(k1, [k2] * 65, sf, s2)),
             (-5, lambda: mt.TriangulateMatches(k1, [k2] * 65, np.full((65, k1.n), -1, np.int32), sf, s2)),
             (-5, lambda: mt.TriangulateMatches(blank(2049), [k2], np.full((1, 2049), -1, np.int32), sf, s2)),
             (-1, lambda: mt.CreateNewMapPoints(k1, [k2, bad], sf, s2)),
             (-1, lambda: mt.CreateNewMapPoints(bad, [k2], sf, s2)),
             (-1, lambda: mt.TriangulateMatches(k1, [bad], none, sf, s2)),
             (-1, lambda: mt.TriangulateMatches(k1, [k2], past, sf, s2)),
             (-1, lambda: mt.TriangulateMatches(k1, [k2], below, sf, s2))]
    for code, call in calls:
        err, launches = _stage_launches(ctx, call)
        assert isinstance(err, OrbHipError) and err.code == code and launches == 0
    past[0, 5] = k2.n - 1                     # the last feature itself is accepted as an index
    assert mt.TriangulateMatches(k1, [k2], past, sf, s2).nmatches.tolist() == [1]
    r = mt.CreateNewMapPoints(blank(2048), [k2] * 64, sf, s2)     # the envelope itself
    assert r.n == 0 and r.first.shape == (2048,)
    assert mt.CreateNewMapPoints(k1, [], sf, s2).n == 0 and mt.CreateNewMapPoints(blank(0), [k2], sf, s2).n == 0


def test_search_before_and_after(ctx):
    """SearchForTriangulation on the same context (the same staging block) around the new calls
    returns what it returns on a fresh context."""
    s, small = P.parity_scene(2), synthetic_triangulation_scene(65, 1, seed=27, n_nodes=2)
    mt = ORBmatcher(0.6, True, ctx=ctx)

    def search(m, sc):
        return m.SearchForTriangulation(sc["kf1"], sc["neighbours"], sc["scale_factors"], sc["level_sigma2"])
    fresh = Context()
    want = [search(ORBmatcher(0.6, True, ctx=fresh), sc) for sc in (s, small)]
    fresh.close()
    before = search(mt, s)
    new1 = library(ctx, s, 1)
    mid = search(mt, small)
    new2 = from_matches(ctx, s, new1.match12)
    after = search(mt, s)
    for got, w in ((before, want[0]), (mid, want[1]), (after, want[0])):
        assert got[0].tolist() == w[0].tolist() and np.array_equal(got[1], w[1])
    assert new1.n > 0 and new2.n == new1.n and np.array_equal(new1.match12[[0, 2, 3]], want[0][1][[0, 2, 3]])
