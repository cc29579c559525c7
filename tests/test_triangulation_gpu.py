"""orbhip_search_for_triangulation on the GPU against the numpy restatement
(tests/triangulation_numpy.py): match indices and counts must be EQUAL. The restatement is fed the
library's own F12 and epipole (orbhip_triangulation_geometry, itself bit-exact with the restatement:
tests/test_triangulation.py), so every fp32 comparison of the walk is reproduced bit for bit."""
import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, OrbHipError
from orb_slam3_ros2_amd.matcher import ORBmatcher, TriKeyFrame
from orb_slam3_ros2_amd.synthetic import synthetic_triangulation_scene

import triangulation_numpy as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _library(ctx, kf1, nbrs, sf, s2, ori):
    return ORBmatcher(0.6, bool(ori), ctx=ctx).SearchForTriangulation(kf1, nbrs, sf, s2)


def _parity(ctx, kf1, nbrs, sf, s2, ori):
    """Runs both, asserts equality, returns the restatement's (nmatches, match12, counters)."""
    geoms = [kf1.geometry(k) for k in nbrs]
    rn, rm, cnt, _ = T.search_for_triangulation(kf1, nbrs, sf, s2, ori, geoms)
    gn, gm = _library(ctx, kf1, nbrs, sf, s2, ori)
    assert gm.shape == (len(nbrs), kf1.n) and gn.shape == (len(nbrs),)
    bad = np.argwhere(gm != rm)
    assert bad.size == 0, f"{len(bad)} entries differ, first (pair, idx1) {bad[:5].tolist()}: " \
                          f"gpu {gm[tuple(bad[:5].T)].tolist()} restatement {rm[tuple(bad[:5].T)].tolist()}"
    assert gn.tolist() == rn.tolist()
    assert gn.tolist() == (gm >= 0).sum(1).tolist()
    return rn, rm, cnt


def _scene_parity(ctx, s, ori):
    return _parity(ctx, s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], ori)


ORI = pytest.mark.parametrize("ori", [0, 1])


@ORI
@pytest.mark.parametrize("k", range(len(T.PARITY_SCENES)))
def test_parity_scene_set(ctx, k, ori):
    """n = 300, B = 3: the scenes whose Conditions tests/test_triangulation.py asserts (every gate
    fires, ties, shared targets, orientation pruning)."""
    rn, rm, cnt = _scene_parity(ctx, T.parity_scene(k), ori)
    assert (rn > 0).all()
    if ori:   # k_tri_search's rotation filter removes matches of every pair
        s = T.parity_scene(k)
        geoms = [s["kf1"].geometry(x) for x in s["neighbours"]]
        off = T.search_for_triangulation(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 0, geoms)[0]
        assert (rn < off).all()


@ORI
@pytest.mark.parametrize("n1", [1, 63, 64, 65, 257])
def test_size_edges(ctx, n1, ori):
    """n1 x n2 over 1, 63, 64, 65, 257 (the five n2 as five neighbours of one call), two nodes."""
    s = synthetic_triangulation_scene(n1, 5, seed=10 + n1, n_nodes=2, n2=[1, 63, 64, 65, 257])
    assert [k.n for k in s["neighbours"]] == [1, 63, 64, 65, 257] and s["kf1"].n == n1
    rn, _, _ = _scene_parity(ctx, s, ori)
    if n1 >= 63:
        assert rn[1:].min() > 0      # not vacuous: every neighbour of >= 63 features is matched


def _unclaimed(k):
    return (k.node >= 0) & (k.weight > 0) & (k.has_mp == 0)


@ORI
@pytest.mark.parametrize("ncand", [64, 65])
def test_one_node_with_64_and_65_candidates(ctx, ncand, ori):
    """One node on both sides; exactly `ncand` KF2 features are candidates of every KF1 feature."""
    s = synthetic_triangulation_scene(120, 1, seed=20, n_nodes=1, n2=110)
    k2 = s["neighbours"][0]
    extra = np.nonzero(_unclaimed(k2))[0][ncand:]
    assert extra.size > 0
    k2.has_mp[extra] = 1
    assert int(_unclaimed(k2).sum()) == ncand and np.unique(k2.node[k2.node >= 0]).size == 1
    rn, _, _ = _scene_parity(ctx, s, ori)
    assert rn[0] > 0


@ORI
def test_node_on_one_side_only(ctx, ori):
    s = synthetic_triangulation_scene(150, 2, seed=21, n_nodes=3)
    k1 = s["kf1"]
    nodes = np.unique(k1.node[k1.node >= 0])
    k1.node[k1.node == nodes[0]] = 2_000_001              # a node only KF1 has
    for k2 in s["neighbours"]:
        k2.node[k2.node == nodes[1]] = 2_000_002          # a node only the neighbour has
    rn, rm, _ = _scene_parity(ctx, s, ori)
    assert (rm[:, (k1.node == 2_000_001) | (k1.node == nodes[1])] == -1).all() and (rn > 0).all()


@ORI
def test_every_kf1_feature_has_a_mappoint(ctx, ori):
    s = synthetic_triangulation_scene(100, 2, seed=22, n_nodes=3, mp_frac=1.0)
    assert s["kf1"].has_mp.all()
    rn, rm, _ = _scene_parity(ctx, s, ori)
    assert rn.tolist() == [0, 0] and (rm == -1).all()


@ORI
def test_empty_neighbour_between_two(ctx, ori):
    s = synthetic_triangulation_scene(100, 3, seed=23, n_nodes=3, n2=[None, 0, None])
    assert [k.n > 0 for k in s["neighbours"]] == [True, False, True]
    rn, rm, _ = _scene_parity(ctx, s, ori)
    assert rn[1] == 0 and (rm[1] == -1).all() and rn[0] > 0 and rn[2] > 0


@ORI
@pytest.mark.parametrize("B", [1, 20])
def test_batch_sizes(ctx, B, ori):
    """B = 1 and B = 20, a different n2 per neighbour."""
    n2 = [40 + 17 * b for b in range(B)]
    s = synthetic_triangulation_scene(200, B, seed=24, n_nodes=6, n2=n2)
    assert [k.n for k in s["neighbours"]] == n2
    rn, _, _ = _scene_parity(ctx, s, ori)
    assert (rn > 0).all()


@pytest.fixture(scope="module")
def full_scene():
    """n = 2048 on both sides, ~100 nodes; eight matched twins are moved to KF2 indices 2040..2047
    (KF1's last features are its planted duplicates, so its indices up there match as well)."""
    s = synthetic_triangulation_scene(2048, 1, seed=25, n_nodes=100, n2=2048)
    k1, k2 = s["kf1"], s["neighbours"][0]
    _, m, _ = T.search_pair(k1, k2, s["scale_factors"], s["level_sigma2"], 0)
    src = [j for j in dict.fromkeys(m[m >= 0].tolist()) if j < 2040][:8]
    assert len(src) == 8
    for arr in (k2.kps, k2.desc, k2.node, k2.weight, k2.has_mp):
        for k, j in enumerate(src):
            tmp = arr[j].copy(); arr[j] = arr[2040 + k]; arr[2040 + k] = tmp
    return s


@ORI
def test_full_size_with_the_last_indices_matched(ctx, full_scene, ori):
    s = full_scene
    assert s["kf1"].n == 2048 and s["neighbours"][0].n == 2048
    rn, rm, _ = _scene_parity(ctx, s, ori)
    if ori == 0:
        assert set(range(2040, 2048)) <= set(rm[0].tolist())
        assert (rm[0, 2040:] >= 0).any()
    assert rn[0] > 200


def test_envelope(ctx):
    s = synthetic_triangulation_scene(40, 1, seed=26, n_nodes=2)
    k1, k2, sf, s2 = s["kf1"], s["neighbours"][0], s["scale_factors"], s["level_sigma2"]

    def blank(n):
        return TriKeyFrame(np.zeros(n, KP_DTYPE), np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.ones(n),
                           np.zeros(n, np.uint8), k2.pose_q, k2.pose_t, k2.fx, k2.fy, k2.cx, k2.cy)
    mt = ORBmatcher(0.6, False, ctx=ctx)
    for kf, nb in ((blank(2049), [k2]), (k1, [k2, blank(2049)]), (k1, [k2] * 65)):
        with pytest.raises(OrbHipError) as e:
            mt.SearchForTriangulation(kf, nb, sf, s2)
        assert e.value.code == -5          # ORBHIP_ERR_UNSUPPORTED
    nm, m = mt.SearchForTriangulation(blank(2048), [k2] * 64, sf, s2)   # the envelope itself is accepted
    assert nm.shape == (64,) and m.shape == (64, 2048)
    bad = blank(3)
    bad.kps["octave"][1] = len(sf)
    for kf, nb in ((k1, [k2, bad]), (bad, [k2])):
        with pytest.raises(OrbHipError) as e:
            mt.SearchForTriangulation(kf, nb, sf, s2)
        assert e.value.code == -1          # ORBHIP_ERR_ARG
    bad.kps["octave"][1] = -1
    with pytest.raises(OrbHipError) as e:
        mt.SearchForTriangulation(k1, [bad], sf, s2)
    assert e.value.code == -1
    # B == 0 and an empty KF1 return 0 matches
    nm, m = mt.SearchForTriangulation(k1, [], sf, s2)
    assert nm.shape == (0,) and m.shape == (0, k1.n)
    nm, m = mt.SearchForTriangulation(blank(0), [k2, k2], sf, s2)
    assert nm.tolist() == [0, 0] and m.shape == (2, 0)


def test_repeatability_on_one_context(ctx):
    """Calls of different B and n on one context (the staging block grows, then is reused by a
    smaller call) return what fresh contexts return."""
    big = T.parity_scene(0)
    small = synthetic_triangulation_scene(65, 1, seed=27, n_nodes=2)
    mid = synthetic_triangulation_scene(200, 7, seed=28, n_nodes=6)
    order = [small, big, small, mid, big]
    got = [_library(ctx, s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 1) for s in order]
    for s, (gn, gm) in zip(order, got):
        fresh = Context()
        fn, fm = _library(fresh, s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 1)
        fresh.close()
        assert gn.tolist() == fn.tolist() and np.array_equal(gm, fm)
        assert gn.sum() > 0
