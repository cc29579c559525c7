"""The Sim3 functions LoopClosing calls (Fuse and SearchByProjection with a Sim3) on the CPU, no
context: definitional cases of the restatement (tests/sim3_numpy.py), each with an answer that
follows from the rule in DESIGN.md; the three statements of the greedy pass against each other; the
conditions the parity scenes must meet for tests/test_sim3_gpu.py to mean something; the exported
symbols; the C++ mirror."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import orb_scale_tables

import fuse_numpy as F
import sim3_numpy as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SF, S2 = orb_scale_tables()
INV_S2 = (f32(1.0) / S2).astype(f32)
BASE_DESC = np.random.Generator(np.random.PCG64(78)).integers(0, 256, 32, dtype=np.uint8)


def _flip(desc, nbits):
    d = np.array(desc, np.uint8)
    for b in range(nbits):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _kf(kps, descs, claimed=None):
    kf = F.make_keyframe(kps, descs)
    if claimed is not None:
        kf.claimed = np.array(claimed, np.uint8)
    return kf


def _search(kf, pts, descs, th=3.0, ratio=1.0, skip=None):
    """(match, match_dist, level, counters) of the literal loop, after checking that the sorted-list
    and fixed-point forms give the same."""
    a = (kf, np.stack([p["P"] for p in pts]), np.stack([p["normal"] for p in pts]), [p["min_dist"] for p in pts],
         [p["max_dist"] for p in pts], np.stack(descs), th, ratio, skip)
    nm, match, dist, lvl, cnt = S.search_by_projection_sim3(*a)
    lists, lvl2 = S.candidate_lists(*a)
    for other in (S.resolve_sorted(lists), S.resolve_fixed_point(lists)):
        assert other[0] == nm and np.array_equal(other[1], match) and np.array_equal(other[2], dist)
    assert np.array_equal(lvl, lvl2) and nm == int((match >= 0).sum()) == cnt["accepted"]
    return match.tolist(), dist.tolist(), lvl.tolist(), cnt


# ---- definitional cases ----

def test_two_points_with_one_best_keypoint_the_lower_index_gets_it():
    pt = F.make_point(300.0, 200.0, 4.0, 2)
    u, v = pt["u"], pt["v"]
    # the second candidate within thr: the later point gets it
    kf = _kf([(u, v, 2), (u + f32(1), v, 2)], [BASE_DESC, _flip(BASE_DESC, 40)])
    match, dist, lvl, cnt = _search(kf, [pt, pt], [BASE_DESC, BASE_DESC])
    assert (match, dist, lvl) == ([0, 1], [0, 40], [2, 2]) and cnt["cand_taken"] == 1
    # the second candidate above thr: the later point gets nothing, although keypoint 0 was below thr
    kf = _kf([(u, v, 2), (u + f32(1), v, 2)], [BASE_DESC, _flip(BASE_DESC, 60)])
    match, dist, _, cnt = _search(kf, [pt, pt], [BASE_DESC, BASE_DESC])
    assert (match, dist) == ([0, -1], [0, 256]) and cnt["above_thr"] == 1 and cnt["cand_taken"] == 1
    # no second candidate at all
    match, dist, _, cnt = _search(_kf([(u, v, 2)], [BASE_DESC]), [pt, pt], [BASE_DESC, BASE_DESC])
    assert (match, dist) == ([0, -1], [0, 256]) and cnt["no_candidate"] == 1


def test_a_chain_of_three_moves_every_later_point_one_further():
    """Three equal points, three keypoints at distances 0, 10, 20: point m gets keypoint m (the
    fixed-point form needs three rounds of change for this)."""
    pt = F.make_point(300.0, 200.0, 4.0, 2)
    u, v = pt["u"], pt["v"]
    kf = _kf([(u + f32(1), v, 2), (u, v, 2), (u - f32(1), v, 2)], [_flip(BASE_DESC, 20), BASE_DESC, _flip(BASE_DESC, 10)])
    match, dist, _, _ = _search(kf, [pt] * 3, [BASE_DESC] * 3)
    assert (match, dist) == ([1, 2, 0], [0, 10, 20])
    lists, _ = S.candidate_lists(kf, np.stack([pt["P"]] * 3), np.stack([pt["normal"]] * 3), [pt["min_dist"]] * 3,
                                 [pt["max_dist"]] * 3, np.stack([BASE_DESC] * 3), 3.0, 1.0)
    assert S.resolve_fixed_point(lists)[3] == 4            # three rounds that change something, one that does not


def test_keypoint_claimed_at_call_time_is_never_matched():
    pt = F.make_point(300.0, 200.0, 4.0, 2)
    u, v = pt["u"], pt["v"]
    kps, descs = [(u, v, 2), (u + f32(1), v, 2)], [BASE_DESC, _flip(BASE_DESC, 30)]
    assert _search(_kf(kps, descs), [pt], [BASE_DESC])[0] == [0]
    match, dist, _, cnt = _search(_kf(kps, descs, claimed=[1, 0]), [pt], [BASE_DESC])
    assert (match, dist) == ([1], [30]) and cnt["cand_claimed"] == 1
    match, dist, _, cnt = _search(_kf(kps, descs, claimed=[1, 1]), [pt], [BASE_DESC])
    assert (match, dist) == ([-1], [256]) and cnt["no_candidate"] == 1


def test_skipped_point_claims_nothing():
    pt = F.make_point(300.0, 200.0, 4.0, 2)
    kf = _kf([(pt["u"], pt["v"], 2)], [BASE_DESC])
    match, dist, lvl, cnt = _search(kf, [pt, pt], [BASE_DESC, BASE_DESC], skip=[1, 0])
    assert (match, dist, lvl) == ([-1, 0], [256, 0], [-1, 2]) and cnt["skip"] == 1


@pytest.mark.parametrize("ratio,bits,kept", [(1.0, 50, True), (1.0, 51, False), (1.5, 75, True), (1.5, 76, False)])
def test_threshold_edges(ratio, bits, kept):
    assert float(S.threshold(ratio)) == 50.0 * ratio
    pt = F.make_point(300.0, 200.0, 4.0, 2)
    match, dist, lvl, cnt = _search(_kf([(pt["u"], pt["v"], 2)], [_flip(BASE_DESC, bits)]), [pt], [BASE_DESC], ratio=ratio)
    assert (match, dist, lvl) == (([0], [bits], [2]) if kept else ([-1], [256], [2]))
    assert cnt["above_thr"] == (not kept)


@pytest.mark.parametrize("level", [0, 7])
def test_candidate_2_455_sigma_away_is_accepted_where_fuse_rejects_it(level):
    """5.99 = 2.4474^2: Fuse's chi-square gate drops a keypoint 2.455 level sigma from the projection;
    the Sim3 functions have no such gate."""
    pt = F.make_point(300.0, 200.0, 4.0, level)
    x = f32(pt["u"] + f32(2.455) * SF[level])
    kf = _kf([(x, pt["v"], level)], [BASE_DESC])
    a = (pt["P"][None], pt["normal"][None], [pt["min_dist"]], [pt["max_dist"]], [BASE_DESC])
    _, idx, dist, _, cnt = F.fuse([kf], *a, INV_S2, 3.0)
    assert (idx[0, 0], dist[0, 0]) == (-1, 256) and cnt["cand_chi2"] == 1
    assert _search(kf, [pt], [BASE_DESC])[:2] == ([0], [0])
    nf, idx, dist, lvl = S.fuse_sim3([kf], *a, 3.0)
    assert (nf[0], idx[0, 0], dist[0, 0], lvl[0, 0]) == (1, 0, 0, level)


@pytest.mark.parametrize("octave,kept", [(2, False), (3, True), (4, True), (5, False)])
def test_octave_gate_keeps_level_minus_one_and_level(octave, kept):
    pt = F.make_point(300.0, 200.0, 4.0, 4)
    kf = _kf([(pt["u"], pt["v"], octave)], [BASE_DESC])
    match, dist, lvl, cnt = _search(kf, [pt], [BASE_DESC])
    assert lvl == [4] and (match, dist) == (([0], [0]) if kept else ([-1], [256]))
    assert cnt["cand_level_low"] == (octave == 2) and cnt["cand_level_high"] == (octave == 5)
    nf, idx, dist, lvl = S.fuse_sim3([kf], pt["P"][None], pt["normal"][None], [pt["min_dist"]], [pt["max_dist"]],
                                     [BASE_DESC], 4.0)
    assert (idx[0, 0], dist[0, 0], lvl[0, 0]) == ((0, 0, 4) if kept else (-1, 256, 4))


def test_fuse_sim3_reports_a_distance_above_th_low_and_rejects_it():
    pt = F.make_point(300.0, 200.0, 4.0, 2)
    for bits, want in ((50, (0, 50)), (51, (-1, 51))):
        kf = _kf([(pt["u"], pt["v"], 2)], [_flip(BASE_DESC, bits)])
        nf, idx, dist, _ = S.fuse_sim3([kf], pt["P"][None], pt["normal"][None], [pt["min_dist"]], [pt["max_dist"]],
                                       [BASE_DESC], 4.0)
        assert (idx[0, 0], dist[0, 0]) == want and nf[0] == (bits == 50)


# ---- the three statements of the greedy pass ----

@pytest.mark.parametrize("k", range(len(S.PARITY_SCENES)))
def test_loop_sorted_lists_and_fixed_point_agree_on_the_parity_scenes(k):
    s = S.parity_scene(k)
    nm, match, dist, lvl, _ = s["expected"]
    lists, lvl2 = S.lists_of_scene(s)
    a, b = S.resolve_sorted(lists), S.resolve_fixed_point(lists)
    for other in (a, b):
        assert other[0] == nm and np.array_equal(other[1], match) and np.array_equal(other[2], dist)
    assert np.array_equal(lvl, lvl2)
    print(f"scene {k}: {nm} matches, {b[3]} rounds")


@pytest.mark.parametrize("claimed", [False, True])
def test_chain_scene_point_m_gets_the_mth_free_keypoint(claimed):
    s = S.chain_scene(300, 320, every_second_claimed=claimed)
    assert list(F.Grid(s["kf"]).cells) == [(32, 24)]
    nm, match, dist, lvl, _ = S.search_scene(s)
    free = np.arange(0, 300, 2) if claimed else np.arange(300)
    want = np.full(320, -1)
    want[:len(free)] = free
    assert match.tolist() == want.tolist() and nm == len(free) and (lvl == 7).all()
    assert (dist[:len(free)] == 0).all() and (dist[len(free):] == 256).all()
    lists, _ = S.lists_of_scene(s)
    assert all(len(keys) == len(free) for keys in lists)
    a, b = S.resolve_sorted(lists), S.resolve_fixed_point(lists)
    assert np.array_equal(a[1], match) and np.array_equal(b[1], match) and b[3] == len(free) + 2     # every keypoint placed, then the rest lose theirs


def test_cluster_scene_has_long_lists_with_distinct_keys():
    """The scene tests/test_sim3_gpu.py uses for lists past the stored capacity: every point's list
    is longer than 32, points end up 30 and more entries down their list, some with nothing."""
    s = S.cluster_scene()
    nm, match, dist, _, cnt = S.search_scene(s)
    lists, _ = S.lists_of_scene(s)
    a, b = S.resolve_sorted(lists), S.resolve_fixed_point(lists)
    assert np.array_equal(a[1], match) and np.array_equal(b[1], match) and np.array_equal(b[2], dist)
    assert min(len(keys) for keys in lists) > 32 and a[3].max() >= 30 and (a[3] < 0).sum() >= 3
    assert len({k[0] for k in lists[0]}) > 16 and len({k[1] for k in lists[0]}) > 8      # distances, cells
    assert len(F.Grid(s["kf"]).cells) > 8 and cnt["cand_claimed"] > 0 and b[3] > 16


# ---- Fuse with a Sim3 ----

@pytest.mark.parametrize("k", range(len(F.PARITY_SCENES)))
def test_fuse_sim3_equals_fuse_with_zero_inv_level_sigma2(k):
    """(double)(e2 * 0) > 5.99 never holds, so Fuse with an all-zero table is the Sim3 rule."""
    s = F.parity_scene(k)
    for ps in (s["pair_skip"], None):
        want = F.fuse_scene(dict(s, ratios=None), inv_level_sigma2=np.zeros(8, f32), th=4.0, pair_skip=ps)
        got = S.fuse_sim3(s["kfs"], s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], 4.0,
                          s["skip"], ps)
        for g, w in zip(got, want[:4]):
            assert np.array_equal(g, w)
        assert want[4]["cand_chi2"] == 0 and got[0].min() > 50
    # and the gate matters on these scenes: with the real table some pairs come out differently
    real = F.fuse_scene(dict(s, ratios=None), th=4.0)
    assert real[4]["cand_chi2"] > 0 and not np.array_equal(real[1], got[1])


# ---- conditions of the parity scene set ----

def test_parity_scene_conditions():
    assert sorted({(s["th"], s["ratio"]) for s in S.PARITY_SCENES}) == sorted(S.SETTINGS) == [(3, 1.5), (5, 1.0), (8, 1.5)]
    for k in range(len(S.PARITY_SCENES)):
        s = S.parity_scene(k)
        nm, match, dist, lvl, cnt = s["expected"]
        assert s["kf"].kps.shape[0] == 300 and match.shape == (400,)
        assert int(s["kf"].claimed.sum()) >= 10                        # keypoints claimed at call time
        for key in S.GATE_COUNTERS:                                    # every gate fires, both tie kinds too
            assert cnt[key] > 0, (k, key)
        assert set(np.unique(lvl[lvl >= 0]).tolist()) == set(range(8))
        lists = s["lists"]
        pos = S.resolve_sorted(lists)[3]
        has_list = np.array([len(keys) > 0 for keys in lists])
        not_first, later, none = int((has_list & (pos != 0)).sum()), int((pos > 0).sum()), int((has_list & (pos < 0)).sum())
        print(f"scene {k}: {nm} matches, {not_first} points not their first entry, {later} a later one, {none} none; "
              f"counters {cnt}")
        assert not_first >= 20 and later >= 5 and none >= 20
        # PredictScale's ceil is more than 1e-3 from a step for EVERY point that reaches it
        assert {m for m, _ in s["ratios"]} == set(np.nonzero(lvl >= 0)[0].tolist())
        assert min(abs(x - round(x)) for _, x in s["ratios"]) > 1e-3
        # matches are one-to-one and never a keypoint claimed at call time
        got = match[match >= 0]
        assert len(set(got.tolist())) == len(got) and not s["kf"].claimed[got].any()
        assert (dist[match >= 0] <= float(S.threshold(s["ratio"]))).all() and (dist[match < 0] == 256).all()


# ---- the symbols ----

def test_the_sim3_entry_points_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    from orb_slam3_ros2_amd import _lib
    L = _lib.lib()
    for name in ("orbhip_fuse_sim3", "orbhip_search_by_projection_sim3"):
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", src, re.M)
        assert name in _lib.EXPORTED and hasattr(L, name)
    assert L.orbhip_abi_version() == 1
    # argument checks that need no device
    assert L.orbhip_fuse_sim3(None, None, 1, None, None, 4.0, None, None, None, None) == -1
    assert L.orbhip_search_by_projection_sim3(None, None, None, 3.0, 1.5, None, None, None) == -1
    assert L.orbhip_test_sim3_list_cap() >= 1
    from orb_slam3_ros2_amd.matcher import ORBmatcher
    assert callable(ORBmatcher.FuseSim3) and callable(ORBmatcher.SearchByProjectionSim3)


# ---- the C++ mirror ----

def test_cpp_mirror_names_the_sim3_functions(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tu = tmp_path / "sim3_mirror.cpp"
    tu.write_text('''#include "orbhip.hpp"
int loop(orbhip_ctx* ctx, const std::vector<orbhip_frame>& kfs, const orbhip_local_points& mps,
         const std::vector<uint8_t>& pair_skip, std::vector<std::vector<int>>& best, std::vector<int>& match,
         std::vector<int>& dist, std::vector<int>& level) {
    orbhip::ORBmatcher matcher;
    std::vector<int> a = matcher.FuseSim3(ctx, kfs, mps, pair_skip, 4.0f, best);
    std::vector<int> b = matcher.FuseSim3(ctx, kfs, mps, pair_skip, 4.0f, best, &best, &best);
    int n = matcher.SearchByProjectionSim3(ctx, kfs[0], mps, 3, 1.5f, match);
    n += matcher.SearchByProjectionSim3(ctx, kfs[0], mps, 8, 1.5f, match, &dist, &level);
    int (*f)(orbhip_ctx*, const orbhip_frame*, int, const orbhip_local_points*, const uint8_t*, float, int32_t*,
             int32_t*, int32_t*, int32_t*) = &orbhip_fuse_sim3;
    int (*g)(orbhip_ctx*, const orbhip_frame*, const orbhip_local_points*, float, float, int32_t*, int32_t*,
             int32_t*) = &orbhip_search_by_projection_sim3;
    (void)f; (void)g;
    return n + (int)a.size() + (int)b.size();
}
''')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
