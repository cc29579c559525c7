"""ORBmatcher::Fuse on the CPU, no context: definitional cases of the restatement
(tests/fuse_numpy.py), each with an answer that follows from the rule in DESIGN.md; the conditions
the parity scenes must meet for tests/test_fuse_gpu.py to mean something; the exported symbol; the
C++ mirror."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import D435I, FUSE_KINDS, fuse_level_margin, orb_scale_tables

import fuse_numpy as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = D435I
f32 = np.float32
SF, S2 = orb_scale_tables()
INV_S2 = (f32(1.0) / S2).astype(f32)
LOG_SF = float(np.log(f32(1.2)))
RNG = np.random.Generator(np.random.PCG64(77))
BASE_DESC = RNG.integers(0, 256, 32, dtype=np.uint8)


def _flip(desc, nbits):
    d = np.array(desc, np.uint8)
    for b in range(nbits):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


_kf, _point = F.make_keyframe, F.make_point


def _fuse1(kf, pt, desc=BASE_DESC, th=3.0, **over):
    a = dict(points=pt["P"][None], normals=pt["normal"][None], min_dist=[pt["min_dist"]], max_dist=[pt["max_dist"]])
    a.update(over)
    nf, idx, dist, lvl, cnt = F.fuse([kf], a["points"], a["normals"], a["min_dist"], a["max_dist"], [desc], INV_S2, th,
                                     a.get("skip"), a.get("pair_skip"))
    assert nf[0] == int(idx[0, 0] >= 0) == cnt["accepted"]
    return int(idx[0, 0]), int(dist[0, 0]), int(lvl[0, 0]), cnt


# ---- definitional cases ----

@pytest.mark.parametrize("level", [0, 3, 7])
def test_exact_projection_matches_its_keypoint(level):
    pt = _point(200.3, 150.7, 3.0, level)
    kf = _kf([(50.0, 60.0, level), (pt["u"], pt["v"], level), (400.0, 300.0, level)], [_flip(BASE_DESC, 90),
                                                                                      BASE_DESC, BASE_DESC])
    assert _fuse1(kf, pt)[:3] == (1, 0, level)


def test_twin_in_an_earlier_cell_wins_then_the_lower_index():
    pt = _point(CAM["cx"], CAM["cy"], 3.0, 7)     # r = 10.7 px, chi-square bound 8.8 px
    u, v = pt["u"], pt["v"]
    d = _flip(BASE_DESC, 7)
    g = F.Grid(_kf([(u + f32(6), v, 7), (u - f32(6), v, 7)], [d, d]))
    assert len(g.cells) == 2                      # two cells, the one of index 1 has the lower px
    idx, dist, _, cnt = _fuse1(_kf([(u + f32(6), v, 7), (u - f32(6), v, 7)], [d, d]), pt)
    assert (idx, dist) == (1, 7) and cnt["tie_cell"] == 1 and cnt["tie_index"] == 0
    # the same cell: the lower index, whichever of the two positions it has
    for a, b in ((f32(1), f32(1.5)), (f32(1.5), f32(1))):
        kf = _kf([(u + a, v, 7), (u + b, v, 7)], [d, d])
        assert len(F.Grid(kf).cells) == 1
        idx, dist, _, cnt = _fuse1(kf, pt)
        assert (idx, dist) == (0, 7) and cnt["tie_index"] == 1 and cnt["tie_cell"] == 0
    # a strictly better candidate later in the walk still wins
    kf = _kf([(u - f32(6), v, 7), (u + f32(6), v, 7)], [d, _flip(BASE_DESC, 6)])
    assert _fuse1(kf, pt)[:2] == (1, 6)


def test_th_low_50_is_accepted_and_51_is_not():
    pt = _point(300.0, 200.0, 4.0, 2)
    for bits, want in ((50, (0, 50)), (51, (-1, 51))):
        idx, dist, lvl, cnt = _fuse1(_kf([(pt["u"], pt["v"], 2)], [_flip(BASE_DESC, bits)]), pt)
        assert (idx, dist) == want and lvl == 2 and cnt["th_low"] == (bits == 51)


@pytest.mark.parametrize("octave,kept", [(2, False), (3, True), (4, True), (5, False)])
def test_octave_gate_keeps_level_minus_one_and_level(octave, kept):
    pt = _point(300.0, 200.0, 4.0, 4)
    idx, dist, lvl, cnt = _fuse1(_kf([(pt["u"], pt["v"], octave)], [BASE_DESC]), pt)
    assert lvl == 4
    assert (idx, dist) == ((0, 0) if kept else (-1, 256))
    assert cnt["cand_level_low"] == (octave == 2) and cnt["cand_level_high"] == (octave == 5)


@pytest.mark.parametrize("octave", [0, 7])
@pytest.mark.parametrize("chi2,kept", [(5.9, True), (6.1, False)])
def test_chi_square_gate(octave, chi2, kept):
    pt = _point(300.0, 200.0, 4.0, octave)
    x = f32(pt["u"] + f32(np.sqrt(chi2 * float(S2[octave]))))
    ex = pt["u"] - x
    got = np.float64((ex * ex + f32(0) * f32(0)) * INV_S2[octave])
    assert (got <= 5.99) == kept and abs(got - chi2) < 0.01      # the planted error is on the side meant
    assert abs(float(ex)) < 3.0 * float(SF[octave])               # and inside the window
    idx, dist, lvl, cnt = _fuse1(_kf([(x, pt["v"], octave)], [BASE_DESC]), pt)
    assert lvl == octave and (idx, dist) == ((0, 0) if kept else (-1, 256)) and cnt["cand_chi2"] == (not kept)


def test_image_bound_minimum_is_inclusive_and_maximum_strict():
    pt = _point(CAM["cx"], CAM["cy"], 3.0, 1)
    assert pt["P"][0] == 0 and pt["P"][1] == 0                    # on the optical axis: u = cx, v = cy exactly
    assert pt["u"] == f32(CAM["cx"]) and pt["v"] == f32(CAM["cy"])
    kp = [(pt["u"], pt["v"], 1)]
    W, H, cx, cy = CAM["w"], CAM["h"], CAM["cx"], CAM["cy"]
    assert _fuse1(_kf(kp, [BASE_DESC], bounds=(cx, W, 0, H)), pt)[:2] == (0, 0)
    assert _fuse1(_kf(kp, [BASE_DESC], bounds=(0, W, cy, H)), pt)[:2] == (0, 0)
    for bounds in ((0, cx, 0, H), (0, W, 0, cy)):
        idx, dist, lvl, cnt = _fuse1(_kf(kp, [BASE_DESC], bounds=bounds), pt)
        assert (idx, dist, lvl) == (-1, 256, -1) and cnt["outside"] == 1


def test_point_behind_the_camera_is_rejected():
    pt = _point(300.0, 200.0, 3.0, 2)
    kf = _kf([(pt["u"], pt["v"], 2)], [BASE_DESC])
    assert _fuse1(kf, pt)[0] == 0
    back = dict(pt, P=(pt["P"] * f32(-1)).astype(f32), normal=(pt["normal"] * f32(-1)).astype(f32))
    idx, dist, lvl, cnt = _fuse1(kf, back)                        # the same pixel, z < 0
    assert (idx, dist, lvl) == (-1, 256, -1) and cnt["behind"] == 1


def test_distance_range_both_sides_of_both_bounds():
    pt = _point(300.0, 200.0, 3.0, 2)
    kf = _kf([(pt["u"], pt["v"], 2)], [BASE_DESC])
    d = float(pt["dist"])
    for mn, want in ((d / 0.8 * 0.999, "in"), (d / 0.8 * 1.001, "dist_low")):
        idx, _, lvl, cnt = _fuse1(kf, pt, min_dist=[f32(mn)])
        assert (idx, lvl) == ((0, 2) if want == "in" else (-1, -1)) and cnt["dist_low"] == (want != "in")
    # (max_dist below dist3D: the ratio is below 1, PredictScale clamps to level 0; octave 0 keypoint)
    kf0 = _kf([(pt["u"], pt["v"], 0)], [BASE_DESC])
    for mx, want in ((d / 1.2 * 1.001, "in"), (d / 1.2 * 0.999, "dist_high")):
        idx, _, lvl, cnt = _fuse1(kf0, pt, max_dist=[f32(mx)])
        assert (idx, lvl) == ((0, 0) if want == "in" else (-1, -1)) and cnt["dist_high"] == (want != "in")


def test_viewing_angle_both_sides_of_60_degrees():
    pt = _point(CAM["cx"], CAM["cy"], 3.0, 2)                     # PO along +z
    kf = _kf([(pt["u"], pt["v"], 2)], [BASE_DESC])
    for deg, ok in ((59.0, True), (61.0, False)):
        a = np.deg2rad(deg)
        nrm = np.array([np.sin(a), 0, np.cos(a)], f32)
        idx, _, lvl, cnt = _fuse1(kf, pt, normals=nrm[None])
        assert (idx, lvl) == ((0, 2) if ok else (-1, -1)) and cnt["angle"] == (not ok)


def test_window_over_each_grid_edge_and_the_early_returns():
    g = F.Grid(_kf([], np.zeros((0, 32))))
    r = f32(5)
    W, H = f32(CAM["w"]), f32(CAM["h"])
    assert F.step8_rectangle(g, f32(2), f32(240), r) == (0, 1, 23, 25)        # left edge: floor(-0.3) -> 0
    assert F.step8_rectangle(g, f32(638), f32(240), r) == (63, 63, 23, 25)    # right: ceil(64.3) -> 63
    assert F.step8_rectangle(g, f32(320), f32(2), r) == (31, 33, 0, 1)        # top
    assert F.step8_rectangle(g, f32(320), f32(478), r) == (31, 33, 47, 47)    # bottom: ceil(48.3) -> 47
    # the early returns (reached only with (u, v) outside the bounds, which step 3 excludes)
    assert F.step8_rectangle(g, W + f32(6), f32(240), r) is None              # nMinCellX >= 64
    assert F.step8_rectangle(g, f32(-16), f32(240), r) is None                # nMaxCellX < 0
    assert F.step8_rectangle(g, f32(320), H + f32(6), r) is None              # nMinCellY >= 48
    assert F.step8_rectangle(g, f32(320), f32(-16), r) is None                # nMaxCellY < 0
    assert F.step8_area(g, W + f32(6), f32(240), r) is None
    # whole pairs at the four edges: the keypoint lies in the clipped rectangle and is found
    # (level 7: r = 10.7 px; on the far side the keypoint sits 5 px inside, PosInGrid's round puts
    # x >= 635 / y >= 475 outside the grid)
    def inside(a, size):
        return a + 1.0 if a < 40 else (a - 5.0 if a > size - 40 else a)
    for u, v in ((1.5, 240.0), (638.5, 240.0), (320.0, 1.5), (320.0, 478.5), (1.0, 1.0), (638.9, 478.9)):
        pt = _point(u, v, 3.0, 7)
        kf = _kf([(f32(inside(float(pt["u"]), 640)), f32(inside(float(pt["v"]), 480)), 7), (320.0, 240.0, 7)],
                 [BASE_DESC, BASE_DESC])
        rect = F.step8_rectangle(F.Grid(kf), pt["u"], pt["v"], F.step7_radius(F.Grid(kf), 3.0, 7))
        assert (rect[0] == 0 or rect[1] == 63 or rect[2] == 0 or rect[3] == 47), rect    # clipped
        idx, dist, lvl, cnt = _fuse1(kf, pt)
        assert (idx, dist, lvl) == (0, 0, 7) and cnt["no_window"] == 0, (u, v)


def test_keypoint_outside_the_grid_is_never_a_candidate():
    """PosInGrid rounds: x >= 635 gives px = 64 and the keypoint is in no cell (as the reference)."""
    pt = _point(636.0, 240.0, 3.0, 3)
    kf = _kf([(pt["u"], pt["v"], 3)], [BASE_DESC])
    assert F.Grid(kf).cells == {}
    idx, dist, lvl, cnt = _fuse1(kf, pt)
    assert (idx, dist, lvl) == (-1, 256, 3) and cnt["no_candidate"] == 1


def test_skip_and_pair_skip_are_honoured():
    pt = _point(300.0, 200.0, 3.0, 2)
    kf = _kf([(pt["u"], pt["v"], 2)], [BASE_DESC])
    assert _fuse1(kf, pt, skip=[0], pair_skip=[[0]])[:3] == (0, 0, 2)
    idx, dist, lvl, cnt = _fuse1(kf, pt, skip=[1])
    assert (idx, dist, lvl) == (-1, 256, -1) and cnt["skip"] == 1
    idx, dist, lvl, cnt = _fuse1(kf, pt, pair_skip=[[1]])
    assert (idx, dist, lvl) == (-1, 256, -1) and cnt["pair_skip"] == 1
    # pair_skip is per keyframe: two keyframes, the point skipped in the first only
    P = dict(points=pt["P"][None], normals=pt["normal"][None], min_dist=[pt["min_dist"]], max_dist=[pt["max_dist"]])
    nf, idx, _, _, _ = F.fuse([kf, kf], P["points"], P["normals"], P["min_dist"], P["max_dist"], [BASE_DESC], INV_S2,
                              3.0, None, [[1], [0]])
    assert nf.tolist() == [0, 1] and idx[:, 0].tolist() == [-1, 0]


def test_walk_result_is_the_key_minimum():
    """The reference's walk (strict <, first wins) equals the minimum of (dist, cell, idx) over the
    gated candidates: recomputed here from scratch for every pair of a parity scene."""
    s = F.parity_scene(0)
    _, idx, dist, lvl, _ = s["expected"]
    for b, kf in enumerate(s["kfs"]):
        g = F.Grid(kf)
        for m in range(idx.shape[1]):
            if lvl[b, m] < 0:
                continue
            L = int(lvl[b, m])
            u, v = F.step2_project(g, F.step1_camera(g, [f32(x) for x in s["points"][m]]))
            cand = F.step8_area(g, u, v, F.step7_radius(g, s["th"], L))
            keys = []
            for cell, j in cand:
                o = int(g.octave[j])
                ex, ey = u - g.x[j], v - g.y[j]
                if L - 1 <= o <= L and not np.float64((ex * ex + ey * ey) * INV_S2[o]) > 5.99:
                    keys.append((int(F._POP[g.desc[j] ^ s["mp_desc"][m]].sum()), cell, j))
            best = min(keys) if keys else (256, -1, -1)
            assert dist[b, m] == best[0] and idx[b, m] == (best[2] if best[0] <= 50 else -1)


# ---- conditions of the parity scene set ----

def test_parity_scene_conditions():
    for k in range(len(F.PARITY_SCENES)):
        s = F.parity_scene(k)
        nf, idx, dist, lvl, cnt = s["expected"]
        n = s["points"].shape[0]
        print(f"scene {k}: fused {nf.tolist()} counters {cnt}")
        assert idx.shape == (3, 300) and all(kf.kps.shape[0] == 300 for kf in s["kfs"])
        for key in F.GATE_COUNTERS:                       # every gate fires, both tie kinds too
            assert cnt[key] > 0, (k, key)
        assert (nf * 3 >= n).all(), nf                    # at least a third of the points of every keyframe
        assert set(np.unique(lvl[lvl >= 0]).tolist()) == set(range(8))
        assert (dist[(idx < 0) & (dist < 256)] > 50).all() and (dist[idx >= 0] <= 50).all()
        assert set(s["kind"].tolist()) == set(FUSE_KINDS)
        # PredictScale's ceil is at least 1e-3 away from a step for EVERY pair that reaches it
        reached = {(b, m) for b, m, _ in s["ratios"]}
        assert reached == {(int(b), int(m)) for b, m in np.argwhere(lvl >= 0)}
        margin = min(abs(x - round(x)) for _, _, x in s["ratios"])
        print(f"scene {k}: level margin {margin:.2e} over {len(reached)} pairs")
        assert margin > 1e-3
        assert fuse_level_margin(s["kfs"], s["points"], s["max_dist"]).min() > 2e-3


def test_generator_nudges_a_violating_point():
    """A seed whose raw scene has a pair within the margin comes out clean, no pair left out: the
    generator scales that point's distance range (deterministically), it drops nothing."""
    from orb_slam3_ros2_amd.synthetic import synthetic_fuse_scene
    a = synthetic_fuse_scene(60, 2000, 4, seed=5)      # 8000 pairs: some raw ratio falls within 2e-3
    b = synthetic_fuse_scene(60, 2000, 4, seed=5)
    assert a["points"].shape[0] == 2000 and np.array_equal(a["max_dist"], b["max_dist"])
    assert a["nudged"] > 0 and a["nudged"] == b["nudged"]
    assert fuse_level_margin(a["kfs"], a["points"], a["max_dist"]).min() > 2e-3
    ratio = a["max_dist"].astype(np.float64) / a["min_dist"]
    assert np.allclose(ratio, 1.2 ** 7, rtol=1e-5)


# ---- the symbol ----

def test_orbhip_fuse_is_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    assert re.search(r"^\s*int\s+orbhip_fuse\s*\(", src, re.M)
    from orb_slam3_ros2_amd import _lib
    assert "orbhip_fuse" in _lib.EXPORTED and hasattr(_lib.lib(), "orbhip_fuse")
    assert _lib.lib().orbhip_abi_version() == 1
    # argument checks that need no device
    assert _lib.lib().orbhip_fuse(None, None, 1, None, None, None, 3.0, None, None, None, None) == -1


# ---- the C++ mirror ----

def test_cpp_mirror_names_fuse(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tu = tmp_path / "fuse_mirror.cpp"
    tu.write_text('''#include "orbhip.hpp"
std::vector<int> fuse_all(orbhip_ctx* ctx, const std::vector<orbhip_frame>& kfs, const orbhip_local_points& mps,
                          const std::vector<uint8_t>& pair_skip, const std::vector<float>& inv_sigma2,
                          std::vector<std::vector<int>>& best, std::vector<std::vector<int>>& dist,
                          std::vector<std::vector<int>>& level) {
    orbhip::ORBmatcher matcher;
    std::vector<int> a = matcher.Fuse(ctx, kfs, mps, pair_skip, inv_sigma2, 3.0f, best);
    std::vector<int> b = matcher.Fuse(ctx, kfs, mps, pair_skip, inv_sigma2, 3.0f, best, &dist, &level);
    int (*c_entry)(orbhip_ctx*, const orbhip_frame*, int, const orbhip_local_points*, const uint8_t*, const float*,
                   float, int32_t*, int32_t*, int32_t*, int32_t*) = &orbhip_fuse;
    (void)c_entry;
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
''')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
