"""The stereo branch of ORBmatcher::Fuse on the CPU, no context: direct cases of the restatement
(tests/stereo_fuse_numpy.py) whose answers follow from the rule in DESIGN.md "Stereo LocalMapping";
the reduction to the monocular restatement; the conditions the stereo parity scenes must meet for
tests/test_stereo_fuse_gpu.py to mean something; the symbol, the Python dispatch and the C++ mirror."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import (fuse_level_margin, orb_scale_tables, synthetic_fuse_scene,
                                          synthetic_stereo_fuse_scene)

import fuse_numpy as F
import stereo_fuse_numpy as SF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
_, S2 = orb_scale_tables()
INV_S2 = (f32(1.0) / S2).astype(f32)
CASES = SF.direct_cases()


# ---- direct cases ----

@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_direct_case(c):
    """The stereo restatement gives the answer the definition gives, and the monocular restatement on
    the same keyframe without u_right gives the monocular answer."""
    if c["chi2"] is not None and "sigma" in c["name"]:
        # the planted error lies on the side of 7.8 the case means, by more than fp32 rounding
        assert (c["chi2"] <= 7.8) == (c["want"][0] == 0) and abs(c["chi2"] - 7.8) > 1e-2
    nf, idx, dist, lvl, cnt = SF.fuse_stereo([c["kf"]], *SF.direct_args(c), INV_S2, 3.0)
    assert (int(idx[0, 0]), int(dist[0, 0])) == c["want"] and lvl[0, 0] == c["octave"] and nf[0] == (c["want"][0] == 0)
    assert cnt["cand_stereo"] + cnt["cand_mono"] == 1 and cnt["cand_stereo"] == (c["chi2"] is not None)
    _, idx, dist, _, _ = F.fuse([SF.mono_keyframe(c["kf"])], *SF.direct_args(c), INV_S2, 3.0)
    assert (int(idx[0, 0]), int(dist[0, 0])) == c["mono"]


def test_direct_cases_cover_both_sides_of_both_bounds():
    by = {c["name"]: c for c in CASES}
    for o in (0, 7):
        c = by[f"uv_2.6_sigma_perfect_ur_octave{o}"]
        assert 5.99 < c["chi2"] < 7.8 and abs(c["chi2"] - 2.6 ** 2) < 1e-2       # er = 0: the (u, v) terms alone
        assert abs(by[f"ur_2.79_sigma_octave{o}"]["chi2"] - 2.79 ** 2) < 1e-2
        assert abs(by[f"ur_2.80_sigma_octave{o}"]["chi2"] - 2.80 ** 2) < 1e-2
    assert by["ur_zero_is_stereo"]["chi2"] > 1e3 and by["ur_nan_is_monocular"]["chi2"] is None


def test_right_projection_is_u_minus_bf_over_z_to_fp32_accuracy():
    c = CASES[0]
    g = F.Grid(c["kf"])
    P = [f32(x) for x in c["pt"]["P"]]
    Pc = F.step1_camera(g, P)
    u, _ = F.step2_project(g, Pc)
    want = float(u) - float(f32(c["kf"].bf)) / float(Pc[2])
    assert abs(float(SF.right_projection(g, c["kf"].bf, Pc, u)) - want) < 1e-4


# ---- reduction ----

@pytest.mark.parametrize("k", range(len(F.PARITY_SCENES)))
def test_every_ur_minus_one_reduces_to_the_monocular_restatement(k):
    s = F.parity_scene(k)
    kfs = [SF.stereo_keyframe(kf, np.full(kf.kps.shape[0], -1.0, f32), 30.0, 0.08) for kf in s["kfs"]]
    got = SF.fuse_stereo_scene(dict(s, ratios=None), kfs=kfs)
    for g, w in zip(got[:4], s["expected"][:4]):
        assert np.array_equal(g, w)
    for key in F.COUNTERS:
        assert got[4][key] == s["expected"][4][key], key
    assert got[4]["cand_stereo"] == 0 and got[4]["only_78"] == 0 and got[4]["only_er"] == 0


# ---- conditions of the stereo parity scene set ----

def test_stereo_parity_scene_conditions():
    for k in range(len(SF.PARITY_SCENES)):
        s = SF.parity_scene(k)
        nf, idx, dist, lvl, cnt = s["expected"]
        n = s["points"].shape[0]
        print(f"scene {k}: fused {nf.tolist()} counters {cnt}")
        assert idx.shape == (3, 300) and all(kf.kps.shape[0] == 300 for kf in s["kfs"])
        assert cnt["only_78"] >= 10            # candidates accepted only because of 7.8
        assert cnt["only_er"] >= 10            # candidates rejected only because of er
        for kf in s["kfs"]:                    # stereo and monocular keypoints mixed in every keyframe
            assert (kf.u_right >= 0).sum() >= 30 and (kf.u_right < 0).sum() >= 30
            assert kf.bf > 0 and kf.b > 0
        assert cnt["cand_stereo"] >= 100 and cnt["cand_mono"] >= 30
        assert (nf * 4 >= n).all(), nf
        # the stereo rule decides differently from the monocular one on these scenes, both ways
        mono = F.fuse_scene(dict(s, ratios=None), kfs=s["mono_kfs"])
        gained, lost = (idx >= 0) & (mono[1] < 0), (idx < 0) & (mono[1] >= 0)
        print(f"scene {k}: {int(gained.sum())} pairs fused only by the stereo rule, {int(lost.sum())} only by the monocular")
        assert gained.sum() >= 5 and lost.sum() >= 5
        # PredictScale's ceil is more than 1e-3 away from a step for EVERY pair that reaches it:
        # the GPU comparison leaves no pair out
        reached = {(b, m) for b, m, _ in s["ratios"]}
        assert reached == {(int(b), int(m)) for b, m in np.argwhere(lvl >= 0)}
        margin = min(abs(x - round(x)) for _, _, x in s["ratios"])
        print(f"scene {k}: level margin {margin:.2e} over {len(reached)} pairs")
        assert margin > 1e-3
        assert fuse_level_margin(s["kfs"], s["points"], s["max_dist"]).min() > 2e-3


def test_stereo_scene_leaves_the_monocular_scene_alone():
    """The stereo scene draws from a generator of its own: the base scene is what it was."""
    a = synthetic_fuse_scene(80, 70, 2, seed=9)
    s = synthetic_stereo_fuse_scene(80, 70, 2, seed=9)
    b = synthetic_fuse_scene(80, 70, 2, seed=9)
    for key in ("points", "normals", "min_dist", "max_dist", "mp_desc", "skip", "pair_skip"):
        assert np.array_equal(a[key], b[key]) and np.array_equal(a[key], s[key])
    for ka, kb, ks in zip(a["kfs"], b["kfs"], s["kfs"]):
        assert np.array_equal(ka.kps, kb.kps) and np.array_equal(ka.desc, kb.desc)
        assert np.array_equal(ka.desc, ks.desc) and np.array_equal(ka.kps["octave"], ks.kps["octave"])
        assert ka.u_right is None and ks.u_right.shape == (80,)


def test_walk_result_is_the_key_minimum_under_the_stereo_gate():
    """The reference's walk (strict <, first wins) equals the minimum of (dist, cell, idx) over the
    candidates the stereo gate passes: recomputed from scratch for every pair of a parity scene."""
    s = SF.parity_scene(0)
    _, idx, dist, lvl, _ = s["expected"]
    for b, kf in enumerate(s["kfs"]):
        g = F.Grid(kf)
        for m in range(idx.shape[1]):
            if lvl[b, m] < 0:
                continue
            L = int(lvl[b, m])
            Pc = F.step1_camera(g, [f32(x) for x in s["points"][m]])
            u, v = F.step2_project(g, Pc)
            urp = SF.right_projection(g, kf.bf, Pc, u)
            keys = []
            for cell, j in F.step8_area(g, u, v, F.step7_radius(g, s["th"], L)):
                o = int(g.octave[j])
                ex, ey = u - g.x[j], v - g.y[j]
                e2 = ex * ex + ey * ey
                if kf.u_right[j] >= 0:
                    er = urp - kf.u_right[j]
                    ok = not np.float64((e2 + er * er) * INV_S2[o]) > 7.8
                else:
                    ok = not np.float64(e2 * INV_S2[o]) > 5.99
                if L - 1 <= o <= L and ok:
                    keys.append((int(F._POP[g.desc[j] ^ s["mp_desc"][m]].sum()), cell, j))
            best = min(keys) if keys else (256, -1, -1)
            assert dist[b, m] == best[0] and idx[b, m] == (best[2] if best[0] <= 50 else -1)


# ---- the symbol, the dispatch, the C++ mirror ----

def test_orbhip_fuse_stereo_is_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    assert re.search(r"^\s*int\s+orbhip_fuse_stereo\s*\(", src, re.M)
    from orb_slam3_ros2_amd import _lib
    assert "orbhip_fuse_stereo" in _lib.EXPORTED and hasattr(_lib.lib(), "orbhip_fuse_stereo")
    # argument checks that need no device
    assert _lib.lib().orbhip_fuse_stereo(None, None, 1, None, None, None, 3.0, None, None, None, None) == -1


def test_python_fuse_refuses_mixed_keyframes():
    """All keyframes of a call carry u_right or none does: ValueError before the library is called."""
    from orb_slam3_ros2_amd.matcher import ORBmatcher
    c = CASES[0]
    mt = ORBmatcher.__new__(ORBmatcher)          # no context: the check comes first
    for kfs in ([c["kf"], SF.mono_keyframe(c["kf"])], [SF.mono_keyframe(c["kf"]), c["kf"]]):
        with pytest.raises(ValueError):
            mt.Fuse(kfs, *SF.direct_args(c), INV_S2, 3.0)


def test_cpp_mirror_names_the_stereo_fuse(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tu = tmp_path / "stereo_fuse_mirror.cpp"
    tu.write_text('''#include "orbhip.hpp"
std::vector<int> fuse_all(orbhip_ctx* ctx, const std::vector<orbhip_stereo_view>& kfs, const orbhip_local_points& mps,
                          const std::vector<uint8_t>& pair_skip, const std::vector<float>& inv_sigma2,
                          std::vector<std::vector<int>>& best, std::vector<std::vector<int>>& dist,
                          std::vector<std::vector<int>>& level) {
    orbhip::ORBmatcher matcher;
    std::vector<int> a = matcher.Fuse(ctx, kfs, mps, pair_skip, inv_sigma2, 3.0f, best);
    std::vector<int> b = matcher.Fuse(ctx, kfs, mps, pair_skip, inv_sigma2, 3.0f, best, &dist, &level);
    int (*c_entry)(orbhip_ctx*, const orbhip_stereo_view*, int, const orbhip_local_points*, const uint8_t*,
                   const float*, float, int32_t*, int32_t*, int32_t*, int32_t*) = &orbhip_fuse_stereo;
    (void)c_entry;
    a.insert(a.end(), b.begin(), b.end());
    return a;
}
''')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
