"""The stereo branches of SearchForTriangulation / CreateNewMapPoints on the CPU, no context: direct
cases of the restatement (tests/stereo_create_points_numpy.py) whose answers follow from the rule in
DESIGN.md "Stereo LocalMapping", the stereo_cos sweep of Decision 4, the reduction to the monocular
restatement, the conditions the stereo parity scenes must meet for
tests/test_stereo_create_points_gpu.py to mean something, and the claim against a sequential
simulation of upstream's loop.

A NaN depth never reaches status 12: stereo_cos of it is NaN, every comparison with it is false, and
the rule goes on to branch (d). The case is kept and asserts that."""
import collections
import os
import re

import numpy as np
import pytest

from orb_slam3_ros2_amd.matcher import ORBmatcher

import create_points_numpy as C
import stereo_create_points_numpy as S
import test_create_points as P
import triangulation_numpy as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SF, S2 = P.SF, P.S2
B_ST = 0.08
BF = float(f32(f32(P.CAM["fx"]) * f32(B_ST)))
IDENT = P.IDENT


def stereo_kf(pixel, octave, ur, depth, q=IDENT, c=(0, 0, 0), b=B_ST):
    """A one-feature stereo keyframe centred at c (ur < 0: a monocular feature)."""
    k = P.keyframe([pixel], [octave], q, P.pose_t(q, c))
    return S.with_stereo(k, [ur], [depth], BF, b)


def right(pixel, z):
    """The right coordinate of a pixel at depth z (float64)."""
    return pixel[0] - BF / z


def direct_cases():
    """name -> (kf1, kf2, status, source, monocular status, keyword arguments)."""
    cases = {}
    P4, c2 = np.array([0.3, -0.2, 4.0]), np.array([0.5, 0.0, 0.0])

    def add(name, k1, k2, status, source, mono, **kw):
        cases[name] = (k1, k2, status, source, mono, kw)
    # (a) with a stereo feature above cos_max: at 500 m the rays are 1e-3 rad apart (monocular: 3), the
    # stereo parallax of 0.08 m is 1.6e-4 rad, so cosP < cosS1 and the point is triangulated
    Pfar = P4 / 4.0 * 500.0
    p1, p2 = P.proj(Pfar), P.proj(Pfar, c=c2)
    add("a_stereo_above_cos_max", stereo_kf(p1, 0, right(p1, 500.0), 500.0), stereo_kf(p2, 0, -1, -1, c=c2), 1, 1, 3)
    # (b) / (c): a point 30 m away seen from 0.02 m apart: the stereo parallax (0.08 m) beats the rays'
    P30, cn = np.array([2.0, -1.0, 30.0]), np.array([0.02, 0.0, 0.0])
    p1, p2 = P.proj(P30), P.proj(P30, c=cn)
    add("b_unprojected_from_kf1", stereo_kf(p1, 0, right(p1, 30.0), 30.0), stereo_kf(p2, 0, -1, -1, c=cn), 1, 2, 3)
    add("c_unprojected_from_kf2", stereo_kf(p1, 0, -1, -1), stereo_kf(p2, 0, right(p2, 30.0), 30.0, c=cn), 1, 3, 3)
    # both stereo: only cosS1 is replaced. Feature 2's depth of 0.5 m would give a stereo parallax of
    # 0.16 rad and send the pair to (c) with a wrong point; the rule never looks at it
    cb = np.array([0.3, 0.0, 0.0])
    p1, p2 = P.proj(P30), P.proj(P30, c=cb)
    add("both_stereo_only_cosS1", stereo_kf(p1, 0, right(p1, 30.0), 30.0), stereo_kf(p2, 0, right(p2, 30.0), 0.5, c=cb),
        1, 1, 3)
    # (d) with a stereo feature: rays more than 90 degrees apart (cosS1 ~ 1 is neither below cosP nor
    # below cosS2 = cosP + 1), and a NaN depth (no comparison holds)
    p1 = P.proj(P4)
    add("d_rays_apart", stereo_kf(p1, 0, right(p1, 4.0), 4.0), stereo_kf((320.0, 240.0), 0, -1, -1, P.rot_y(100.0), c2),
        2, 0, 2)
    p2 = P.proj(P4, c=c2)
    add("d_nan_depth", stereo_kf(p1, 0, right(p1, 4.0), np.nan), stereo_kf(p2, 0, -1, -1, c=c2), 3, 0, 1)
    # status 12: the feature chosen for UnprojectStereo has no positive depth
    p1, p2 = P.proj(P30), P.proj(P30, c=cn)
    add("12_zero_depth_kf1", stereo_kf(p1, 0, right(p1, 30.0), 0.0), stereo_kf(p2, 0, -1, -1, c=cn), 12, 2, 3)
    add("12_negative_depth_kf1", stereo_kf(p1, 0, right(p1, 30.0), -30.0), stereo_kf(p2, 0, -1, -1, c=cn), 12, 2, 3)
    add("12_zero_depth_kf2", stereo_kf(p1, 0, -1, -1), stereo_kf(p2, 0, right(p2, 30.0), 0.0, c=cn), 12, 3, 3)
    # 7 / 8 by the right coordinate alone: exact pixels (eX = eY ~ 0), eR on both sides of
    # sqrt(7.8) sigma = 2.7928 sigma, at octaves 0 and 3
    for o in (0, 3):
        sig = float(SF[o])
        p1, p2 = P.proj(P4), P.proj(P4, c=c2)
        for k, st in ((2.79, 1), (2.80, 7), (-2.79, 1), (-2.80, 7)):
            add(f"7_ur_{k}_sigma_octave{o}", stereo_kf(p1, o, right(p1, 4.0) - k * sig, 4.0),
                stereo_kf(p2, o, -1, -1, c=c2), st, 1, 1)
        for k, st in ((2.79, 1), (2.80, 8), (-2.79, 1), (-2.80, 8)):
            add(f"8_ur_{k}_sigma_octave{o}", stereo_kf(p1, o, -1, -1),
                stereo_kf(p2, o, right(p2, 4.0) - k * sig, 4.0, c=c2), st, 1, 1)
    return cases


DIRECT = direct_cases()


def run_direct(name, stereo=True):
    k1, k2, _, _, _, kw = DIRECT[name]
    f1, f2 = (S.feature(k1, 0), S.feature(k2, 0)) if stereo else (S.MONO, S.MONO)
    det = {}
    st, X, src = S.triangulate_pair(C.Camera(k1), C.Camera(k2), k1.kps[0], k2.kps[0], f1, f2, SF, S2, detail=det, **kw)
    return st, X, src, det


@pytest.mark.parametrize("name", list(DIRECT))
def test_direct_case(name):
    k1, k2, want, source, mono, kw = DIRECT[name]
    st, X, src, det = run_direct(name)
    assert (st, src) == (want, source), (name, st, src, det)
    # without the stereo members the rule is the monocular one, which create_points_numpy states
    st0, X0, src0, _ = run_direct(name, stereo=False)
    m_st, m_X = C.triangulate_pair(C.Camera(k1), C.Camera(k2), k1.kps[0], k2.kps[0], SF, S2, **kw)
    assert st0 == m_st == mono and np.array_equal(X0.view(np.uint32), m_X.view(np.uint32))
    assert src0 == (1 if m_st not in (2, 3) else 0)
    if name in ("b_unprojected_from_kf1", "c_unprojected_from_kf2"):
        # fp32 unprojection of a point 30 m away: a dozen roundings of 2^-24 relative on 30 m: < 5e-5 m
        assert np.abs(X.astype(np.float64) - [2.0, -1.0, 30.0]).max() < 5e-5
    if name == "both_stereo_only_cosS1":
        assert det["cosS2"] == det["cosP"] + f32(1.0) and det["cosS1"] < f32(1.0)
        assert float(S.stereo_cos(B_ST, 0.5)) < float(det["cosP"])        # what cosS2 would have been
    if want == 12 or want in (2, 3):
        assert not X.any()


def test_stereo_cos_sweep():
    """Decision 4 on 2,000,000 samples (b in 0.03 .. 0.6, d in 0.2 .. 60): the closed form in fp64,
    rounded once, equals the correctly rounded float32 of float64 cos(2 atan2(b / 2, d)) on every
    sample. Finding (printed, not asserted): the fp32 chain cosf(2 atan2f(b / 2, d)) differs from that
    value on a fraction of the samples (0.56 % where this was first measured)."""
    rng = np.random.Generator(np.random.PCG64(4))
    b = rng.uniform(0.03, 0.6, 2_000_000).astype(f32)
    d = rng.uniform(0.2, 60.0, 2_000_000).astype(f32)
    h, D = b.astype(np.float64) * 0.5, d.astype(np.float64)
    closed = ((D * D - h * h) / (D * D + h * h)).astype(f32)
    exact = np.cos(2.0 * np.arctan2(h, D)).astype(f32)
    assert np.array_equal(closed, exact), int((closed != exact).sum())
    chain = np.cos(f32(2.0) * np.arctan2(b * f32(0.5), d)).astype(f32)
    print(f"fp32 chain differs on {100.0 * (chain != exact).mean():.2f} % of the samples")
    for i in range(0, 2_000_000, 4001):           # the scalar restatement is the same function
        assert S.stereo_cos(b[i], d[i]) == closed[i]


def test_epipole_radius_pair_is_matched_by_the_stereo_search_only():
    """KF2 0.5 m ahead on the optical axis: its epipole is the principal point, and the point's twin
    lies 0.6 px from it. The monocular search excludes the pair; with either feature stereo it matches."""
    Pt, c2 = np.array([0.004, 0.002, 4.0]), (0.0, 0.0, 0.5)
    p1, p2 = P.proj(Pt), P.proj(Pt, c=c2)
    assert np.hypot(p2[0] - 320.0, p2[1] - 240.0) < 1.0
    k1m, k2m = P.keyframe([p1], [0]), P.keyframe([p2], [0], t=P.pose_t(IDENT, c2))
    n, m, cnt = T.search_pair(k1m, k2m, SF, S2, 0)
    assert n == 0 and cnt["epipole"] == 1
    for s1, s2 in ((True, False), (False, True), (True, True)):
        k1 = S.with_stereo(k1m, [right(p1, 4.0) if s1 else -1], [4.0 if s1 else -1], BF, B_ST)
        k2 = S.with_stereo(k2m, [right(p2, 3.5) if s2 else -1], [3.5 if s2 else -1], BF, B_ST)
        n, m, cnt = S.search_pair(k1, k2, SF, S2, 0)
        assert n == 1 and m.tolist() == [0] and cnt["epipole_radius"] == 1 and cnt["epi_matches"] == 1
    n, m, cnt = S.search_pair(S.all_mono(k1m), S.all_mono(k2m), SF, S2, 0)
    assert n == 0 and cnt["epipole"] == 1


def test_mb_gate_on_both_sides_of_the_baseline():
    k1 = P.keyframe([(1, 1)], [0])
    k2 = P.keyframe([(1, 1)], [0], t=P.pose_t(IDENT, (0.5, 0, 0)))
    cam1, cam2 = C.Camera(k1), C.Camera(k2)
    assert not S.gated(cam1, cam2, f32(0.5))                         # baseline == b: not below it
    assert S.gated(cam1, cam2, np.nextafter(f32(0.5), f32(1)))
    assert not S.gated(cam1, cam2, np.nextafter(f32(0.5), f32(0)))
    r = S.create_new_map_points(S.all_mono(k1), [S.all_mono(k2, b=0.6)], SF, S2, 0)
    assert r.gated.tolist() == [1] and r.nmatches.tolist() == [0] and not r.status.any() and (r.match12 == -1).all()


# ---- reduction ----
@pytest.mark.parametrize("k", range(len(P.PARITY_SEEDS)))
def test_no_stereo_feature_reduces_to_the_monocular_restatement(k):
    """Every u_right = -1 and b below every baseline: the monocular rule without median_depth."""
    s = P.parity_scene(k)
    want = C.create_new_map_points(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 0, None,
                                   far=s["far_threshold"])
    got = S.create_new_map_points(S.all_mono(s["kf1"]), [S.all_mono(x) for x in s["neighbours"]], s["scale_factors"],
                                  s["level_sigma2"], 0, far=s["far_threshold"])
    assert not got.gated.any() and got.n == want.n > 0
    for name in ("match12", "nmatches", "gated", "status", "first", "nnew", "new_nbr", "new_idx1", "new_idx2"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    assert np.array_equal(got.x3d_all.view(np.uint32), want.x3d_all.view(np.uint32))
    assert np.array_equal(np.ascontiguousarray(got.new_x3d).view(np.uint32),
                          np.ascontiguousarray(want.new_x3d).view(np.uint32))
    assert np.array_equal(got.source, ((want.status == 1) | (want.status >= 4)).astype(np.uint8))


# ---- the stereo parity scene set ----
PARITY_SEEDS = (0, 1, 2)
_cache = {}


def parity_scene(k):
    """Stereo scene k: n = 300, B = 3 plus the neighbour gated by mb (built once; read-only)."""
    if k not in _cache:
        from orb_slam3_ros2_amd.synthetic import synthetic_stereo_new_points_scene
        _cache[k] = synthetic_stereo_new_points_scene(300, 3, PARITY_SEEDS[k])
    return _cache[k]


def parity_result(k):
    """(result, details, search counters) of the restatement on scene k, check_orientation = 0 (cached)."""
    key = ("r", k)
    if key not in _cache:
        s = parity_scene(k)
        det, cnt = [], []
        r = S.create_new_map_points(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 0,
                                    far=s["far_threshold"], details=det, counters=cnt)
        _cache[key] = (r, det, cnt)
    return _cache[key]


def test_stereo_parity_scene_conditions():
    for k in range(len(PARITY_SEEDS)):
        s = parity_scene(k)
        r, det, cnt = parity_result(k)
        k1, nb = s["kf1"], s["neighbours"]
        assert len(nb) == 4 and k1.n == 300
        assert r.gated.tolist() == [0, 1, 0, 0]                       # one neighbour gated by mb
        assert r.nmatches[1] == 0 and (r.nmatches[[0, 2, 3]] > 0).all()
        assert r.n >= 50
        a_stereo = sum(1 for b, i, _ in det if r.source[b, i] == 1
                       and (k1.u_right[i] >= 0 or nb[b].u_right[r.match12[b, i]] >= 0))
        n_b, n_c = int((r.source == 2).sum()), int((r.source == 3).sum())
        mono7 = sum(1 for _, _, d in det if d.get("mono7"))
        mono8 = sum(1 for _, _, d in det if d.get("mono8"))
        epi = sum(c["epi_matches"] for c in cnt if c)
        st = collections.Counter(r.status.ravel().tolist())
        print(f"scene {k}: {r.n} new points, branches a-with-stereo {a_stereo} b {n_b} c {n_c}, 7 / 8 by the right "
              f"coordinate alone {mono7} / {mono8}, epipole-radius matches {epi}, status {dict(st)}")
        assert a_stereo >= 10 and n_b >= 10 and n_c >= 10
        assert mono7 >= 3 and mono8 >= 3
        assert epi >= 3
        for kf in [k1] + nb:                                          # stereo and monocular features mixed
            assert (kf.u_right >= 0).sum() >= 30 and (kf.u_right < 0).sum() >= 30


@pytest.mark.parametrize("k", range(len(PARITY_SEEDS)))
def test_claim_equals_the_sequence(k):
    """Upstream's sequential loop under the stereo rule yields exactly the batched list, check_orientation = 0."""
    s = parity_scene(k)
    r = parity_result(k)[0]
    nbr, idx1, idx2, x3d = S.sequential(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 0,
                                        far=s["far_threshold"])
    assert nbr.tolist() == r.new_nbr.tolist() and idx1.tolist() == r.new_idx1.tolist()
    assert idx2.tolist() == r.new_idx2.tolist()
    assert np.array_equal(x3d.view(np.uint32), np.ascontiguousarray(r.new_x3d).view(np.uint32))
    assert len(nbr) >= 50


def test_stereo_scene_leaves_the_monocular_generators_alone():
    from orb_slam3_ros2_amd.synthetic import synthetic_new_points_scene, synthetic_stereo_new_points_scene
    a = synthetic_new_points_scene(80, 2, seed=5)
    synthetic_stereo_new_points_scene(80, 2, seed=5)
    b = synthetic_new_points_scene(80, 2, seed=5)
    for ka, kb in zip([a["kf1"]] + a["neighbours"], [b["kf1"]] + b["neighbours"]):
        for name in ("kps", "desc", "node", "weight", "has_mp", "pose_q", "pose_t"):
            assert np.array_equal(getattr(ka, name), getattr(kb, name)), name
        assert ka.u_right is None


# ---- the symbols, the dispatch ----
def test_stereo_symbols_are_declared_and_exported():
    src = open(os.path.join(ROOT, "include", "orbhip.h")).read()
    from orb_slam3_ros2_amd import _lib
    for name in ("orbhip_search_for_triangulation_stereo", "orbhip_create_new_map_points_stereo",
                 "orbhip_triangulate_matches_stereo"):
        assert re.search(r"^\s*int\s+" + name + r"\s*\(", src, re.M)
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
    assert "orbhip_tri_stereo_keyframe" in src
    L = _lib.lib()
    assert L.orbhip_search_for_triangulation_stereo(None, None, None, 1, None, None, 8, 0, None, None) == -1
    assert L.orbhip_create_new_map_points_stereo(None, None, None, 1, None, None, 8, 0, None, None, None) == -1


def test_python_refuses_mixed_keyframes_and_a_median_depth():
    k1, k2 = DIRECT["b_unprojected_from_kf1"][:2]
    mono2 = P.keyframe([(1, 1)], [0])
    mt = ORBmatcher.__new__(ORBmatcher)           # no context: the checks come first
    with pytest.raises(ValueError):
        mt.SearchForTriangulation(k1, [k2, mono2], SF, S2)
    with pytest.raises(ValueError):
        mt.CreateNewMapPoints(mono2, [k2], SF, S2)
    with pytest.raises(ValueError):
        mt.CreateNewMapPoints(k1, [k2], SF, S2, median_depth=[4.0])


def test_cpp_mirror_names_the_stereo_calls(tmp_path):
    import shutil
    import subprocess
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    tu = tmp_path / "stereo_new_points_mirror.cpp"
    tu.write_text('''#include "orbhip.hpp"
size_t all(orbhip_ctx* ctx, const orbhip_tri_stereo_keyframe& kf1, const std::vector<orbhip_tri_stereo_keyframe>& nbrs,
           const std::vector<float>& sf, const std::vector<float>& s2) {
    orbhip::ORBmatcher matcher(0.6f, false);
    std::vector<std::vector<int>> m12;
    std::vector<uint8_t> gated, source;
    matcher.SearchForTriangulation(ctx, kf1, nbrs, sf, s2, m12);
    auto a = matcher.CreateNewMapPoints(ctx, kf1, nbrs, sf, s2, 1.5f * sf[1]);
    auto b = matcher.CreateNewMapPoints(ctx, kf1, nbrs, sf, s2, 1.5f * sf[1], 0.9998, 0.f, &gated, &source);
    auto c = matcher.TriangulateMatches(ctx, kf1, nbrs, m12, sf, s2, 1.5f * sf[1], 0.9998, 0.f, &source);
    int (*e1)(orbhip_ctx*, const orbhip_tri_stereo_keyframe*, const orbhip_tri_stereo_keyframe*, int, const float*,
              const float*, int, int, int32_t*, int32_t*) = &orbhip_search_for_triangulation_stereo;
    int (*e2)(orbhip_ctx*, const orbhip_tri_stereo_keyframe*, const orbhip_tri_stereo_keyframe*, int, const float*,
              const float*, int, int, const orbhip_tri_params*, orbhip_new_points*, uint8_t*) =
        &orbhip_create_new_map_points_stereo;
    int (*e3)(orbhip_ctx*, const orbhip_tri_stereo_keyframe*, const orbhip_tri_stereo_keyframe*, int, const int32_t*,
              const float*, const float*, int, const orbhip_tri_params*, orbhip_new_points*, uint8_t*) =
        &orbhip_triangulate_matches_stereo;
    (void)e1; (void)e2; (void)e3;
    return a.size() + b.size() + c.size();
}
''')
    r = subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
