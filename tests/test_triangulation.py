"""SearchForTriangulation on the CPU: the host geometry (orbhip_triangulation_geometry) against the
numpy restatement bit for bit and against float64; the restatement itself against cases whose answer
follows from the rule's definition; and the Conditions of the parity scene set, so that the GPU
parity test (tests/test_triangulation_gpu.py) is known to exercise every gate."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, TriKeyFrameC, lib
from orb_slam3_ros2_amd.matcher import TriKeyFrame
from orb_slam3_ros2_amd.synthetic import (D435I, _mat_to_quat, _rodrigues, orb_scale_tables, pinhole_project,
                                          quat_to_rot64, synthetic_triangulation_scene)

import triangulation_numpy as T

CAM = D435I
SF, S2 = orb_scale_tables()


def _camera_only(q, t, cam=CAM):
    """A keyframe without features: all the geometry reads is the pose and the intrinsics."""
    z = np.zeros(0)
    return TriKeyFrame(np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8), z, z, z, q, t, cam["fx"], cam["fy"],
                       cam["cx"], cam["cy"])


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).reshape(-1).tolist()


def _assert_geometry_bit_exact(k1, k2):
    F, ep = k1.geometry(k2)
    Fn, epn = T.geometry(k1, k2)
    assert _bits(F) == _bits(Fn), (F, Fn)
    assert _bits(ep) == _bits(epn), (ep, epn)
    return F, ep


def test_geometry_bit_exact_random_poses():
    rng = np.random.default_rng(42)
    for k in range(50):
        q1 = _mat_to_quat(_rodrigues(rng.normal(size=3) * 0.8)).astype(np.float32)
        q2 = _mat_to_quat(_rodrigues(rng.normal(size=3) * 0.8)).astype(np.float32)
        cam2 = dict(fx=CAM["fx"] * rng.uniform(0.7, 1.3), fy=CAM["fy"] * rng.uniform(0.7, 1.3),
                    cx=CAM["cx"] + rng.normal() * 10, cy=CAM["cy"] + rng.normal() * 10)
        k1 = _camera_only(q1, rng.normal(size=3).astype(np.float32))
        k2 = _camera_only(q2, rng.normal(size=3).astype(np.float32), cam2 if k % 2 else CAM)
        F, ep = _assert_geometry_bit_exact(k1, k2)
        assert np.isfinite(F).all() and np.abs(F).max() > 0


def test_geometry_identity_relative_pose_is_all_zero():
    """t12 = 0: F12 = 0, so den == 0 for every KF1 feature and nothing matches."""
    q = np.array([0, 0, 0, 1], np.float32)
    t = np.array([0.25, -0.5, 1.0], np.float32)
    k1, k2 = _camera_only(q, t), _camera_only(q, t)
    F, _ = _assert_geometry_bit_exact(k1, k2)
    assert (F == 0).all()
    s = _mini_pair()
    kf1, kf2 = s["kf1"], s["kf2"]
    kf2.pose_q, kf2.pose_t = kf1.pose_q.copy(), kf1.pose_t.copy()
    kf2.kps["x"], kf2.kps["y"] = kf1.kps["x"], kf1.kps["y"]
    kf1.pose_q[:] = q
    kf2.pose_q[:] = q
    n, m, cnt = T.search_pair(kf1, kf2, SF, S2, 0)
    assert n == 0 and (m == -1).all() and cnt["epiline"] + cnt["epipole"] == kf1.n


def test_geometry_sideways_baseline_epipole_far_outside():
    q = np.array([0, 0, 0, 1], np.float32)
    k1 = _camera_only(q, np.array([0.0, 0.0, 0.0], np.float32))
    k2 = _camera_only(q, np.array([-0.3, 0.0, 1e-4], np.float32))   # C2 = (-0.3, 0, 1e-4): C2z != 0
    F, ep = _assert_geometry_bit_exact(k1, k2)
    assert np.isfinite(ep).all() and abs(ep[0]) > 1e5
    # an exactly sideways baseline (C2z == 0) divides by zero: the same bits on both sides, inf or nan
    k3 = _camera_only(q, np.array([-0.3, 0.0, 0.0], np.float32))
    _, ep3 = _assert_geometry_bit_exact(k1, k3)
    assert not np.isfinite(ep3).all()


def _f64_closed_form(k1, k2):
    R1, R2 = quat_to_rot64(k1.pose_q), quat_to_rot64(k2.pose_q)
    t1, t2 = k1.pose_t.astype(np.float64), k2.pose_t.astype(np.float64)
    R12 = R1 @ R2.T
    t12 = t1 - R12 @ t2
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])

    def kinv(k):
        fx, fy, cx, cy = (float(np.float32(v)) for v in (k.fx, k.fy, k.cx, k.cy))
        return np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]]), (fx, fy, cx, cy)
    K1i, _ = kinv(k1)
    K2i, (fx2, fy2, cx2, cy2) = kinv(k2)
    C2 = R2 @ (-R1.T @ t1) + t2
    return K1i.T @ tx @ R12 @ K2i, np.array([fx2 * C2[0] / C2[2] + cx2, fy2 * C2[1] / C2[2] + cy2])


def test_geometry_against_float64():
    """The formula, not the bits: F12 against the float64 closed form, and the epipolar distance of
    noise-free correspondences below 0.05 px (fp32 round-off at 640 x 480 is about 1e-3 px)."""
    rng = np.random.default_rng(3)
    for seed in range(3):
        s = synthetic_triangulation_scene(60, 3, seed)
        k1 = s["kf1"]
        for b, k2 in enumerate(s["neighbours"]):
            F, ep = k1.geometry(k2)
            F64, ep64 = _f64_closed_form(k1, k2)
            # every entry is a sum of <= 3 products of quantities bounded by max |F64| / min(1/f) ...:
            # about 20 fp32 roundings (2^-24 each) of intermediates no larger than |t12| ~ max |F64| * f,
            # scaled back by 1/f: well below 200 * 2^-24 ~ 1.2e-5 of the largest entry
            assert np.abs(F.astype(np.float64) - F64).max() <= 1.2e-5 * np.abs(F64).max()
            if b % 3 == 1:   # the forward neighbour: |C2z| ~ 0.45, a well-conditioned quotient
                assert np.abs(ep - ep64).max() <= 1e-3 * max(1.0, np.abs(ep64).max())
            # noise-free correspondences of the two cameras
            z = rng.uniform(2, 8, 200)
            X1 = np.stack([rng.uniform(-0.4, 0.4, 200) * z, rng.uniform(-0.3, 0.3, 200) * z, z], 1)
            Pw = (X1 - k1.pose_t.astype(np.float64)) @ quat_to_rot64(k1.pose_q)
            x1, _ = pinhole_project(k1.pose_q, k1.pose_t, s["cam"], Pw)
            x2, _ = pinhole_project(k2.pose_q, k2.pose_t, s["cam"], Pw)
            Fd = F.astype(np.float64)
            h1 = np.concatenate([x1, np.ones((200, 1))], 1)
            line = h1 @ Fd                                       # rows: (a, b, c) = x1^T F12
            num = (line[:, :2] * x2).sum(1) + line[:, 2]
            d = np.abs(num) / np.sqrt(line[:, 0] ** 2 + line[:, 1] ** 2)
            assert d.max() < 0.05, d.max()


def test_geometry_null_arguments():
    k = TriKeyFrameC()
    F = (ctypes.c_float * 9)()
    ep = (ctypes.c_float * 2)()
    L = lib()
    assert L.orbhip_triangulation_geometry(None, ctypes.byref(k), F, ep) == -1
    assert L.orbhip_triangulation_geometry(ctypes.byref(k), ctypes.byref(k), None, ep) == -1


# ---- restatement KATs: cases whose answer follows from the definition ----

def _mini_pair(m=12, forward=False, seed=0):
    """Two keyframes seeing m points, noise free: KF2 feature j is the twin of KF1 feature j
    (identical descriptors, one node, no MapPoints, octave 0, equal angles). KF2 moves sideways, or
    forward along the optical axis (epipole inside the image)."""
    rng = np.random.default_rng(seed)
    q1 = np.array([0, 0, 0, 1], np.float32)
    t1 = np.zeros(3, np.float32)
    c = np.array([0.0, 0.0, 0.5]) if forward else np.array([0.4, 0.0, 0.0])
    Rrel = _rodrigues(np.array([0.01, -0.02, 0.015]))
    q2 = _mat_to_quat(Rrel).astype(np.float32)
    t2 = (Rrel @ (-c)).astype(np.float32)
    z = rng.uniform(2, 6, m)
    u, v = rng.uniform(60, 580, m), rng.uniform(60, 420, m)
    Pw = np.stack([(u - CAM["cx"]) / CAM["fx"] * z, (v - CAM["cy"]) / CAM["fy"] * z, z], 1)
    return _pair_from_points(Pw, q1, t1, q2, t2, rng)


def _pair_from_points(Pw, q1, t1, q2, t2, rng):
    m = Pw.shape[0]
    desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    kfs = []
    for q, t in ((q1, t1), (q2, t2)):
        uv, depth = pinhole_project(q, t, CAM, Pw)
        assert (depth > 0).all()
        k = np.zeros(m, KP_DTYPE)
        k["x"], k["y"] = uv[:, 0].astype(np.float32), uv[:, 1].astype(np.float32)
        k["size"] = 31.0
        kfs.append(TriKeyFrame(k, desc.copy(), np.full(m, 77, np.int32), np.ones(m), np.zeros(m, np.uint8), q, t,
                               CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"]))
    return dict(kf1=kfs[0], kf2=kfs[1], Pw=Pw)


def _append(kf, j, **over):
    """A copy of kf with feature j appended again (fields overridden by `over`)."""
    k = np.concatenate([kf.kps, kf.kps[j:j + 1]])
    for f in ("x", "y", "octave", "angle"):
        if f in over:
            k[f][-1] = over[f]
    return TriKeyFrame(k, np.concatenate([kf.desc, over.get("desc", kf.desc[j])[None]]),
                       np.append(kf.node, over.get("node", kf.node[j])), np.append(kf.weight, kf.weight[j]),
                       np.append(kf.has_mp, over.get("has_mp", kf.has_mp[j])), kf.pose_q, kf.pose_t, kf.fx, kf.fy,
                       kf.cx, kf.cy)


def _flip(desc, bits):
    d = desc.copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _run(s, ori=0):
    return T.search_pair(s["kf1"], s["kf2"], SF, S2, ori)


def test_kat_twins_match():
    s = _mini_pair()
    n, m, cnt = _run(s)
    assert n == s["kf1"].n and m.tolist() == list(range(s["kf1"].n))
    assert cnt == dict(epipole=0, epiline=0, ties=0, shared=0, pruned=0)
    assert _run(s, 1)[1].tolist() == m.tolist()   # equal angles: one rotation bin, nothing pruned


def test_kat_mappoints_are_neither_source_nor_target():
    s = _mini_pair()
    s["kf2"].has_mp[3] = 1
    s["kf1"].has_mp[5] = 1
    n, m, _ = _run(s)
    assert m[3] == -1 and m[5] == -1 and n == s["kf1"].n - 2
    assert 3 not in m.tolist()


def test_kat_other_node_weight_zero_and_no_node_never_match():
    s = _mini_pair()
    s["kf2"].node[1] = 78          # another node
    s["kf1"].weight[2] = 0.0       # not in KF1's FeatureVector
    s["kf2"].weight[4] = 0.0       # not in KF2's
    s["kf1"].node[6] = -1
    s["kf2"].node[7] = -1
    n, m, _ = _run(s)
    assert [m[i] for i in (1, 2, 4, 6, 7)] == [-1] * 5 and n == s["kf1"].n - 5


def test_kat_equal_distance_the_higher_index_wins():
    s = _mini_pair()
    m0 = s["kf1"].n
    s["kf2"] = _append(s["kf2"], 4)                       # an exact copy of twin 4 at index m0
    n, m, cnt = _run(s)
    assert m[4] == m0 and cnt["ties"] == 1
    # a strictly closer candidate at a lower index keeps the match; a farther one later does not take it
    s = _mini_pair()
    s["kf2"] = _append(s["kf2"], 4, desc=_flip(s["kf2"].desc[4], [0, 9, 100]))
    n, m, cnt = _run(s)
    assert m[4] == 4 and cnt["ties"] == 0
    s["kf2"].desc[4] = _flip(s["kf1"].desc[4], [1, 2, 3, 4, 5])   # now the first is at 5, the copy at 3
    assert _run(s)[1][4] == m0


def test_kat_two_sources_share_one_target():
    s = _mini_pair()
    m0 = s["kf1"].n
    s["kf1"] = _append(s["kf1"], 2, desc=_flip(s["kf1"].desc[2], [7, 8]))
    n, m, cnt = _run(s)
    assert m[2] == 2 and m[m0] == 2 and cnt["shared"] == 1 and n == m0 + 1


def _epipole_pair(offsets_px, octaves):
    """Forward motion; point j projects `offsets_px[j]` px from the epipole in image 2."""
    rng = np.random.default_rng(5)
    q1 = np.array([0, 0, 0, 1], np.float32)
    t1 = np.zeros(3, np.float32)
    c = np.array([0.02, -0.01, 0.5])
    q2 = q1.copy()
    t2 = (-c).astype(np.float32)
    e2 = t2.astype(np.float64)                            # KF1's centre (the world origin) in KF2's frame
    ep = np.array([CAM["fx"] * e2[0] / e2[2] + CAM["cx"], CAM["fy"] * e2[1] / e2[2] + CAM["cy"]])
    pts = []
    for k, off in enumerate(offsets_px):
        a = 0.7 + 1.3 * k
        px, py, d = ep[0] + off * np.cos(a), ep[1] + off * np.sin(a), 4.0
        X2 = np.array([(px - CAM["cx"]) / CAM["fx"] * d, (py - CAM["cy"]) / CAM["fy"] * d, d])
        pts.append(X2 - t2.astype(np.float64))            # R2 = I: Xw = X2 - t2
    s = _pair_from_points(np.array(pts), q1, t1, q2, t2, rng)
    s["kf2"].kps["octave"] = np.array(octaves, np.int32)
    s["ep"] = ep
    return s


def test_kat_twin_near_the_epipole_is_rejected():
    """The exclusion radius is 10 * sqrt(mvScaleFactors[octave2]) px: 10 px at octave 0, 14.4 at 4."""
    s = _epipole_pair([5.0, 9.5, 10.5, 12.0, 12.0, 15.0], [0, 0, 0, 0, 4, 4])
    _, ep = T.geometry(s["kf1"], s["kf2"])
    assert np.abs(ep - s["ep"]).max() < 1e-2
    n, m, cnt = _run(s)
    assert m.tolist() == [-1, -1, 2, 3, -1, 5] and cnt["epipole"] == 3 and cnt["epiline"] == 0


@pytest.mark.parametrize("octave", [0, 2, 5])
def test_kat_epipolar_line_gate(octave):
    """dsqr < 3.84 sigma^2, i.e. closer than 1.96 sigma (sigma = the level's scale factor): a twin
    displaced 2 sigma off its line is rejected, one displaced 0.5 sigma is accepted."""
    s = _mini_pair()
    k1, k2 = s["kf1"], s["kf2"]
    F64, _ = _f64_closed_form(k1, k2)
    k2.kps["octave"] = octave
    sigma = float(SF[octave])
    for j, mult in ((1, 2.0), (2, -2.0), (3, 0.5), (4, -0.5), (5, 1.9), (6, 2.02)):
        a, b, _ = np.array([k1.kps["x"][j], k1.kps["y"][j], 1.0], np.float64) @ F64
        nrm = np.array([a, b]) / np.hypot(a, b)
        k2.kps["x"][j] = np.float32(k2.kps["x"][j] + mult * sigma * nrm[0])
        k2.kps["y"][j] = np.float32(k2.kps["y"][j] + mult * sigma * nrm[1])
    n, m, cnt = _run(s)
    assert [m[j] for j in (1, 2, 6)] == [-1, -1, -1] and [m[j] for j in (3, 4, 5)] == [3, 4, 5]
    assert cnt["epiline"] == 3 and n == k1.n - 3


def test_kat_orientation_filter():
    """roundf(rot * (1 / 30)) bins, bin 30 -> 0, ComputeThreeMaxima keeps at most three bins."""
    assert [T.roundf(v) for v in (0.5, 1.5, 2.5, 0.49, 11.5)] == [1, 2, 3, 0, 12]   # halves away from zero
    s = _mini_pair(m=20)
    a1 = np.zeros(20, np.float32)
    # rot = angle1 - angle2 (+360): 10 features in bin 0, 5 in bin 2 (rot 60), 3 in bin 11 (rot 330), 2 in bin 6
    a2 = np.array([0] * 10 + [300] * 5 + [30] * 3 + [180] * 2, np.float32)
    s["kf1"].kps["angle"], s["kf2"].kps["angle"] = a1, a2
    n, m, cnt = _run(s, 1)
    assert cnt["pruned"] == 2 and m[18] == -1 and m[19] == -1 and n == 18
    assert T.three_maxima([100, 10, 9] + [0] * 27) == (0, 1, -1)
    assert T.three_maxima([101, 10, 10] + [0] * 27) == (0, -1, -1)


# ---- Conditions of the parity scene set (the restatement alone, its own geometry) ----

def test_parity_scene_conditions():
    total = dict(epipole=0, epiline=0, ties=0, shared=0, pruned=0)
    for k in range(len(T.PARITY_SCENES)):
        s = T.parity_scene(k)
        k1 = s["kf1"]
        free = int((k1.has_mp == 0).sum())
        assert k1.n == 300 and len(s["neighbours"]) == 3
        # the forward neighbour's epipole lies inside the image
        _, ep = T.geometry(k1, s["neighbours"][1])
        assert 0 < ep[0] < 640 and 0 < ep[1] < 480
        nm0, m0, c0, _ = T.search_for_triangulation(k1, s["neighbours"], SF, S2, 0)
        nm1, m1, c1, _ = T.search_for_triangulation(k1, s["neighbours"], SF, S2, 1)
        print(f"scene {k}: free {free} matches {nm0.tolist()} / oriented {nm1.tolist()} counters {c1}")
        assert (nm0 >= 0.1 * free).all() and (nm1 >= 0.1 * free).all(), (nm0, nm1, free)
        for key in ("epipole", "epiline", "ties", "shared"):
            assert c0[key] == c1[key]     # the walk does not depend on the orientation switch
            total[key] += c0[key]
        total["pruned"] += c1["pruned"]
        assert c0["pruned"] == 0
        # features outside the FeatureVector are never matched, on either side
        out1 = (k1.weight <= 0) | (k1.node < 0)
        assert out1.any() and (m0[:, out1] == -1).all()
        for b, k2 in enumerate(s["neighbours"]):
            out2 = np.nonzero((k2.weight <= 0) | (k2.node < 0) | (k2.has_mp != 0))[0]
            assert out2.size and not np.isin(m0[b], out2).any()
    assert total["epipole"] >= 5 and total["epiline"] >= 20 and total["ties"] >= 5, total
    assert total["shared"] >= 5 and total["pruned"] >= 5, total
