"""Test infrastructure shared by test_ba_stereo.py (CPU) and test_ba_stereo_gpu.py: the comparison
of a BA result with the fp64 restatement (tests/ba_stereo_numpy.py) under the per-edge erase
thresholds (7.815 on stereo edges, 5.991 on monocular ones), and the stereo problems built by hand
on top of synthetic_stereo_ba_problem."""
import numpy as np

from orb_slam3_ros2_amd.optimizer import StereoBAProblem
from orb_slam3_ros2_amd.synthetic import synthetic_stereo_ba_problem
from tests.helpers import REL, qsign


def thresholds(prob) -> np.ndarray:
    ur = getattr(prob, "edge_ur", None)
    if ur is None:
        return np.full(prob.edge_pose.shape[0], 5.991)
    return np.where(np.asarray(ur, np.float32) >= 0, 7.815, 5.991)


def compare_ba_stereo(g, o, prob, exact_schedule=True, point_rel=REL):
    """tests.helpers.compare_ba with the per-edge threshold: the LM schedule (runs that end on the
    iteration budget), chi2, poses and points to REL, and the erase flags, which may differ only
    where the reference's chi2 is within 1e-3 of the edge's threshold."""
    dq = np.abs(qsign(g.pose_q) - qsign(o["pose_q"])).max()
    dt = np.abs(g.pose_t.astype(np.float64) - o["pose_t"]).max() / max(1.0, np.abs(o["pose_t"]).max())
    dp = np.abs(g.points.astype(np.float64) - o["points"]).max() / max(1.0, np.abs(o["points"]).max())
    dchi = abs(g.final_chi2 - o["final_chi2"]) / max(abs(o["final_chi2"]), 1e-300)
    print(f"stereo BA schedule gpu {g.iterations_done}/{g.lm_trials} ref {o['iterations_done']}/{o['lm_trials']} "
          f"dchi2={dchi:.2e} dq={dq:.2e} dt={dt:.2e} dp={dp:.2e}")
    if exact_schedule:
        assert (g.iterations_done, g.lm_trials) == (o["iterations_done"], o["lm_trials"])
    assert abs(g.initial_chi2 - o["initial_chi2"]) <= REL * abs(o["initial_chi2"])
    assert abs(g.final_chi2 - o["final_chi2"]) <= REL * abs(o["final_chi2"])
    assert dq < REL and dt < REL and dp < point_rel, (dq, dt, dp)
    th = thresholds(prob)
    gout = (g.edge_chi2 > th) | (g.edge_depth_ok == 0)
    oout = (o["edge_chi2"] > th) | (o["edge_depth_ok"] == 0)
    diff = np.nonzero(gout != oout)[0]
    assert all(abs(o["edge_chi2"][e] - th[e]) < 1e-3 for e in diff), diff
    assert np.array_equal(np.sort(g.outlier_edges(th)), np.nonzero(gout)[0])


def with_edges(sp, gt, kfs_per_point, stereo_per_point, seed):
    """sp's poses, intrinsics and its first len(kfs_per_point) points under a new edge list:
    point m is seen by the keyframes kfs_per_point[m] (in that order: the order of the landmark's
    edges), stereo where stereo_per_point[m][k]. Observations from the ground truth + 1.2^octave px
    of noise; bf and the deltas are sp's."""
    rng = np.random.Generator(np.random.PCG64(seed))
    M = len(kfs_per_point)
    ep = np.array([k for ks in kfs_per_point for k in ks], np.int32)
    em = np.array([m for m, ks in enumerate(kfs_per_point) for _ in ks], np.int32)
    st = np.array([s for ss in stereo_per_point for s in ss], bool)
    E = ep.shape[0]
    Xc = np.einsum("eij,ej->ei", gt["R"][ep], gt["points"][em]) + gt["t"][ep]
    octave = rng.integers(0, sp.inv_sigma2.shape[0], size=E).astype(np.int32)
    sig = np.power(1.2, octave.astype(np.float64))
    fx, fy, cx, cy = (float(np.float32(v)) for v in (sp.fx, sp.fy, sp.cx, sp.cy))
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    uv = np.stack([u, fy * Xc[:, 1] / Xc[:, 2] + cy], 1) + rng.normal(size=(E, 2)) * sig[:, None]
    ur = u - sp.bf / Xc[:, 2] + rng.normal(size=E) * sig
    assert (ur[st] >= 0).all()
    return StereoBAProblem(**{**sp.__dict__, "points": sp.points[:M].copy(), "edge_pose": ep, "edge_point": em,
                              "edge_uv": uv.astype(np.float32), "edge_octave": octave,
                              "edge_ur": np.where(st, ur, -1.0).astype(np.float32)})


def edge_count_problem(seed=41):
    """10 keyframes, 62 landmarks with 1, 2, 3, 4, 5 and 9 observations (every loop form of the
    landmark kernels: four lanes per landmark, two preloaded edges per lane). Landmark 0 has 9
    observations with its only stereo edge at position 8 (the first edge past the two preloaded
    ones of its lane, taken through edge_error_at in the fused back-substitution); landmark 1 has 9
    with its stereo edges at positions 0 and 1 (preloaded). Keyframe 0 is fixed."""
    sp, gt = synthetic_stereo_ba_problem(n_kf=10, n_pts=62, seed=seed)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    kfs = [sorted(rng.choice(10, 9, replace=False).tolist()) for _ in range(2)]
    ste = [[k == 8 for k in range(9)], [k < 2 for k in range(9)]]
    for m in range(2, 62):
        cnt = (1, 2, 3, 4, 5, 9)[m % 6]
        kfs.append(sorted(rng.choice(10, cnt, replace=False).tolist()))
        ste.append((rng.random(cnt) < 0.7).tolist())
    p = with_edges(sp, gt, kfs, ste, seed + 7)
    counts = np.bincount(p.edge_point)
    assert set(counts.tolist()) == {1, 2, 3, 4, 5, 9}
    return p


def wide_pose_problem(seed=43):
    """4 keyframes, 400 landmarks each seen by all four: 400 edges per pose (more than the 256 of
    lin_pose_wg's work-group and the 64 of lin_pose's wave). Keyframe 0 is fixed and has stereo and
    monocular edges, keyframe 1 has only stereo edges, keyframe 2 only monocular ones, keyframe 3
    both."""
    sp, gt = synthetic_stereo_ba_problem(n_kf=4, n_pts=400, seed=seed)
    assert np.array_equal(np.bincount(sp.edge_pose), [400] * 4) and (gt["ur"] >= 0).all()
    ur = np.where(gt["stereo"], gt["ur"], -1.0)
    ur[sp.edge_pose == 1] = gt["ur"][sp.edge_pose == 1]
    ur[sp.edge_pose == 2] = -1.0
    sp.edge_ur = ur.astype(np.float32)
    k0 = sp.edge_ur[sp.edge_pose == 0]
    assert sp.pose_fixed[0] == 1 and (k0 >= 0).any() and (k0 < 0).any()
    return sp
