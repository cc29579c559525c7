"""The fp64 numpy restatement of the bundle adjustment with stereo edges (tests/ba_stereo_numpy.py),
the yardstick of test_ba_stereo_gpu.py, proven on the CPU: on monocular problems it is the oracle
(oracle/ba_oracle.cpp); with EdgeStereoSE3ProjectXYZ edges it has the properties the edge is there
for; and the stereo generator leaves the monocular one's draws alone."""
import numpy as np
import pytest

from orb_slam3_ros2_amd.optimizer import StereoBAProblem
from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem, synthetic_stereo_ba_problem
from tests.ba_stereo_numpy import StereoBA, _qtomat, ba_solve
from tests.helpers import REL, qsign


def _outliers_case():
    # test_lba_with_outliers_and_several_fixed at (12, 300)
    prob, _ = synthetic_ba_problem(n_kf=12, n_pts=300, seed=9)
    prob.pose_fixed[:3] = 1
    prob.edge_uv[::23] += 35.0
    return prob


@pytest.mark.parametrize("case", ["8x100", "20x600", "outliers"])
def test_restatement_is_the_oracle_on_monocular_problems(oracle, case):
    """Both are fp64 with the same order of operations over edges and landmarks; they differ in the
    rounding of the small dense products (numpy's einsum / matmul against the oracle's left-to-right
    sums) and of the LDL^T column updates. Measured on this suite's three cases: the schedules are
    equal, the fp64 initial chi2 is bit-equal, the final chi2 differs by at most 1.3e-15 relative
    (1.9e-15 over the other problems tried), per-edge chi2, poses and points (float32 outputs) by 0.
    Asserted with a margin of 10x: chi2 to 2e-14 relative; the float32 outputs to 10 float32
    roundoffs (2^-24 relative to the array's scale), the least a float32 comparison can resolve
    above the measured 0."""
    prob = {"8x100": lambda: synthetic_ba_problem(n_kf=8, n_pts=100, seed=1)[0],
            "20x600": lambda: synthetic_ba_problem(n_kf=20, n_pts=600, seed=2)[0], "outliers": _outliers_case}[case]()
    r, o = ba_solve(prob), oracle.ba_solve(prob)
    assert (r["iterations_done"], r["lm_trials"]) == (o["iterations_done"], o["lm_trials"])
    di = abs(r["initial_chi2"] - o["initial_chi2"]) / abs(o["initial_chi2"])
    df = abs(r["final_chi2"] - o["final_chi2"]) / abs(o["final_chi2"])
    u32 = 2.0 ** -24
    d = {k: float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max() / max(1.0, np.abs(b).max()))
         for k, a, b in [("pose_q", qsign(r["pose_q"]), qsign(o["pose_q"])), ("pose_t", r["pose_t"], o["pose_t"]),
                         ("points", r["points"], o["points"]), ("edge_chi2", r["edge_chi2"], o["edge_chi2"])]}
    print(f"restatement vs oracle {case}: dinit={di:.2e} dfinal={df:.2e} {d}")
    assert di <= 2e-14 and df <= 2e-14, (di, df)
    assert all(v <= 10 * u32 for v in d.values()), d
    assert np.array_equal(r["edge_depth_ok"], o["edge_depth_ok"])


def _exact_observations(sp, gt):
    """sp with every observation at the ground truth's projection (float32 rounding only)."""
    Xc = np.einsum("eij,ej->ei", gt["R"][sp.edge_pose], gt["points"][sp.edge_point]) + gt["t"][sp.edge_pose]
    fx, fy, cx, cy = (float(np.float32(v)) for v in (sp.fx, sp.fy, sp.cx, sp.cy))
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    sp.edge_uv = np.stack([u, fy * Xc[:, 1] / Xc[:, 2] + cy], 1).astype(np.float32)
    sp.edge_ur = np.where(gt["stereo"], u - sp.bf / Xc[:, 2], -1.0).astype(np.float32)
    return sp


def test_exact_stereo_observations_converge():
    """Noise-free (u, v, ur) and a perturbed state: the solve returns to the ground truth. The final
    chi2 is below 1e-6 of the initial one and every pose within REL of the ground truth."""
    sp, gt = synthetic_stereo_ba_problem(n_kf=8, n_pts=100, seed=5)
    sp = _exact_observations(sp, gt)
    sp.iterations = 30
    r = ba_solve(sp)
    assert r["final_chi2"] < 1e-6 * r["initial_chi2"], (r["initial_chi2"], r["final_chi2"])
    from orb_slam3_ros2_amd.synthetic import _mat_to_quat
    qgt = np.array([_mat_to_quat(R) for R in gt["R"]])
    dq = np.abs(qsign(r["pose_q"]) - qsign(qgt)).max()
    dt = np.abs(r["pose_t"] - gt["t"]).max() / max(1.0, np.abs(gt["t"]).max())
    assert dq < REL and dt < REL, (dq, dt)


def _single_observation_problem(stereo):
    """(8, 100) with exact observations plus landmark 100, seen by keyframe 3 alone through one edge,
    started 0.2 m behind its true position along that keyframe's viewing ray."""
    sp, gt = synthetic_stereo_ba_problem(n_kf=8, n_pts=100, seed=6)
    sp = _exact_observations(sp, gt)
    X = np.array([0.1, -0.05, 0.15])
    R, t = gt["R"][3], gt["t"][3]
    Xc = R @ X + t
    ray = R.T @ (Xc / np.linalg.norm(Xc))
    fx, fy, cx, cy = (float(np.float32(v)) for v in (sp.fx, sp.fy, sp.cx, sp.cy))
    u = fx * Xc[0] / Xc[2] + cx
    sp.points = np.vstack([sp.points, (X + 0.2 * ray)[None]]).astype(np.float32)
    sp.edge_pose = np.append(sp.edge_pose, 3).astype(np.int32)
    sp.edge_point = np.append(sp.edge_point, 100).astype(np.int32)
    sp.edge_uv = np.vstack([sp.edge_uv, [[u, fy * Xc[1] / Xc[2] + cy]]]).astype(np.float32)
    sp.edge_octave = np.append(sp.edge_octave, 0).astype(np.int32)
    sp.edge_ur = np.append(sp.edge_ur, u - sp.bf / Xc[2] if stereo else -1.0).astype(np.float32)
    return sp, X, ray


def test_single_stereo_edge_determines_a_landmark():
    """A landmark seen by one keyframe through one stereo edge has an invertible Hll at lambda = 0
    (three rows) and moves to its true depth; through one monocular edge Hll has rank 2, its null
    space is the viewing ray, and the depth stays where it started. The third row carries the depth:
    no caller can fake it with monocular edges."""
    res = {}
    for stereo in (True, False):
        sp, X, ray = _single_observation_problem(stereo)
        s = StereoBA(sp)
        H = s.landmark_hessians()[100]
        sv = np.linalg.svd(H, compute_uv=False)
        # the viewing ray of the edge at the state Hll was taken at (keyframe 3's perturbed pose)
        Xc = s.camera_points()[-1]
        ray0 = _qtomat(s.q[3]).T @ (Xc / np.linalg.norm(Xc))
        r = ba_solve(sp)
        res[stereo] = (sv, float((r["points"][100] - X) @ ray), H, ray0)
    sv, depth_err, _, _ = res[True]
    assert sv[2] > 1e-6 * sv[0], sv                    # invertible
    assert abs(depth_err) < 0.01, depth_err             # from 0.2 m off to within 1 cm
    sv, depth_err, H, ray0 = res[False]
    assert sv[2] < 1e-12 * sv[0] and sv[1] > 1e-6 * sv[0], sv   # rank 2
    assert np.abs(H @ ray0).max() < 1e-9 * sv[0]
    assert abs(depth_err - 0.2) < 0.02, depth_err       # the depth did not move


def test_stereo_edge_has_its_own_huber_delta():
    """chi2 between 5.991 and 7.815: a stereo edge is not robustified (rho1 == 1, delta^2 = 7.815), the
    same observation as a monocular edge is (delta^2 = 5.991)."""
    sp, gt = synthetic_stereo_ba_problem(n_kf=8, n_pts=100, seed=8)
    sp = _exact_observations(sp, gt)
    # the state at the ground truth, so that each error is what the test puts into the observation
    from orb_slam3_ros2_amd.synthetic import _mat_to_quat
    sp.pose_q = np.array([_mat_to_quat(R) for R in gt["R"]], np.float32)
    sp.pose_t, sp.points = gt["t"].astype(np.float32), gt["points"].astype(np.float32)
    e = int(np.nonzero(gt["stereo"])[0][5])
    info = float(sp.inv_sigma2[sp.edge_octave[e]])
    sp.edge_uv[e, 1] += np.float32(np.sqrt(6.9 / info))
    _, chi2, _, rho1 = StereoBA(sp).errors()
    assert 5.991 < chi2[e] < 7.815, chi2[e]
    assert rho1[e] == 1.0
    mono = StereoBAProblem(**{**sp.__dict__, "edge_ur": np.where(np.arange(sp.edge_ur.shape[0]) == e, -1.0,
                                                                   sp.edge_ur).astype(np.float32)})
    _, chi2m, _, rho1m = StereoBA(mono).errors()
    assert 5.991 < chi2m[e] < 7.815 and rho1m[e] < 1.0, (chi2m[e], rho1m[e])
    assert rho1m[e] == pytest.approx(np.sqrt(np.float32(5.991)) / np.sqrt(chi2m[e]), rel=1e-12)


@pytest.mark.parametrize("seed,nkf,npts", [(7, 50, 2000), (3, 8, 100)])
def test_stereo_generator_leaves_the_monocular_draws(seed, nkf, npts):
    """synthetic_stereo_ba_problem draws from a generator of its own: the monocular problem inside it
    is synthetic_ba_problem's for the same seed, bit for bit, and so is the ground truth."""
    m, gm = synthetic_ba_problem(n_kf=nkf, n_pts=npts, seed=seed)
    s, gs = synthetic_stereo_ba_problem(n_kf=nkf, n_pts=npts, seed=seed)
    for k, v in m.__dict__.items():
        w = getattr(s, k)
        assert np.array_equal(v, w) and np.asarray(v).dtype == np.asarray(w).dtype, k
    for k in ("R", "t", "points"):
        assert np.array_equal(gm[k], gs[k])
    st = s.edge_ur >= 0
    assert 0.6 < st.mean() < 0.8 and np.array_equal(st, gs["stereo"])
    assert s.bf == float(np.float32(np.float32(s.fx) * 0.05))   # a 50 mm baseline
    assert np.array_equal(s.mono().edge_uv, m.edge_uv) and not hasattr(s.mono(), "edge_ur")
