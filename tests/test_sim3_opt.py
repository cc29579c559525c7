"""Optimizer::OptimizeSim3 (U:src/Optimizer.cc): the float64 restatement tests/sim3_opt_numpy.py held
to what the function must do. Upstream pins nothing here (no fixtures), so the restatement is pinned
by definitional tests: exact observations converge to the true Sim3 (free and fixed scale), planted
gross mismatches are the cleared matches, the second round runs 5 or 10 iterations, fewer than 10
remaining pairs return 0 with the Sim3 untouched, step 2 reads the chi2 of the last
computeActiveErrors (stale after a rejected final trial), Sim3(u) equals closed forms in its four
branches, and the numeric Jacobian equals the analytic derivative. Last, every problem the GPU file
runs is shown to have results that do not depend on the edge order.

The stale-chi2 scene: a first round can only end in a rejected trial after all ten trials of one
iteration failed, and by then lambda has grown by 2^45, so the rejected state lies within about 1e-6
(relative chi2) of the estimate. Measured on the scene below: the largest |stale - recomputed| is
4.6e-6 at a chi2 of 5470; no edge lies that close to th2 = 10, and th2 cannot be placed between the
two values of an edge without moving the Huber width and with it both values. The masks of the two
rules are therefore equal on every scene found; what the test asserts is that the scene has the
property, that the chi2 step 2 compares are bit for bit the stale ones and not the recomputed ones,
and that the mask is the one the stale values give.
"""
import numpy as np
import pytest

import sim3_opt_cases as C
import sim3_opt_numpy as ref
from orb_slam3_ros2_amd.synthetic import synthetic_sim3_opt_problem


def _qdist(a, b):
    return 1.0 - abs(float(np.dot(a / np.linalg.norm(a), b / np.linalg.norm(b))))


def _exact(prob, gt):
    """Observations recomputed from the float32 points under the true Sim3 (float64), kept in float64."""
    X1, X2 = prob.X1c.astype(np.float64), prob.X2c.astype(np.float64)
    Y = gt["s"] * X2 @ gt["R"].T + gt["t"]
    Z = (X1 - gt["t"]) @ gt["R"] / gt["s"]
    c1, c2 = prob.cam1.astype(np.float64), prob.cam2.astype(np.float64)
    prob.obs1 = np.stack([Y[:, 0] / Y[:, 2] * c1[0] + c1[2], Y[:, 1] / Y[:, 2] * c1[1] + c1[3]], 1).astype(np.float32)
    prob.obs2 = np.stack([Z[:, 0] / Z[:, 2] * c2[0] + c2[2], Z[:, 1] / Z[:, 2] * c2[1] + c2[3]], 1).astype(np.float32)
    return prob


@pytest.mark.parametrize("fix_scale", [False, True])
def test_exact_observations_converge(fix_scale):
    prob, gt = synthetic_sim3_opt_problem(n=120, outlier_frac=0.0, seed=11, fix_scale=fix_scale)
    prob = _exact(prob, gt)
    r = ref.optimize_sim3(prob)
    assert r["n_in"] == 120 and r["n_bad"] == 0 and r["keep"].all()
    # float32 observations: 3e-5 px, over a focal length of 600 px and depths of a few metres
    assert _qdist(r["q"], ref.mat_to_quat(gt["R"])) < 1e-10
    assert np.abs(r["t"] - gt["t"]).max() < 1e-5
    assert abs(r["s"] - gt["s"]) < 1e-5 * gt["s"]
    if fix_scale:
        assert r["s"] == prob.s == 1.0      # bit-identical: sigma is zeroed before every oplus
    else:
        assert r["s"] != prob.s


def test_planted_mismatches_are_the_cleared_ones():
    prob = C.plant_mismatches(C.clean_problem(200, 12), 40)
    r = ref.optimize_sim3(prob)
    assert not r["keep"][:40].any() and r["keep"][40:].all()
    assert r["n_bad"] == 40 and r["n_in"] == 160


def test_generator_marks_its_bad_pairs():
    prob, gt = synthetic_sim3_opt_problem(n=400, outlier_frac=0.2, seed=13, proj_frac=0.25)
    assert gt["by_projection"].sum() > 40 and not (gt["by_projection"] & (prob.obs2[:, 0] > 2.0)).any()
    r = ref.optimize_sim3(prob)
    kept = r["keep"].astype(bool)
    # mismatches and pairs with upstream's normalised obs2 go; of the others only the chi2 tail
    assert not kept[gt["bad"]].any()
    assert kept[~gt["bad"]].mean() > 0.9
    assert r["n_in"] == int(kept.sum())


def test_second_round_runs_five_or_ten_iterations():
    clean = ref.optimize_sim3(C.clean_problem(100, 14, rot_noise=0.02, trans_noise=0.05, scale_noise=0.03))
    assert clean["n_bad"] == 0 and clean["round_iters"][0] == 5 and clean["round_iters"][1] <= 5
    assert sum(clean["round_iters"]) <= clean["lm_trials"] <= 10 * 10      # (5 + 5) iterations of <= 10 trials
    bad = C.reference("left10")
    assert bad["n_bad"] > 0 and 5 < bad["round_iters"][1] <= 10             # more than 5: only nBad > 0 allows it
    assert sum(bad["round_iters"]) <= bad["lm_trials"] <= 15 * 10
    big = C.reference("large1000")
    assert big["n_bad"] > 0 and big["round_iters"] == [5, 10] and 15 <= big["lm_trials"] <= 150


def test_fewer_than_ten_left_returns_zero():
    p9, p10 = C.case("left9"), C.case("left10")
    r9, r10 = C.reference("left9"), C.reference("left10")
    assert p9.X1c.shape[0] - r9["n_bad"] == 9 and p10.X1c.shape[0] - r10["n_bad"] == 10
    assert r9["n_in"] == 0 and len(r9["round_iters"]) == 1
    assert np.array_equal(r9["q"], p9.q) and np.array_equal(r9["t"], p9.t) and r9["s"] == p9.s
    assert r9["keep"].tolist() == [0] * 3 + [1] * 9         # only the clears of step 2
    assert r10["n_in"] == 10 and len(r10["round_iters"]) == 2
    assert not np.array_equal(r10["t"], p10.t)
    # every pair bad, and no pair at all
    rb = C.reference("allbad")
    assert rb["n_in"] == 0 and rb["n_bad"] == 40 and not rb["keep"].any()
    r0 = C.reference("size0")
    assert r0["n_in"] == 0 and r0["lm_trials"] == 0 and r0["s"] == C.case("size0").s


def test_step_two_reads_the_stale_chi2():
    prob, seed = C.stale_problem()
    assert prob is not None, "no seed whose first round ends in a rejected trial"
    r = C.reference("stale")
    assert r["round1_last_rejected"]
    stale, fresh = r["chi2_step2"], r["chi2_step2_fresh"]
    assert not np.array_equal(stale, fresh)
    # (see the module docstring: the two differ by a rejected step under a lambda grown by 2^45)
    assert np.abs(stale - fresh).max() <= 1e-5 * np.maximum(fresh, 1.0).max()
    bad = (stale[:, 0] > prob.th2) | (stale[:, 1] > prob.th2)
    assert r["n_bad"] == int(bad.sum()) and not r["keep"][bad].any()
    rr = ref.optimize_sim3(prob, recompute_step2=True)
    assert np.array_equal(rr["chi2_step2"], stale)         # the option changes what is compared, not what ran


# ---------------------------------------------------------------- Sim3(u)
def _expm(M, terms=40):
    out, term = np.eye(M.shape[0]), np.eye(M.shape[0])
    for k in range(1, terms):
        term = term @ M / k
        out = out + term
    return out


def _closed_form(u):
    """exp of the 4 x 4 generator [[Omega + sigma I, upsilon], [0, 0]] by its power series: s R and t."""
    w, v, sg = u[:3], u[3:6], u[6]
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + sg * np.eye(3)
    G[:3, 3] = v
    E = _expm(G)
    return E[:3, :3], E[:3, 3]


@pytest.mark.parametrize("u, tol", [
    (np.array([3e-6, -2e-6, 1e-6, 0.3, -0.2, 0.1, 4e-6]), 1e-5),      # |sigma| < eps, theta < eps (C = 1 drops sigma / 2)
    (np.array([0.3, -0.2, 0.4, 0.3, -0.2, 0.1, -5e-6]), 1e-5),        # |sigma| < eps, theta >= eps (C = 1, not (s - 1) / sigma)
    (np.array([3e-6, -2e-6, 1e-6, 0.3, -0.2, 0.1, 0.2]), 1e-5),       # |sigma| >= eps, theta < eps (R drops theta^3)
    (np.array([0.3, -0.2, 0.4, 0.3, -0.2, 0.1, 0.2]), 1e-12),         # |sigma| >= eps, theta >= eps
    (np.array([1.2, 0.7, -0.9, -1.0, 0.5, 2.0, -0.4]), 1e-12),
])
def test_sim3_exp_against_the_closed_form(u, tol):
    q, t, s = ref.sim3_exp(u)
    sR, tt = _closed_form(u)
    assert abs(s - np.exp(u[6])) <= 1e-15 * s
    assert np.abs(s * ref.quat_to_mat(q / np.linalg.norm(q)) - sR).max() < max(tol, 1e-12)
    assert np.abs(t - tt).max() < tol
    # Sim3(u) Sim3(-u) = identity
    qi, ti, si = ref.sim3_mul((q, t, s), ref.sim3_exp(-u))
    assert _qdist(qi, np.array([0, 0, 0, 1.0])) < 1e-12 and np.abs(ti).max() < max(tol, 1e-12) and abs(si - 1) < 1e-12
    # inverse() undoes map()
    X = np.array([[0.3, -1.0, 4.0]])
    back = ref.sim3_map(ref.sim3_inv((q, t, s)), ref.sim3_map((q, t, s), X))
    assert np.abs(back - X).max() < 1e-9


def test_small_branch_tolerances_are_the_dropped_terms():
    # theta < eps keeps R = I + Omega + Omega^2: the error is theta^3 / 6 < 2e-16; upstream's B of the
    # third branch lacks a "- 1" and is ~ 1 / sigma^3, times Omega^2 upsilon ~ theta^2 |upsilon|
    u = np.array([3e-6, -2e-6, 1e-6, 0.3, -0.2, 0.1, 0.2])
    _, t, _ = ref.sim3_exp(u)
    _, tt = _closed_form(u)
    theta2 = float(u[:3] @ u[:3])
    assert np.abs(t - tt).max() <= 2.0 * theta2 * np.abs(u[3:6]).max() / abs(u[6]) ** 3


# ---------------------------------------------------------------- the numeric Jacobian
def test_numeric_jacobian_against_the_analytic_derivative():
    prob, _ = synthetic_sim3_opt_problem(n=1, outlier_frac=0.0, seed=15)
    p = ref.normalized(prob)
    S = (p["q"], p["t"], p["s"])
    J12, J21 = ref.numeric_jacobians(S, p, False)
    R = ref.quat_to_mat(p["q"])
    skew = lambda a: np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])  # noqa: E731

    def dproj(cam, Y):
        return np.array([[cam[0] / Y[2], 0, -cam[0] * Y[0] / Y[2] ** 2], [0, cam[1] / Y[2], -cam[1] * Y[1] / Y[2] ** 2]])

    # e12 = obs1 - project(Y), Y = (exp(u) S).map(X2): dY/du = [-[Y]x | I | Y]
    Y = ref.sim3_map(S, p["X2"])[0]
    A12 = -dproj(p["cam1"], Y) @ np.hstack([-skew(Y), np.eye(3), Y[:, None]])
    # e21 = obs2 - project(Z), Z = (exp(u) S)^-1.map(X1) = S^-1.map(exp(-u).map(X1)): dZ/du = R^T / s [[X1]x | -I | -X1]
    X1 = p["X1"][0]
    Z = ref.sim3_map(ref.sim3_inv(S), p["X1"])[0]
    A21 = -dproj(p["cam2"], Z) @ (R.T / p["s"]) @ np.hstack([skew(X1), -np.eye(3), -X1[:, None]])
    # relative to the Jacobian's largest entry: the scale column of e12 is exactly 0 analytically
    # (the whole of Y scales), and the difference quotient's noise (1e-16 x 500 px / 1e-9) is absolute
    assert np.abs(J12[0] - A12).max() <= 1e-5 * np.abs(A12).max()
    assert np.abs(J21[0] - A21).max() <= 1e-5 * np.abs(A21).max()
    assert np.abs(A12[:, 6]).max() < 1e-9 and np.abs(A21[:, 6]).max() > 1.0
    # fixed scale: column 6 is exactly 0
    F12, F21 = ref.numeric_jacobians(S, p, True)
    assert not F12[:, :, 6].any() and not F21[:, :, 6].any()
    assert np.array_equal(F12[:, :, :6], J12[:, :, :6])


def test_fixed_scale_solve_needs_no_special_case():
    # H66 = lambda, b6 = 0: the LDL^T goes through and x6 = 0
    rng = np.random.default_rng(3)
    A = rng.normal(size=(6, 6))
    H = np.zeros((7, 7))
    H[:6, :6] = A @ A.T + np.eye(6)
    b = np.append(rng.normal(size=6), 0.0)
    x = ref.ldlt_solve(H + 1e-3 * np.eye(7), b)
    assert x is not None and x[6] == 0.0
    assert np.abs((H + 1e-3 * np.eye(7)) @ x - b).max() < 1e-12


# ---------------------------------------------------------------- the GPU file's scenes
def test_points_behind_the_camera_are_defined():
    r = C.reference("behind")
    assert np.isfinite(r["t"]).all() and np.isfinite(r["s"])
    assert not r["keep"][:5].any()          # a finite, far-off projection: cleared in step 2
    assert r["n_in"] > 50


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_cases_are_order_stable(name):
    """The device sums the edges in another order than the restatement, so comparing keep, n_in and
    n_bad by equality is only honest for problems whose restatement does not depend on the edge
    order (a seed that fails is replaced in sim3_opt_cases.SEED; nothing is loosened or left out)."""
    prob, r = C.case(name), C.reference(name)
    for seed in (1, 2):
        q, perm = C.permuted(prob, seed)
        rp = ref.optimize_sim3(q)
        keep = np.empty_like(rp["keep"])
        keep[perm] = rp["keep"]
        assert np.array_equal(keep, r["keep"]) and rp["n_in"] == r["n_in"] and rp["n_bad"] == r["n_bad"]
        assert _qdist(rp["q"], r["q"]) < 1e-12 and np.abs(rp["t"] - r["t"]).max() < 1e-6   # the order moves the pose far less than the device tolerance
