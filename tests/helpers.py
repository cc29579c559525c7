"""Shared test helpers: compare product keypoints/descriptors with the oracle's; the numerics of
the dense-solver tests (SPD test matrices, a long-double reference solve, the backward error);
the BA result comparison against the oracle."""
import numpy as np

from orb_slam3_ros2_amd._lib import KP_DTYPE

U = 2.0 ** -53          # fp64 unit roundoff
ETA_CAP = 8.0           # backward error cap of the dense solvers, in units of U
FWD_CAP = 8.0           # forward error cap, in units of cond * U
REL = 1e-4              # north_star: BA state against the oracle
# The condition number the forward bound uses on band_spd's family M M^T + n I: the family's own
# bound (M M^T has its spectrum in [0, 4n]), not each matrix's 2-norm value (1.2 .. 5). A 2-norm
# condition number does not bound a max-norm forward error, and the band matrices show it: in units
# of their own cond_2 u, fp64 LAPACK's Cholesky is at 2.2, its LU at 6.6 and the fp64 model of the
# panel algorithm at 3.8 (n = 600, band), which would leave the cap of 8 two times above the
# references instead of the six to ten times it has on every other case. In units of 5 u the same
# references are at 0.8 / 2.4 / 1.4 (band) and 1.3 / 2.2 / 1.2 (dense).
BAND_COND = 5.0


def spd_with_spectrum(n: int, cond: float, rng) -> np.ndarray:
    """A = Q diag(ev) Q^T, Q from the QR of a normal matrix, ev = geomspace(1, cond, n) * 1e3."""
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.geomspace(1.0, cond, n) * 1e3
    A = (Q * ev) @ Q.T
    return 0.5 * (A + A.T)


def band_spd(n: int, shape: str, rng) -> np.ndarray:
    """M M^T + n I (cond <= 5): M dense ("dense"), lower banded with bandwidth 120 ("band"), or the
    band plus a coupling of the last 120 rows to the first 120 columns ("loop", C5's shape)."""
    if shape == "dense":
        M = rng.normal(size=(n, n))
    else:
        bw = 120
        M = np.zeros((n, n))
        for i in range(n):
            lo = max(0, i - bw)
            M[i, lo:i + 1] = rng.normal(size=i + 1 - lo)
        if shape == "loop":
            M[n - 120:, :120] = rng.normal(size=(120, 120)) * 0.3
    A = M @ M.T + n * np.eye(n)
    return 0.5 * (A + A.T)


def _need_longdouble():
    # not a skip: without an extended type the reference below is no better than the code under test
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble has no 64-bit mantissa on this host"


def solve_longdouble(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """x = A^{-1} b by a column Cholesky and two triangular solves, all in np.longdouble."""
    _need_longdouble()
    n = A.shape[0]
    L = np.tril(A).astype(np.longdouble)
    for j in range(n):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        d = np.sqrt(L[j, j])
        assert d > 0, "reference Cholesky: not positive definite"
        L[j, j] = d
        L[j + 1:, j] /= d
    y = b.astype(np.longdouble)
    for j in range(n):           # column-oriented forward solve
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):   # backward solve with L^T
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def backward_error(A: np.ndarray, x: np.ndarray, b: np.ndarray) -> float:
    """The normwise backward error |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), in long double."""
    _need_longdouble()
    Al, xl, bl = A.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    r = np.abs(bl - Al @ xl).max()
    return float(r / (np.abs(Al).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max()))


def check_solve(A: np.ndarray, x: np.ndarray, b: np.ndarray, cond: float | None = None) -> tuple:
    """The solver yardstick: backward error <= ETA_CAP u and, when cond is given, the forward error
    against solve_longdouble <= FWD_CAP cond u. The caps come from the references, not from the
    kernels: fp64 LAPACK stays below 0.37 u / 0.42 cond u and an fp64 model of the panel algorithm
    (explicit inverses of the diagonal factors) below 0.82 u / 0.46 cond u on these families.
    Returns (eta / u, forward / (cond u) or None) and prints them (pytest -s shows the figures)."""
    eta = backward_error(A, x, b) / U
    fwd = None
    if cond is not None:
        ref = solve_longdouble(A, b)
        fwd = float(np.abs(x.astype(np.longdouble) - ref).max() / np.abs(ref).max()) / (cond * U)
    print(f"SOLVE n={A.shape[0]} cond={cond} eta/u={eta:.3f} fwd/(cond u)={fwd if fwd is None else round(fwd, 3)}")
    assert eta <= ETA_CAP, (eta, fwd)
    assert fwd is None or fwd <= FWD_CAP, (eta, fwd)
    return eta, fwd


def qsign(q):
    q = q.astype(np.float64)
    return q * np.where(q[:, 3:4] < 0, -1.0, 1.0)


def compare_ba(g, o, prob, exact_schedule=True, point_rel=REL):
    """A GPU BAResult against the oracle's dict: the LM schedule, chi2, poses and points."""
    # Run to full convergence, g2o stops on rho == 0 (bit-equal chi2 of two trials): where that
    # happens depends on the last bits of the sums, so the schedule is compared only for runs
    # that stop on the iteration budget (the LocalBundleAdjustment case, optimize(10)).
    dq = np.abs(qsign(g.pose_q) - qsign(o["pose_q"])).max()
    tscale = max(1.0, np.abs(o["pose_t"]).max())
    dt = np.abs(g.pose_t.astype(np.float64) - o["pose_t"]).max() / tscale
    pscale = max(1.0, np.abs(o["points"]).max())
    dp = np.abs(g.points.astype(np.float64) - o["points"]).max() / pscale
    dchi = abs(g.final_chi2 - o["final_chi2"]) / max(abs(o["final_chi2"]), 1e-300)
    print(f"BA schedule gpu {g.iterations_done}/{g.lm_trials} oracle {o['iterations_done']}/{o['lm_trials']} "
          f"dchi2={dchi:.2e} dq={dq:.2e} dt={dt:.2e} dp={dp:.2e}")
    if exact_schedule:
        assert (g.iterations_done, g.lm_trials) == (o["iterations_done"], o["lm_trials"])
    assert abs(g.final_chi2 - o["final_chi2"]) <= REL * abs(o["final_chi2"])
    assert dq < REL and dt < REL and dp < point_rel, (dq, dt, dp)
    gout = (g.edge_chi2 > 5.991) | (g.edge_depth_ok == 0)
    oout = (o["edge_chi2"] > 5.991) | (o["edge_depth_ok"] == 0)
    # flags may only differ for edges whose chi2 sits within rounding of the threshold
    diff = np.nonzero(gout != oout)[0]
    assert all(abs(o["edge_chi2"][e] - 5.991) < 1e-3 for e in diff)


def oracle_kps_to_struct(k6: np.ndarray) -> np.ndarray:
    out = np.zeros(k6.shape[0], KP_DTYPE)
    for i, f in enumerate(["x", "y", "size", "angle", "response"]):
        out[f] = k6[:, i]
    out["octave"] = k6[:, 5].astype(np.int32)
    return out


def diff_report(gk, gd, ok, od, max_lines=10) -> str:
    lines = [f"n gpu={len(gk)} oracle={len(ok)}"]
    n = min(len(gk), len(ok))
    for f in KP_DTYPE.names:
        bad = np.nonzero(gk[f][:n] != ok[f][:n])[0]
        if len(bad):
            lines.append(f"field {f}: {len(bad)} mismatches, first idx {bad[:5].tolist()}")
    if gd is not None and od is not None:
        bad = np.nonzero(np.any(gd[:n] != od[:n], axis=1))[0]
        if len(bad):
            lines.append(f"desc: {len(bad)} rows differ, first {bad[:5].tolist()}")
    for i in range(min(n, max_lines)):
        if any(gk[f][i] != ok[f][i] for f in KP_DTYPE.names):
            lines.append(f"  [{i}] gpu={gk[i]} oracle={ok[i]}")
    return "\n".join(lines)
