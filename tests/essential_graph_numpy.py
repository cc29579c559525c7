"""Optimizer::OptimizeEssentialGraph (U:src/Optimizer.cc) restated literally in float64 numpy.

The graph is what the adapter builds from the Map: arrays only. The formulas, each with the
upstream file that holds it (Sim3 product, inverse, exponential and oplus are sim3_opt_numpy's):

  VertexSim3Expmap: estimate (q xyzw, t, s) as g2o::Sim3, never renormalised; a fixed flag per
      vertex; one fix_scale for the graph; oplusImpl(u): u[6] = 0 when fix_scale, estimate =
      Sim3(u) * estimate                               U:Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h
  EdgeSim3(i, j, Sji), vertex(0) = i, vertex(1) = j, information I7, no robust kernel:
      e = (Sji * Si * Sj^-1).log(), chi2 = e.e          U:Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h
  Sim3::log()                                           U:Thirdparty/g2o/g2o/types/sim3.h
      sigma = log(s), R = r.toRotationMatrix(), d = 0.5 (tr R - 1), eps = 1e-5,
      dR = (R32 - R23, R13 - R31, R21 - R12)
      |sigma| <  eps, d >  1 - eps: omega = 0.5 dR, A = 1/2, B = 1/6, C = 1
      |sigma| <  eps, else:         theta = acos(d), omega = theta / (2 sqrt(1 - d^2)) dR,
                                    A = (1 - cos theta) / theta^2, B = (theta - sin theta) / theta^3, C = 1
      |sigma| >= eps, d >  1 - eps: C = (s - 1) / sigma, omega = 0.5 dR,
                                    A = ((sigma - 1) s + 1) / sigma^2,
                                    B = ((0.5 sigma^2 - sigma + 1) s) / sigma^3
      |sigma| >= eps, else:         C as above, theta and omega as in the second branch,
                                    a = s sin theta, b = s cos theta, c = theta^2 + sigma^2,
                                    A = (a sigma + (1 - b) theta) / (theta c),
                                    B = (C - ((b - 1) sigma + a theta) / c) / theta^2
      W = A Omega + B Omega^2 + C I, Omega = skew(omega); upsilon = W.lu().solve(t) (3x3, partial
      pivoting); log = (omega, upsilon, sigma)
  Jacobians: numeric, BaseBinaryEdge::linearizeOplus; a fixed vertex gets none. Per free vertex and
      component d: oplus(+1e-9 e_d), computeError, pop, oplus(-1e-9 e_d), computeError, pop,
      column = (e+ - e-) / 2e-9                         U:Thirdparty/g2o/g2o/core/base_binary_edge.hpp
  H_ii += Ji^T Ji, H_jj += Jj^T Jj, H_ij += Ji^T Jj, b_i += -Ji^T e, b_j += -Jj^T e: several edges
      between one pair sum (upstream's sInsertedEdges only dedups covisibility edges).
  BlockSolver_7_3 + LinearSolverEigen + Levenberg with setUserLambdaInit(1e-16): lambda0 is the
      user value, not 1e-5 max diag. rho, accept / reject, the lambda update, the 10-trial cap and
      the stop on rho == 0 are sim3_opt_numpy._optimize's. No marginalised vertex: one solve of
      (H + lambda I) x = b over the free vertices per trial (a dense LDL^T without pivoting here).
      initializeOptimization(); computeActiveErrors(); optimize(iterations), upstream 20.
  Map points (the loop that follows optimize upstream): P' = Swc_corrected[ref].map(Scw_before[ref]
      .map(P)), Scw_before the vertex's input estimate, Swc_corrected the inverse of its optimised
      one; P float32 in and out, the arithmetic in double in the order written below.

Edges are evaluated in arrays: the batched product, inverse and log below repeat the scalar
operation order (every product and sum its own rounding), which the device kernels repeat too; only
the sums over edges differ in order.
"""
import numpy as np

from sim3_opt_numpy import oplus, qmul, sim3_exp, sim3_inv, sim3_mul  # noqa: F401

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)
EPS = 0.00001


# ---------------------------------------------------------------- batched Sim3 arithmetic: (n, 8) rows
def _qrot(q, v):
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    vx, vy, vz = v[:, 0], v[:, 1], v[:, 2]
    ux = y * vz - z * vy
    uy = z * vx - x * vz
    uz = x * vy - y * vx
    ux = ux + ux
    uy = uy + uy
    uz = uz + uz
    cx = y * uz - z * uy
    cy = z * ux - x * uz
    cz = x * uy - y * ux
    return np.stack([vx + w * ux + cx, vy + w * uy + cy, vz + w * uz + cz], 1)


def bmul(a, b):
    """Row-wise g2o::Sim3 product of (n, 8) arrays (either may be a single row)."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    n = max(a.shape[0], b.shape[0])
    a, b = np.broadcast_to(a, (n, 8)), np.broadcast_to(b, (n, 8))
    ax, ay, az, aw = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    bx, by, bz, bw = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    out = np.empty((n, 8))
    out[:, 0] = aw * bx + ax * bw + ay * bz - az * by
    out[:, 1] = aw * by + ay * bw + az * bx - ax * bz
    out[:, 2] = aw * bz + az * bw + ax * by - ay * bx
    out[:, 3] = aw * bw - ax * bx - ay * by - az * bz
    out[:, 4:7] = a[:, 7:8] * _qrot(a[:, 0:4], b[:, 4:7]) + a[:, 4:7]
    out[:, 7] = a[:, 7] * b[:, 7]
    return out


def binv(a):
    a = np.atleast_2d(a)
    out = np.empty_like(a)
    out[:, 0:3] = -a[:, 0:3]
    out[:, 3] = a[:, 3]
    k = -1.0 / a[:, 7]
    out[:, 4:7] = _qrot(out[:, 0:4], k[:, None] * a[:, 4:7])
    out[:, 7] = 1.0 / a[:, 7]
    return out


def bmap(a, X):
    """s (r X) + t row-wise."""
    a = np.atleast_2d(a)
    return a[:, 7:8] * _qrot(a[:, 0:4], X) + a[:, 4:7]


def _rot(q):
    """Eigen's Quaternion::toRotationMatrix, (n, 3, 3)."""
    x, y, z, w = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.empty((q.shape[0], 3, 3))
    R[:, 0, 0] = 1 - (tyy + tzz); R[:, 0, 1] = txy - twz; R[:, 0, 2] = txz + twy
    R[:, 1, 0] = txy + twz; R[:, 1, 1] = 1 - (txx + tzz); R[:, 1, 2] = tyz - twx
    R[:, 2, 0] = txz - twy; R[:, 2, 1] = tyz + twx; R[:, 2, 2] = 1 - (txx + tyy)
    return R


def _lu3_solve(W, t):
    """3x3 partial-pivot LU solve per row of W (n, 3, 3), t (n, 3): the first largest pivot wins."""
    A = W.copy()
    b = t.copy()
    n = A.shape[0]
    rows = np.arange(n)
    with np.errstate(all="ignore"):
        for k in range(2):
            p = k + np.argmax(np.abs(A[:, k:, k]), axis=1)
            Ak, Ap = A[rows, k].copy(), A[rows, p].copy()
            A[rows, k], A[rows, p] = Ap, Ak
            bk, bp = b[rows, k].copy(), b[rows, p].copy()
            b[rows, k], b[rows, p] = bp, bk
            for i in range(k + 1, 3):
                f = A[:, i, k] / A[:, k, k]
                for c in range(k + 1, 3):
                    A[:, i, c] = A[:, i, c] - f * A[:, k, c]
                b[:, i] = b[:, i] - f * b[:, k]
        x2 = b[:, 2] / A[:, 2, 2]
        x1 = (b[:, 1] - A[:, 1, 2] * x2) / A[:, 1, 1]
        x0 = (b[:, 0] - A[:, 0, 1] * x1 - A[:, 0, 2] * x2) / A[:, 0, 0]
    return np.stack([x0, x1, x2], 1)


def sim3_log(a, return_branch=False):
    """g2o::Sim3::log of (n, 8) rows: (n, 7) = (omega, upsilon, sigma). branch: 0..3 in the order of
    the docstring."""
    a = np.atleast_2d(np.asarray(a, np.float64))
    with np.errstate(all="ignore"):
        s = a[:, 7]
        sigma = np.log(s)
        R = _rot(a[:, 0:4])
        d = 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1)
        dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
        small_s = np.abs(sigma) < EPS
        small_r = d > 1 - EPS
        theta = np.arccos(d)
        st, ct = np.sin(theta), np.cos(theta)
        theta2 = theta * theta
        sigma2 = sigma * sigma
        k_big = theta / (2 * np.sqrt(1 - d * d))
        omega = np.where(small_r[:, None], 0.5 * dR, k_big[:, None] * dR)
        C = np.where(small_s, 1.0, (s - 1) / sigma)
        a_, b_ = s * st, s * ct
        c_ = theta2 + sigma2
        A = np.where(small_s,
                     np.where(small_r, 0.5, (1 - ct) / theta2),
                     np.where(small_r, ((sigma - 1) * s + 1) / sigma2, (a_ * sigma + (1 - b_) * theta) / (theta * c_)))
        B = np.where(small_s,
                     np.where(small_r, 1.0 / 6.0, (theta - st) / (theta2 * theta)),
                     np.where(small_r, ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma),
                              (C - ((b_ - 1) * sigma + a_ * theta) / c_) / theta2))
        n = a.shape[0]
        O = np.zeros((n, 3, 3))
        O[:, 0, 1] = -omega[:, 2]; O[:, 0, 2] = omega[:, 1]
        O[:, 1, 0] = omega[:, 2]; O[:, 1, 2] = -omega[:, 0]
        O[:, 2, 0] = -omega[:, 1]; O[:, 2, 1] = omega[:, 0]
        O2 = np.empty((n, 3, 3))
        for r in range(3):
            for c in range(3):
                O2[:, r, c] = O[:, r, 0] * O[:, 0, c] + O[:, r, 1] * O[:, 1, c] + O[:, r, 2] * O[:, 2, c]
        W = (A[:, None, None] * O + B[:, None, None] * O2) + C[:, None, None] * np.eye(3)
        ups = _lu3_solve(W, a[:, 4:7])
    out = np.concatenate([omega, ups, sigma[:, None]], 1)
    if return_branch:
        return out, 2 * (~small_s).astype(int) + (~small_r).astype(int)
    return out


def row(S):
    """A (q, t, s) tuple of sim3_opt_numpy as an 8-row."""
    return np.concatenate([S[0], S[1], [S[2]]])


def tup(r):
    return r[0:4].copy(), r[4:7].copy(), float(r[7])


# ---------------------------------------------------------------- edges
def edge_errors(S, ij, Sji, return_branch=False):
    """(E, 7) errors at the estimates S (n, 8)."""
    return sim3_log(bmul(bmul(Sji, S[ij[:, 0]]), binv(S[ij[:, 1]])), return_branch)


def perturbations(fix_scale):
    """The 14 Sim3(+-1e-9 e_d) of linearizeOplus, row 2 d + (0: +, 1: -)."""
    P = np.empty((14, 8))
    for d in range(7):
        for k, dl in enumerate((DELTA, -DELTA)):
            u = np.zeros(7)
            u[d] = dl
            if fix_scale:
                u[6] = 0.0
            P[2 * d + k] = row(sim3_exp(u))
    return P


def numeric_jacobians(S, fixed, ij, Sji, fix_scale):
    """Ji, Jj: (E, 7, 7) [edge, error row, component]; zero for a fixed vertex."""
    E = ij.shape[0]
    P = perturbations(fix_scale)
    Si, Sj = S[ij[:, 0]], S[ij[:, 1]]
    Sjinv = binv(Sj)
    J = [np.zeros((E, 7, 7)), np.zeros((E, 7, 7))]
    for d in range(7):
        ep = sim3_log(bmul(bmul(Sji, bmul(P[2 * d], Si)), Sjinv))
        em = sim3_log(bmul(bmul(Sji, bmul(P[2 * d + 1], Si)), Sjinv))
        J[0][:, :, d] = SCALAR * (ep - em)
        ep = sim3_log(bmul(bmul(Sji, Si), binv(bmul(P[2 * d], Sj))))
        em = sim3_log(bmul(bmul(Sji, Si), binv(bmul(P[2 * d + 1], Sj))))
        J[1][:, :, d] = SCALAR * (ep - em)
    J[0][fixed[ij[:, 0]] != 0] = 0.0
    J[1][fixed[ij[:, 1]] != 0] = 0.0
    return J[0], J[1]


def free_index(fixed):
    """vertex -> row block of H (-1: fixed), and the number of free vertices."""
    idx = np.full(fixed.shape[0], -1, np.int64)
    free = np.nonzero(fixed == 0)[0]
    idx[free] = np.arange(free.size)
    return idx, int(free.size)


def assemble(Ji, Jj, e, ij, fixed):
    idx, nf = free_index(fixed)
    H = np.zeros((7 * nf, 7 * nf))
    b = np.zeros(7 * nf)
    for k in range(ij.shape[0]):
        i, j = idx[ij[k, 0]], idx[ij[k, 1]]
        if i >= 0:
            H[7 * i:7 * i + 7, 7 * i:7 * i + 7] += Ji[k].T @ Ji[k]
            b[7 * i:7 * i + 7] += -(Ji[k].T @ e[k])
        if j >= 0:
            H[7 * j:7 * j + 7, 7 * j:7 * j + 7] += Jj[k].T @ Jj[k]
            b[7 * j:7 * j + 7] += -(Jj[k].T @ e[k])
        if i >= 0 and j >= 0:
            M = Ji[k].T @ Jj[k]
            H[7 * i:7 * i + 7, 7 * j:7 * j + 7] += M
            H[7 * j:7 * j + 7, 7 * i:7 * i + 7] += M.T
    return H, b


def ldlt_solve(S, b):
    """Dense LDL^T without pivoting (sim3_opt_numpy.ldlt_solve with the inner loops as array
    operations); None where a pivot is zero or not finite."""
    m = S.shape[0]
    L = S.copy()
    d = np.zeros(m)
    with np.errstate(all="ignore"):
        for j in range(m):
            ld = L[j, :j] * d[:j]
            dj = L[j, j] - np.dot(L[j, :j], ld)
            if dj == 0.0 or not np.isfinite(dj):
                return None
            d[j] = dj
            if j + 1 < m:
                L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ ld) * (1.0 / dj)
        x = b.copy()
        for i in range(m):
            x[i] -= np.dot(L[i, :i], x[:i])
        x *= 1.0 / d
        for i in range(m - 1, -1, -1):
            x[i] -= np.dot(L[i + 1:, i], x[i + 1:])
    return x


def np_solve(S, b):
    try:
        x = np.linalg.solve(S, b)
    except np.linalg.LinAlgError:
        return None
    return x if np.all(np.isfinite(x)) else None


# ---------------------------------------------------------------- the procedure
def correct_points(S_in, S_out, points, ref):
    """P' = Swc_corrected[ref].map(Scw_before[ref].map(P)), float32 in and out."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    if P.shape[0] == 0:
        return np.zeros((0, 3), np.float32)
    ref = np.asarray(ref, np.int64)
    Pc = bmap(np.asarray(S_in, np.float64)[ref], P)
    return bmap(binv(np.asarray(S_out, np.float64)[ref]), Pc).astype(np.float32)


def optimize_essential_graph(S, fixed, edge_ij, edge_S, fix_scale=False, iterations=20, lambda_init=1e-16,
                             points=None, point_ref=None, solve=ldlt_solve, edge_order=None):
    """Returns dict(S, points, chi2_initial, chi2_final, iterations_run, lm_trials, lm_rejected,
    accepts (the accept / reject sequence), margins (per trial |chi2 - chi2'| / chi2: how far the
    decision is from a tie), branches (sim3_log's branch per edge at the first
    linearisation), H0, b0 (the first system))."""
    S0 = np.ascontiguousarray(S, np.float64).reshape(-1, 8)
    fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1)
    ij = np.ascontiguousarray(edge_ij, np.int64).reshape(-1, 2)
    Sji = np.ascontiguousarray(edge_S, np.float64).reshape(-1, 8)
    if edge_order is not None:
        ij, Sji = ij[edge_order], Sji[edge_order]
    S = S0.copy()
    idx, nf = free_index(fixed)
    free = np.nonzero(fixed == 0)[0]
    E = ij.shape[0]
    out = dict(iterations_run=0, lm_trials=0, lm_rejected=0, accepts=[], margins=[], branches=np.zeros(0, int), H0=None,
               b0=None)

    def chi_of(Sx):
        if E == 0:
            return 0.0
        e = edge_errors(Sx, ij, Sji)
        return float(np.sum(np.sum(e * e, 1)))

    current = chi_of(S)
    out["chi2_initial"] = current
    lam, ni = 0.0, 2.0
    if E > 0 and nf > 0:
        for it in range(iterations):
            out["iterations_run"] += 1
            e, br = edge_errors(S, ij, Sji, True)
            current = float(np.sum(np.sum(e * e, 1)))
            Ji, Jj = numeric_jacobians(S, fixed, ij, Sji, fix_scale)
            H, b = assemble(Ji, Jj, e, ij, fixed)
            if it == 0:
                lam, ni = float(lambda_init), 2.0
                out["branches"], out["H0"], out["b0"] = br, H.copy(), b.copy()
            rho, qmax = 0.0, 0
            while True:
                x = solve(H + lam * np.eye(7 * nf), b)
                ok = x is not None
                if not ok:
                    x = np.zeros(7 * nf)
                Sn = S.copy()
                for k, v in enumerate(free):
                    Sn[v] = row(oplus(tup(S[v]), x[7 * k:7 * k + 7], fix_scale))
                with np.errstate(all="ignore"):
                    temp = chi_of(Sn)
                    if not ok:
                        temp = np.finfo(np.float64).max
                    scale = 1e-3 + float(np.sum(x * (lam * x + b)))
                    rho = (current - temp) / scale
                accepted = bool(rho > 0 and np.isfinite(temp))
                current_before = current
                if accepted:
                    t2 = 2 * rho - 1
                    alpha = min(1.0 - t2 * t2 * t2, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    current = temp
                    S = Sn
                else:
                    lam *= ni
                    ni *= 2
                    out["lm_rejected"] += 1
                qmax += 1
                out["lm_trials"] += 1
                out["accepts"].append(accepted)
                out["margins"].append(abs(current_before - temp) / max(current_before, 1e-300))
                if not (rho < 0 and qmax < 10):
                    break
            if qmax == 10 or rho == 0:
                break
    out["S"] = S
    out["chi2_final"] = current
    out["points"] = (correct_points(S0, S, points, point_ref) if points is not None and len(points)
                     else np.zeros((0, 3), np.float32))
    return out


def sim3_distance(Sa, Sb):
    """The project's Optimizer metric per vertex, each part scaled so that `< tol` is the bound:
    sqrt(1 - |q.q'|) (unit quaternions taken from the rows), |dt|inf / max(1, |t|inf), |ds| / s."""
    Sa, Sb = np.atleast_2d(Sa), np.atleast_2d(Sb)
    qa = Sa[:, 0:4] / np.linalg.norm(Sa[:, 0:4], axis=1, keepdims=True)
    qb = Sb[:, 0:4] / np.linalg.norm(Sb[:, 0:4], axis=1, keepdims=True)
    dq = np.sqrt(np.maximum(0.0, 1 - np.abs(np.sum(qa * qb, 1))))
    dt = np.max(np.abs(Sa[:, 4:7] - Sb[:, 4:7]), 1) / np.maximum(1.0, np.max(np.abs(Sb[:, 4:7]), 1))
    ds = np.abs(Sa[:, 7] - Sb[:, 7]) / np.abs(Sb[:, 7])
    return float(max(dq.max(), dt.max(), ds.max())) if Sa.shape[0] else 0.0
