"""Optimizer::OptimizeSim3 (U:src/Optimizer.cc) restated literally in float64 numpy.

The formulas, each with the upstream file that holds it:

  estimate S12 = (q, t, s): g2o::Sim3 holds a Quaterniond r, a Vector3d t and a double s
      map(X) = s (r X) + t                                     U:Thirdparty/g2o/g2o/types/sim3.h
      a * b  = (a.r b.r, a.s (a.r b.t) + a.t, a.s b.s)         U:Thirdparty/g2o/g2o/types/sim3.h
      inverse = (r*, r* ((-1 / s) t), 1 / s)                   U:Thirdparty/g2o/g2o/types/sim3.h
      neither the product nor the constructors normalise r; r X is Eigen's
      v + w (2 r_v x v) + r_v x (2 r_v x v)
  Sim3(u), u = (omega, upsilon, sigma)                         U:Thirdparty/g2o/g2o/types/sim3.h
      theta = |omega|, Omega = skew(omega), s = exp(sigma), eps = 1e-5
      |sigma| <  eps, theta <  eps: C = 1, A = 1/2, B = 1/6, R = I + Omega + Omega^2
      |sigma| <  eps, theta >= eps: C = 1, A = (1 - cos) / theta^2, B = (theta - sin) / theta^3,
                                    R = I + sin / theta Omega + (1 - cos) / theta^2 Omega^2
      |sigma| >= eps, theta <  eps: C = (s - 1) / sigma, A = ((sigma - 1) s + 1) / sigma^2,
                                    B = ((sigma^2 / 2 - sigma + 1) s) / sigma^3 (upstream writes it
                                    without the "- 1" the series has; it multiplies Omega^2 upsilon,
                                    below 1e-10 |upsilon|), R = I + Omega + Omega^2
      |sigma| >= eps, theta >= eps: a = s sin, b = s cos, c = theta^2 + sigma^2,
                                    A = (a sigma + (1 - b) theta) / (theta c),
                                    B = (C - ((b - 1) sigma + a theta) / c) / theta^2, R = Rodrigues
      r = Quaterniond(R), t = (A Omega + B Omega^2 + C I) upsilon
  VertexSim3Expmap::oplusImpl(u): u[6] = 0 when _fix_scale; estimate = Sim3(u) * estimate
                                                               U:Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h
  EdgeSim3ProjectXYZ:        e12 = obs1 - cam1.project(S12.map(P3D2c))
  EdgeInverseSim3ProjectXYZ: e21 = obs2 - cam2.project(S12.inverse().map(P3D1c))
      project(X) = (x / z fx + cx, y / z fy + cy); information I2 invSigma2; chi2 = info |e|^2
                                                               U:Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h
  Jacobians: numeric, BaseBinaryEdge::linearizeOplus with the point vertex fixed: per component d,
      oplus(+1e-9 e_d), computeError, pop, oplus(-1e-9 e_d), computeError, pop,
      column = (1 / 2e-9) (e+ - e-)                            U:Thirdparty/g2o/g2o/core/base_binary_edge.hpp
  Huber delta = (float)sqrt(th2): rho = (chi2, 1) below delta^2, else (2 sqrt(chi2) delta - delta^2,
      delta / sqrt(chi2)); H += J^T (rho1 info) J, b += J^T (-(info e) rho1)
                                                               U:Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp
  Levenberg: lambda0 = 1e-5 max diag H, rho = (chi - chi') / (x.(lambda x + b) + 1e-3), accept iff
      rho > 0 and chi' finite: lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), ni = 2; else
      lambda *= ni, ni *= 2; at most 10 trials per iteration; stop when all ten fail or rho == 0
                                                               U:Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp
  The 7x7 system (H + lambda I) x = b is solved by a dense LDL^T without pivoting, as the
  project's other optimizers restate g2o's dense solver.

The procedure (U:src/Optimizer.cc::OptimizeSim3): optimize(5) with Huber; every pair with
e12.chi2() > th2 or e21.chi2() > th2 is removed (the chi2 of the last computeActiveErrors that saw
the edge: stale after a rejected final trial) and counted in nBad, the others lose their kernel;
nCorrespondences - nBad < 10 returns 0 with g2oS12 untouched; optimize(nBad > 0 ? 10 : 5) from a
fresh lambda0; computeError on the remaining pairs, either chi2 > th2 clears the match, the others
count in nIn; g2oS12 = estimate.

The per-edge arithmetic is written in one fixed operation order (every product and sum its own
rounding), which the device kernel repeats; only the sums over the edges differ in order.
"""
import numpy as np

DELTA = 1e-9
SCALAR = 1.0 / (2 * DELTA)


# ---------------------------------------------------------------- quaternion / Sim3 arithmetic
def qrot(q, v):
    """Eigen's Quaternion * Vector3 for q = (x, y, z, w); v is (..., 3)."""
    x, y, z, w = q
    vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
    ux = y * vz - z * vy
    uy = z * vx - x * vz
    uz = x * vy - y * vx
    ux = ux + ux
    uy = uy + uy
    uz = uz + uz
    cx = y * uz - z * uy
    cy = z * ux - x * uz
    cz = x * uy - y * ux
    return np.stack([vx + w * ux + cx, vy + w * uy + cy, vz + w * uz + cz], -1)


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def mat_to_quat(m):
    """Eigen's Quaterniond(Matrix3d), (x, y, z, w)."""
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        s = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (m[k, j] - m[j, k]) * s
        q[j] = (m[j, i] + m[i, j]) * s
        q[k] = (m[k, i] + m[i, k]) * s
    return q


def quat_to_mat(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def sim3_exp(u):
    """g2o::Sim3(const Vector7d&): (q, t, s)."""
    ox, oy, oz = float(u[0]), float(u[1]), float(u[2])
    sigma = float(u[6])
    theta = float(np.sqrt(ox * ox + oy * oy + oz * oz))
    O = np.array([[0.0, -oz, oy], [oz, 0.0, -ox], [-oy, ox, 0.0]])
    O2 = np.empty((3, 3))
    for r in range(3):
        for c in range(3):
            O2[r, c] = O[r, 0] * O[0, c] + O[r, 1] * O[1, c] + O[r, 2] * O[2, c]
    s = float(np.exp(sigma))
    eye = np.eye(3)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B = 1.0 / 2.0, 1.0 / 6.0
            R = (eye + O) + O2
        else:
            theta2 = theta * theta
            st, ct = float(np.sin(theta)), float(np.cos(theta))
            A = (1 - ct) / theta2
            B = (theta - st) / (theta2 * theta)
            R = (eye + (st / theta) * O) + ((1 - ct) / (theta * theta)) * O2
    else:
        C = (s - 1) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1) * s + 1) / sigma2
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
            R = (eye + O) + O2
        else:
            st, ct = float(np.sin(theta)), float(np.cos(theta))
            R = (eye + (st / theta) * O) + ((1 - ct) / (theta * theta)) * O2
            a = s * st
            b = s * ct
            theta2 = theta * theta
            sigma2 = sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1 - b) * theta) / (theta * c)
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1.0 / theta2
    q = mat_to_quat(R)
    W = (A * O + B * O2) + C * eye
    t = np.array([W[r, 0] * u[3] + W[r, 1] * u[4] + W[r, 2] * u[5] for r in range(3)])
    return q, t, s


def sim3_mul(a, b):
    qa, ta, sa = a
    qb, tb, sb = b
    return qmul(qa, qb), sa * qrot(qa, tb) + ta, sa * sb


def sim3_inv(a):
    q, t, s = a
    qc = np.array([-q[0], -q[1], -q[2], q[3]])
    return qc, qrot(qc, (-1.0 / s) * t), 1.0 / s


def sim3_map(a, X):
    q, t, s = a
    return s * qrot(q, X) + t


def oplus(S, u, fix_scale):
    u = np.array(u, np.float64)
    if fix_scale:
        u[6] = 0.0
    return sim3_mul(sim3_exp(u), S)


# ---------------------------------------------------------------- edges
def _project(cam, P):
    with np.errstate(all="ignore"):
        return np.stack([P[:, 0] / P[:, 2] * cam[0] + cam[2], P[:, 1] / P[:, 2] * cam[1] + cam[3]], 1)


def edge_errors(S, p):
    """(e12, e21): n x 2 each, at the estimate S."""
    e12 = p["obs1"] - _project(p["cam1"], sim3_map(S, p["X2"]))
    e21 = p["obs2"] - _project(p["cam2"], sim3_map(sim3_inv(S), p["X1"]))
    return e12, e21


def _chi2(e, info):
    with np.errstate(all="ignore"):
        return info * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])


def numeric_jacobians(S, p, fix_scale):
    """J12, J21: n x 2 x 7, g2o's central differences."""
    n = p["X1"].shape[0]
    J12, J21 = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
    for d in range(7):
        u = np.zeros(7)
        u[d] = DELTA
        ep12, ep21 = edge_errors(oplus(S, u, fix_scale), p)
        u[d] = -DELTA
        em12, em21 = edge_errors(oplus(S, u, fix_scale), p)
        with np.errstate(all="ignore"):
            J12[:, :, d] = SCALAR * (ep12 - em12)
            J21[:, :, d] = SCALAR * (ep21 - em21)
    return J12, J21


def _huber(chi2, delta, robust):
    rho0, rho1 = chi2.copy(), np.ones_like(chi2)
    if robust:
        dsqr = delta * delta
        with np.errstate(all="ignore"):
            big = chi2 > dsqr
            sq = np.sqrt(chi2)
            rho0 = np.where(big, 2 * sq * delta - dsqr, rho0)
            rho1 = np.where(big, delta / sq, rho1)
    return rho0, rho1


def ldlt_solve(S, b):
    """Dense LDL^T without pivoting; None where a pivot is zero or not finite."""
    m = S.shape[0]
    L = S.copy()
    d = np.zeros(m)
    for j in range(m):
        dj = L[j, j]
        for k in range(j):
            dj -= L[j, k] * L[j, k] * d[k]
        if dj == 0.0 or not np.isfinite(dj):
            return None
        d[j] = dj
        idj = 1.0 / dj
        for i in range(j + 1, m):
            s = L[i, j]
            for k in range(j):
                s -= L[i, k] * L[j, k] * d[k]
            L[i, j] = s * idj
    x = b.copy()
    for i in range(m):
        for k in range(i):
            x[i] -= L[i, k] * x[k]
    for i in range(m):
        x[i] *= 1.0 / d[i]
    for i in range(m - 1, -1, -1):
        for k in range(i + 1, m):
            x[i] -= L[k, i] * x[k]
    return x


# ---------------------------------------------------------------- g2o optimize(iterations)
def _optimize(S, p, active, robust, iterations, fix_scale, chi2_last, stats):
    """Levenberg over the active pairs. chi2_last (n x 2) is updated in place with the chi2 of the
    last computeActiveErrors that saw each edge. Returns the estimate."""
    idx = np.nonzero(active)[0]
    if idx.size == 0:
        return S
    q = dict(p)
    for k in ("X1", "X2", "obs1", "obs2", "info1", "info2"):
        q[k] = p[k][idx]
    delta = p["delta"]
    lam, ni = 0.0, 2.0
    stats["iters"].append(0)

    def active_chi(Sx):
        e12, e21 = edge_errors(Sx, q)
        c12, c21 = _chi2(e12, q["info1"]), _chi2(e21, q["info2"])
        chi2_last[idx, 0] = c12
        chi2_last[idx, 1] = c21
        return e12, e21, c12, c21

    for it in range(iterations):
        stats["iters"][-1] += 1
        e12, e21, c12, c21 = active_chi(S)
        J12, J21 = numeric_jacobians(S, q, fix_scale)
        H = np.zeros((7, 7))
        b = np.zeros(7)
        chi = 0.0
        with np.errstate(all="ignore"):
            for e, c2, J, info in ((e12, c12, J12, q["info1"]), (e21, c21, J21, q["info2"])):
                r0, r1 = _huber(c2, delta, robust)
                w = r1 * info
                om = -(info[:, None] * e) * r1[:, None]
                H += np.einsum("n,nri,nrj->ij", w, J, J)
                b += np.einsum("nri,nr->i", J, om)
                chi += float(np.sum(r0))
        current = chi
        if it == 0:
            lam = 1e-5 * float(np.fmax.reduce(np.abs(np.diag(H)), initial=0.0))
            ni = 2.0
        rho, qmax = 0.0, 0
        while True:
            x = ldlt_solve(H + lam * np.eye(7), b)
            ok = x is not None
            if not ok:
                x = np.zeros(7)
            Sn = oplus(S, x, fix_scale)
            _, _, c12, c21 = active_chi(Sn)
            with np.errstate(all="ignore"):
                temp = float(np.sum(_huber(c12, delta, robust)[0])) + float(np.sum(_huber(c21, delta, robust)[0]))
                if not ok:
                    temp = np.finfo(np.float64).max
                scale = 1e-3
                for j in range(7):
                    scale += x[j] * (lam * x[j] + b[j])
                rho = (current - temp) / scale
            accepted = bool(rho > 0 and np.isfinite(temp))
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
            qmax += 1
            stats["trials"] += 1
            stats["last_rejected"] = not accepted
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
    return S


def normalized(prob):
    """The arrays of a Sim3Problem-like object (attributes X1c, X2c, obs1, obs2, inv_sigma2_1,
    inv_sigma2_2, cam1, cam2, q, t, s, th2, fix_scale) as float64, read through float32 as the
    library reads them."""
    f = lambda a, shape: np.ascontiguousarray(a, np.float32).reshape(shape).astype(np.float64)  # noqa: E731
    return dict(X1=f(prob.X1c, (-1, 3)), X2=f(prob.X2c, (-1, 3)), obs1=f(prob.obs1, (-1, 2)), obs2=f(prob.obs2, (-1, 2)),
                info1=f(prob.inv_sigma2_1, -1), info2=f(prob.inv_sigma2_2, -1), cam1=f(prob.cam1, 4), cam2=f(prob.cam2, 4),
                q=np.array(prob.q, np.float64).reshape(4), t=np.array(prob.t, np.float64).reshape(3), s=float(prob.s),
                th2=float(prob.th2), fix_scale=bool(prob.fix_scale))


def optimize_sim3(prob, recompute_step2=False):
    """OptimizeSim3 on a Sim3Problem. recompute_step2=True is NOT upstream: it recomputes the chi2
    of step 2 at the estimate (the tests use it to show that the stale values matter)."""
    p = normalized(prob)
    n = p["X1"].shape[0]
    th2, fix = p["th2"], p["fix_scale"]
    p["delta"] = float(np.float32(np.sqrt(th2)))
    S0 = (p["q"].copy(), p["t"].copy(), p["s"])
    keep = np.ones(n, np.uint8)
    stats = dict(trials=0, last_rejected=False, iters=[])
    out = dict(q=S0[0], t=S0[1], s=S0[2], n_in=0, n_bad=0, keep=keep, lm_trials=0, round1_last_rejected=False,
               chi2_step2=np.zeros((n, 2)), chi2_step2_fresh=np.zeros((n, 2)), round_iters=stats["iters"])
    if n == 0:
        return out
    chi2_last = np.zeros((n, 2))
    S = _optimize(S0, p, np.ones(n, bool), True, 5, fix, chi2_last, stats)
    out["round1_last_rejected"] = stats["last_rejected"]
    e12, e21 = edge_errors(S, p)
    fresh = np.stack([_chi2(e12, p["info1"]), _chi2(e21, p["info2"])], 1)
    out["chi2_step2"], out["chi2_step2_fresh"] = chi2_last.copy(), fresh
    c = fresh if recompute_step2 else chi2_last
    with np.errstate(all="ignore"):
        bad = (c[:, 0] > th2) | (c[:, 1] > th2)
    keep[bad] = 0
    n_bad = int(bad.sum())
    out["n_bad"], out["lm_trials"] = n_bad, stats["trials"]
    if n - n_bad < 10:
        return out
    S = _optimize(S, p, ~bad, False, 10 if n_bad > 0 else 5, fix, chi2_last, stats)
    e12, e21 = edge_errors(S, p)
    with np.errstate(all="ignore"):
        late = ((_chi2(e12, p["info1"]) > th2) | (_chi2(e21, p["info2"]) > th2)) & ~bad
    keep[late] = 0
    out.update(q=S[0], t=S[1], s=S[2], n_in=int((~bad & ~late).sum()), lm_trials=stats["trials"])
    return out
