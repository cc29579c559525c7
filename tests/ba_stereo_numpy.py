"""Test infrastructure: an fp64 numpy restatement of oracle/ba_oracle.cpp's ba_solve (the g2o problem
of Optimizer::LocalBundleAdjustment / BundleAdjustment: Levenberg-Marquardt over the Schur
complement of the landmarks) with g2o's EdgeStereoSE3ProjectXYZ added: an observation with
edge_ur >= 0 has the error obs - (fx x/z + cx, fy y/z + cy, fx x/z + cx - bf/z), the information
I3 * invSigma2[octave], the Huber delta huber_delta_stereo, and the third Jacobian row of
linearizeOplus (the first row with bf R[2,:]/z^2 subtracted on the landmark side and
(-bf y/z^2, +bf x/z^2, 0, 0, 0, -bf/z^2) added on the pose side). A monocular edge keeps a zero
third row, so on a problem without stereo edges every sum receives +0 and this is the oracle.

The same order of operations as the oracle where that is a loop over edges or landmarks (numpy's
unbuffered add.at accumulates in index order); the small dense products inside (3- and 6-term dot
products, the LDL^T column updates) are numpy's, which may round differently from the oracle's
left-to-right sums. Returns the keys of oracle.pyoracle.ba_solve. Not used by the product."""
import numpy as np

_F64_MAX = np.finfo(np.float64).max


def _qrot(q, v):
    """Eigen _transformVector, rows of q (x, y, z, w) on rows of v."""
    u = q[..., :3]
    uv = np.cross(u, v)
    uv = uv + uv
    return v + q[..., 3:4] * uv + np.cross(u, uv)


def _normalize_rotation(q):
    q = np.where(q[..., 3:4] < 0, -q, q)
    return q / np.sqrt((q * q).sum(-1, keepdims=True))


def _qtomat(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.stack([1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
                  1 - (txx + tyy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def _mattoq(m):
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t, w])
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
    c = np.zeros(4)
    c[i] = 0.5 * t
    t = 0.5 / t
    c[3] = (m[k, j] - m[j, k]) * t
    c[j] = (m[j, i] + m[i, j]) * t
    c[k] = (m[k, i] + m[i, k]) * t
    return c


def _se3_exp(u):
    ox, oy, oz = u[0], u[1], u[2]
    theta = np.sqrt(ox * ox + oy * oy + oz * oz)
    O = np.array([[0, -oz, oy], [oz, 0, -ox], [-oy, ox, 0]])
    O2 = O @ O
    I = np.eye(3)
    if theta < 0.00001:
        R = I + O + O2
        V = R
    else:
        a, b = np.sin(theta) / theta, (1 - np.cos(theta)) / (theta * theta)
        c = (theta - np.sin(theta)) / theta ** 3
        R = I + a * O + b * O2
        V = I + b * O + c * O2
    return _normalize_rotation(_mattoq(R)), V @ u[3:6]


def _qmul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _inv3(D):
    """Eigen compute_inverse<3x3> (cofactors) of a stack of matrices, as the oracle's inv3."""
    m = D.reshape(-1, 9).T
    c0 = m[4] * m[8] - m[5] * m[7]
    c1 = m[5] * m[6] - m[3] * m[8]
    c2 = m[3] * m[7] - m[4] * m[6]
    det = m[0] * c0 + m[1] * c1 + m[2] * c2
    i = 1.0 / det
    r = np.stack([c0 * i, (m[2] * m[7] - m[1] * m[8]) * i, (m[1] * m[5] - m[2] * m[4]) * i,
                  c1 * i, (m[0] * m[8] - m[2] * m[6]) * i, (m[2] * m[3] - m[0] * m[5]) * i,
                  c2 * i, (m[1] * m[6] - m[0] * m[7]) * i, (m[0] * m[4] - m[1] * m[3]) * i], -1)
    return r.reshape(-1, 3, 3)


def _ldlt_solve(S, b):
    """Dense LDL^T without pivoting in natural order (the oracle's ldlt_solve); None on a bad pivot."""
    n = S.shape[0]
    L = S.copy()
    d = np.zeros(n)
    for j in range(n):
        lj = L[j, :j]
        dj = L[j, j] - (lj * lj * d[:j]).sum()
        if dj == 0.0 or not np.isfinite(dj):
            return None
        d[j] = dj
        L[j + 1:, j] = (L[j + 1:, j] - L[j + 1:, :j] @ (lj * d[:j])) / dj
    x = b.copy()
    for i in range(n):
        x[i] -= L[i, :i] @ x[:i]
    x /= d
    for i in range(n - 1, -1, -1):
        x[i] -= L[i + 1:, i] @ x[i + 1:]
    return x


def _seq_sum(v):
    s = 0.0
    for t in v.tolist():
        s += t
    return s


class StereoBA:
    """The problem in fp64 (float inputs promoted) and the edge math; `prob` is a BAProblem or a
    StereoBAProblem."""

    def __init__(self, prob):
        p = prob.normalized()
        f = lambda v: float(np.float32(v))  # noqa: E731
        self.P, self.M, self.E = p.pose_q.shape[0], p.points.shape[0], p.edge_pose.shape[0]
        self.q = _normalize_rotation(p.pose_q.astype(np.float64))
        self.t = p.pose_t.astype(np.float64)
        self.X = p.points.astype(np.float64)
        self.fixed = p.pose_fixed.astype(bool)
        self.ep, self.em = p.edge_pose.astype(np.int64), p.edge_point.astype(np.int64)
        self.obs = p.edge_uv.astype(np.float64)
        self.info = p.inv_sigma2.astype(np.float64)[p.edge_octave]
        self.fx, self.fy, self.cx, self.cy = f(p.fx), f(p.fy), f(p.cx), f(p.cy)
        self.delta = f(p.huber_delta)
        ur = getattr(p, "edge_ur", None)
        self.ur = np.full(self.E, -1.0) if ur is None else ur.astype(np.float64)
        self.stereo = self.ur >= 0
        self.bf = f(getattr(p, "bf", 0.0))
        self.delta_s = f(getattr(p, "huber_delta_stereo", 0.0))
        if self.stereo.any() and not self.bf > 0:
            raise ValueError("stereo edges need bf > 0")
        self.iterations, self.early_stop = int(p.iterations), int(p.early_stop)
        self.opt = np.where(self.fixed, -1, np.cumsum(~self.fixed) - 1)
        self.np_ = int((~self.fixed).sum())

    def camera_points(self):
        return _qrot(self.q[self.ep], self.X[self.em]) + self.t[self.ep]

    def errors(self):
        """(e [E,3], chi2, rho0, rho1): computeError + RobustKernelHuber::robustify per edge."""
        Xc = self.camera_points()
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        u, v = self.fx * x / z + self.cx, self.fy * y / z + self.cy
        e = np.zeros((self.E, 3))
        e[:, 0] = self.obs[:, 0] - u
        e[:, 1] = self.obs[:, 1] - v
        with np.errstate(all="ignore"):
            e[:, 2] = np.where(self.stereo, self.ur - (u - self.bf / z), 0.0)
        chi2 = self.info * (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2])
        delta = np.where(self.stereo, self.delta_s, self.delta)
        dsqr = delta * delta
        rob = (delta > 0) & (chi2 > dsqr)
        sq = np.sqrt(np.where(rob, chi2, 1.0))
        rho0 = np.where(rob, 2 * sq * delta - dsqr, chi2)
        rho1 = np.where(rob, delta / sq, 1.0)
        return e, chi2, rho0, rho1

    def linearize(self):
        """A [E,3,3] (landmark), B [E,3,6] (pose: omega, upsilon); zero third rows on monocular edges."""
        Xc = self.camera_points()
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        zero = np.zeros(self.E)
        j00, j02 = -(self.fx / z), self.fx * x / (z * z)
        j11, j12 = -(self.fy / z), self.fy * y / (z * z)
        s0 = np.where(self.stereo, j00, 0.0)
        j22 = np.where(self.stereo, j02 - self.bf / (z * z), 0.0)
        R = _qtomat(self.q[self.ep])
        A = np.stack([j00[:, None] * R[:, 0] + j02[:, None] * R[:, 2], j11[:, None] * R[:, 1] + j12[:, None] * R[:, 2],
                      s0[:, None] * R[:, 0] + j22[:, None] * R[:, 2]], 1)
        B = np.stack([np.stack([j02 * y, j00 * z - j02 * x, -j00 * y, j00, zero, j02], -1),
                      np.stack([j12 * y - j11 * z, -j12 * x, j11 * x, zero, j11, j12], -1),
                      np.stack([j22 * y, s0 * z - j22 * x, -s0 * y, s0, zero, j22], -1)], 1)
        return A, B

    def landmark_hessians(self, rho1=None):
        """Hll [M,3,3] of the current state (robust weights rho1, default: from the current errors)."""
        if rho1 is None:
            rho1 = self.errors()[3]
        A, _ = self.linearize()
        Hll = np.zeros((self.M, 3, 3))
        np.add.at(Hll, self.em, (rho1 * self.info)[:, None, None] * np.einsum("eki,ekj->eij", A, A))
        return Hll


def ba_solve(prob):
    """The oracle's solve() on a BAProblem / StereoBAProblem; returns pyoracle.ba_solve's dict."""
    s = StereoBA(prob)
    P, M, E, npo = s.P, s.M, s.E, s.np_
    n = 6 * npo
    opt = s.opt
    eo = opt[s.ep]
    # landmark columns: the edges of optimised poses per point, by pose optimisation index (stable)
    act = np.nonzero(eo >= 0)[0]
    order = act[np.lexsort((act, eo[act], s.em[act]))]
    cols = np.split(order, np.cumsum(np.bincount(s.em[order], minlength=M))[:-1]) if M else []
    pa, pb = [], []
    for c in cols:
        k = len(c)
        ia, ib = np.triu_indices(k)
        pa.append(c[ia])
        pb.append(c[ib])
    pa = np.concatenate(pa) if pa else np.zeros(0, np.int64)
    pb = np.concatenate(pb) if pb else np.zeros(0, np.int64)
    same = (eo[pa] == eo[pb]) & (pa != pb)   # distinct edges of one pose: the mirrored term
    st = dict(chi2=None)

    def errors():
        e, chi2, rho0, rho1 = s.errors()
        st.update(e=e, chi2=chi2, rho1=rho1)
        return _seq_sum(rho0)

    lam, ni, nBad = 0.0, 2.0, 0
    currentChi = errors()
    chi2_init = currentChi
    iters = trials = 0
    for it in range(s.iterations):
        if it > 0:
            currentChi = errors()
        A, B = s.linearize()
        e, rho1 = st["e"], st["rho1"]
        w = rho1 * s.info
        om = -s.info[:, None] * e * rho1[:, None]
        b = np.zeros(n + 3 * M)
        bl = b[n:].reshape(M, 3)
        np.add.at(bl, s.em, np.einsum("eki,ek->ei", A, om))
        Hll = np.zeros((M, 3, 3))
        np.add.at(Hll, s.em, w[:, None, None] * np.einsum("eki,ekj->eij", A, A))
        Hpp = np.zeros((npo, 6, 6))
        bp = b[:n].reshape(npo, 6)
        np.add.at(bp, eo[act], np.einsum("eki,ek->ei", B[act], om[act]))
        np.add.at(Hpp, eo[act], w[act, None, None] * np.einsum("eki,ekj->eij", B[act], B[act]))
        Hpl = w[:, None, None] * np.einsum("eki,ekj->eij", B, A)   # [E,6,3]
        if it == 0:
            md = 0.0
            if npo:
                md = max(md, np.abs(np.einsum("ijj->ij", Hpp)).max())
            if M:
                md = max(md, np.abs(np.einsum("ijj->ij", Hll)).max())
            lam, ni, nBad = 1e-5 * md, 2.0, 0
        rho, qmax = 0.0, 0
        while True:
            q_bak, t_bak, X_bak = s.q.copy(), s.t.copy(), s.X.copy()
            S4 = np.zeros((npo, 6, npo, 6))
            ii = np.arange(npo)
            S4[ii, :, ii, :] = Hpp + lam * np.eye(6)
            with np.errstate(all="ignore"):
                Dinv = _inv3(Hll + lam * np.eye(3))
            db = np.einsum("mij,mj->mi", Dinv, bl)
            coeff = np.zeros((npo, 6))
            np.add.at(coeff, eo[order], np.einsum("eij,ej->ei", Hpl[order], db[s.em[order]]))
            BD = np.einsum("eij,ejk->eik", Hpl[pa], Dinv[s.em[pa]])
            V = np.einsum("eik,ejk->eij", BD, Hpl[pb])
            i1, i2 = eo[pa], eo[pb]
            np.subtract.at(S4, (i1, slice(None), i2, slice(None)), V)
            off = i1 != i2
            np.subtract.at(S4, (i2[off], slice(None), i1[off], slice(None)), V[off].transpose(0, 2, 1))
            if same.any():
                V2 = np.einsum("eik,ekl,ejl->eij", Hpl[pb[same]], Dinv[s.em[pa[same]]], Hpl[pa[same]])
                np.subtract.at(S4, (i1[same], slice(None), i2[same], slice(None)), V2)
            S = S4.reshape(n, n)
            bs = b[:n] - coeff.reshape(-1)
            xp = _ldlt_solve(S, bs) if n and np.isfinite(S).all() else (np.zeros(0) if n == 0 else None)
            ok2 = xp is not None
            if not ok2:
                xp = np.zeros(n)
            cl3 = bl.copy()
            np.subtract.at(cl3, s.em[order], np.einsum("eij,ei->ej", Hpl[order], xp.reshape(npo, 6)[eo[order]]))
            xl = np.einsum("mij,mj->mi", Dinv, cl3)
            x = np.concatenate([xp, xl.reshape(-1)])
            for i in range(P):
                if opt[i] >= 0:
                    dq, dt = _se3_exp(xp[6 * opt[i]:6 * opt[i] + 6])
                    s.t[i] = dt + _qrot(dq, s.t[i])
                    s.q[i] = _normalize_rotation(_qmul(dq, s.q[i]))
            s.X = s.X + xl
            with np.errstate(all="ignore"):
                tempChi = errors()
            if not ok2:
                tempChi = _F64_MAX
            rho = currentChi - tempChi
            with np.errstate(all="ignore"):
                scale = _seq_sum(x * (lam * x + b)) + 1e-3
                rho /= scale
            if rho > 0 and np.isfinite(tempChi):
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                if s.early_stop:
                    nBad = nBad + 1 if (currentChi - tempChi) < 1e-3 * currentChi else 0
                currentChi = tempChi
            else:
                lam *= ni
                ni *= 2
                s.q, s.t, s.X = q_bak, t_bak, X_bak
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        iters = it + 1
        if qmax == 10 or rho == 0:
            break
        if s.early_stop and nBad >= 3:
            break
    chi2_e = st["chi2"] if st["chi2"] is not None else np.zeros(E)
    z = s.camera_points()[:, 2] if E else np.zeros(0)
    return dict(pose_q=s.q.astype(np.float32), pose_t=s.t.astype(np.float32), points=s.X.astype(np.float32),
                edge_chi2=chi2_e.astype(np.float32), edge_depth_ok=(z > 0).astype(np.uint8), initial_chi2=chi2_init,
                final_chi2=currentChi, iterations_done=iters, lm_trials=trials)
