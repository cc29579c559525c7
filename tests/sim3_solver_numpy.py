"""Sim3Solver restated in numpy (DESIGN.md "Sim3Solver"), the yardstick of orbhip_sim3_solve_batch:
the device must equal it bit for bit.

The fp32 parts are np.float32 operations, one rounding per operation in the written order (scalars
for the hypothesis, elementwise arrays over the correspondences for CheckInliers: the same IEEE
operations). The Jacobi and the normalisation run on Python floats (fp64) with math.sqrt. Also here:
upstream's literal sequential iterate() with its state, the order-free selection the kernels apply,
the literal float64 / float32 closed form (np.linalg.eigh, angle-axis, exp) the accuracy test
measures against, and the parity scene set."""
import functools
import math

import numpy as np

F = np.float32
SWEEPS = 6            # what the library ships: the measured need (SWEEPS_NEEDED) + 1
SWEEPS_NEEDED = 5
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))


def _div(a, b):
    """IEEE fp64 division on Python floats (Python raises on a zero divisor)."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(x):
    return math.nan if x != x or x < 0.0 else math.sqrt(x)


def jacobi_eigvec(N, sweeps=SWEEPS):
    """The eigenvector (w, x, y, z) of the symmetric 4x4 N's largest eigenvalue (in value), not
    normalised: a two-sided cyclic Jacobi over PAIRS, `sweeps` sweeps; ties go to the lowest column."""
    A = [[float(N[r][c]) for c in range(4)] for r in range(4)]   # only r <= c is read or written
    V = [[1.0 if r == c else 0.0 for c in range(4)] for r in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            g = A[p][q]
            if g == 0.0:
                continue
            zeta = _div(A[q][q] - A[p][p], 2.0 * g)
            t = _div(1.0, abs(zeta) + _sqrt(1.0 + zeta * zeta))
            if zeta < 0.0:
                t = -t
            c = _div(1.0, _sqrt(1.0 + t * t))
            s = c * t
            A[p][p] = A[p][p] - t * g
            A[q][q] = A[q][q] + t * g
            A[p][q] = 0.0
            for r in range(4):
                if r != p and r != q:
                    ip = (r, p) if r < p else (p, r)
                    iq = (r, q) if r < q else (q, r)
                    x, y = A[ip[0]][ip[1]], A[iq[0]][iq[1]]
                    A[ip[0]][ip[1]] = c * x - s * y
                    A[iq[0]][iq[1]] = s * x + c * y
                vx, vy = V[r][p], V[r][q]
                V[r][p] = c * vx - s * vy
                V[r][q] = s * vx + c * vy
    best, k = A[0][0], 0
    for j in range(1, 4):
        if A[j][j] > best:
            best, k = A[j][j], j
    return [V[r][k] for r in range(4)]


def quat_to_matrix(q):
    """geom.h quat_to_matrix, float32; q = (x, y, z, w)."""
    two = F(2)
    tx, ty, tz = two * q[0], two * q[1], two * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    one = F(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], F)


def horn_matrix(X1, X2, tri):
    """-> (N 4x4 float32 (upper triangle), Pr1, Pr2 as [point k][coordinate], O1, O2)"""
    P1 = [[F(X1[i, j]) for j in range(3)] for i in tri]
    P2 = [[F(X2[i, j]) for j in range(3)] for i in tri]
    three = F(3)
    O1 = [((P1[0][j] + P1[1][j]) + P1[2][j]) / three for j in range(3)]
    O2 = [((P2[0][j] + P2[1][j]) + P2[2][j]) / three for j in range(3)]
    P1 = [[P1[k][j] - O1[j] for j in range(3)] for k in range(3)]
    P2 = [[P2[k][j] - O2[j] for j in range(3)] for k in range(3)]
    M = [[(P2[0][i] * P1[0][j] + P2[1][i] * P1[1][j]) + P2[2][i] * P1[2][j] for j in range(3)] for i in range(3)]
    N = np.zeros((4, 4), F)
    N[0, 0] = (M[0][0] + M[1][1]) + M[2][2]
    N[0, 1] = M[1][2] - M[2][1]
    N[0, 2] = M[2][0] - M[0][2]
    N[0, 3] = M[0][1] - M[1][0]
    N[1, 1] = (M[0][0] - M[1][1]) - M[2][2]
    N[1, 2] = M[0][1] + M[1][0]
    N[1, 3] = M[2][0] + M[0][2]
    N[2, 2] = (-M[0][0] + M[1][1]) - M[2][2]
    N[2, 3] = M[1][2] + M[2][1]
    N[3, 3] = (-M[0][0] - M[1][1]) + M[2][2]
    return N, P1, P2, O1, O2


def compute_sim3(X1, X2, tri, fix_scale, sweeps=SWEEPS):
    """ComputeSim3 on one triple -> dict(s, R, t, sR, Ri, ti) in float32."""
    with np.errstate(all="ignore"):
        N, P1, P2, O1, O2 = horn_matrix(X1, X2, tri)
        w, x, y, z = jacobi_eigvec(N, sweeps)
        nrm = _sqrt(((w * w + x * x) + y * y) + z * z)
        q = [F(_div(x, nrm)), F(_div(y, nrm)), F(_div(z, nrm)), F(_div(w, nrm))]
        R = quat_to_matrix(q)
        s = F(1)
        if not fix_scale:
            nom = den = None
            for k in range(3):          # column-major over the 3 x 3 matrices
                for i in range(3):
                    p3 = (R[i, 0] * P2[k][0] + R[i, 1] * P2[k][1]) + R[i, 2] * P2[k][2]
                    a1, a2 = P1[k][i] * p3, p3 * p3
                    nom = a1 if nom is None else nom + a1
                    den = a2 if den is None else den + a2
            s = nom / den
        sR = np.array([[s * R[i, j] for j in range(3)] for i in range(3)], F)
        t = np.array([O1[i] - ((sR[i, 0] * O2[0] + sR[i, 1] * O2[1]) + sR[i, 2] * O2[2]) for i in range(3)], F)
        sinv = F(1) / s
        Ri = np.array([[sinv * R[j, i] for j in range(3)] for i in range(3)], F)
        ti = np.array([-((Ri[i, 0] * t[0] + Ri[i, 1] * t[1]) + Ri[i, 2] * t[2]) for i in range(3)], F)
    return dict(s=F(s), R=R, t=t, sR=sR, Ri=Ri, ti=ti)


def _project(cam, X):
    fx, fy, cx, cy = (F(c) for c in cam)
    return (fx * X[:, 0]) / X[:, 2] + cx, (fy * X[:, 1]) / X[:, 2] + cy


def _transform(A, t, X):
    return np.stack([((A[r, 0] * X[:, 0] + A[r, 1] * X[:, 1]) + A[r, 2] * X[:, 2]) + t[r] for r in range(3)], 1)


def check_inliers(hyp, X1, X2, cam1, cam2, max_err1, max_err2):
    """CheckInliers of one hypothesis over all correspondences -> bool[n]."""
    with np.errstate(all="ignore"):
        p1u, p1v = _project(cam1, X1)
        p2u, p2v = _project(cam2, X2)
        q1u, q1v = _project(cam1, _transform(hyp["sR"], hyp["t"], X2))
        q2u, q2v = _project(cam2, _transform(hyp["Ri"], hyp["ti"], X1))
        d1u, d1v, d2u, d2v = p1u - q1u, p1v - q1v, q2u - p2u, q2v - p2v
        e1 = d1u * d1u + d1v * d1v
        e2 = d2u * d2u + d2v * d2v
        assert e1.dtype == F and e2.dtype == F
        return (e1 < max_err1) & (e2 < max_err2)


def pack13(hyp):
    return np.concatenate([[hyp["s"]], hyp["R"].reshape(9), hyp["t"]]).astype(F)


def select(n_inliers, min_inliers):
    """The order-free selection -> (converged or -1, best): the first h above the minimum; else the
    last h of the largest count."""
    n = np.asarray(n_inliers)
    above = np.nonzero(n > min_inliers)[0]
    if above.size:
        return int(above[0]), int(above[0])
    return -1, int(np.nonzero(n == n.max())[0][-1])


def solve(X1, X2, max_err1, max_err2, cam1, cam2, fix_scale, min_inliers, triples, sweeps=SWEEPS):
    """What orbhip_sim3_solve computes -> dict(n_inliers[H], hyp[H, 13], masks[H, n], converged, best,
    sel[13], inliers[n])."""
    X1, X2 = np.asarray(X1, F), np.asarray(X2, F)
    e1, e2 = np.asarray(max_err1, F), np.asarray(max_err2, F)
    H = len(triples)
    n_inl = np.zeros(H, np.int32)
    hyp = np.zeros((H, 13), F)
    masks = np.zeros((H, X1.shape[0]), bool)
    for h, tri in enumerate(triples):
        hy = compute_sim3(X1, X2, [int(i) for i in tri], fix_scale, sweeps)
        masks[h] = check_inliers(hy, X1, X2, cam1, cam2, e1, e2)
        n_inl[h] = masks[h].sum()
        hyp[h] = pack13(hy)
    conv, best = select(n_inl, min_inliers)
    return dict(n_inliers=n_inl, hyp=hyp, masks=masks, converged=conv, best=best, sel=hyp[best].copy(),
                inliers=masks[best].copy())


def T12_of(h13):
    T = np.eye(4, dtype=F)
    T[:3, :3] = h13[0] * h13[1:10].reshape(3, 3)
    T[:3, 3] = h13[10:13]
    return T


class LiteralSolver:
    """Upstream's iterate(), literally: one hypothesis after the other with the class state
    (mnIterations, mnBestInliers, mBestT12, mvbBestInliers) kept across chunked calls."""

    def __init__(self, scene, min_inliers, max_its, triples):
        self.s, self.min_inliers, self.max_its, self.triples = scene, int(min_inliers), int(max_its), triples
        self.mnIterations = 0
        self.mnBestInliers = 0
        self.mBestT12 = np.eye(4, dtype=F)
        self.best_h = -1
        self.N = scene["X1"].shape[0]

    def iterate(self, nIterations):
        s = self.s
        vb = np.zeros(s["n1"], bool)
        if self.N < self.min_inliers:
            return np.eye(4, dtype=F), True, vb, 0, False
        n_cur = 0
        while self.mnIterations < self.max_its and n_cur < nIterations:
            h = self.mnIterations
            n_cur += 1
            self.mnIterations += 1
            hy = compute_sim3(s["X1"], s["X2"], [int(i) for i in self.triples[h]], s["fix_scale"])
            m = check_inliers(hy, s["X1"], s["X2"], s["cam1"], s["cam2"], s["max_err1"], s["max_err2"])
            n_h = int(m.sum())
            if n_h >= self.mnBestInliers:
                self.mnBestInliers, self.best_h = n_h, h
                self.mBestT12 = T12_of(pack13(hy))
                if n_h > self.min_inliers:
                    vb[s["indices1"][m]] = True
                    return self.mBestT12.copy(), False, vb, n_h, True
        return self.mBestT12.copy(), self.mnIterations >= self.max_its, vb, 0, False


def literal_from_counts(n_inliers, min_inliers, chunk):
    """The selection part of the literal loop alone, over given counts in chunks of `chunk` ->
    (converged or -1, best), as the state stands when the loop ends."""
    best_n, best_h, h, H = 0, -1, 0, len(n_inliers)
    while h < H:
        for _ in range(chunk):
            if h >= H:
                break
            if n_inliers[h] >= best_n:
                best_n, best_h = int(n_inliers[h]), h
                if n_inliers[h] > min_inliers:
                    return h, h
            h += 1
    return -1, best_h


# ---- the literal closed form (accuracy yardstick) ----
def literal_sim3(N32, P1, P2, O1, O2, fix_scale, dtype):
    """Upstream's ComputeSim3 after M: the eigenvector by LAPACK (np.linalg.eigh in `dtype`), the
    angle-axis vector through atan2, the rotation by exp (Rodrigues) -> (R, s, t) in `dtype`."""
    Nf = np.array(N32, dtype)
    Nf = np.triu(Nf) + np.triu(Nf, 1).T
    w, v = np.linalg.eigh(Nf)
    e = v[:, int(np.argmax(w))].astype(dtype)
    vec = e[1:4]
    nv = np.sqrt((vec * vec).sum(dtype=dtype))
    ang = np.arctan2(nv, e[0]).astype(dtype)
    with np.errstate(all="ignore"):
        rv = (dtype(2) * ang * vec / nv).astype(dtype)
    th = np.sqrt((rv * rv).sum(dtype=dtype))
    K = np.array([[0, -rv[2], rv[1]], [rv[2], 0, -rv[0]], [-rv[1], rv[0], 0]], dtype)
    if th < np.finfo(dtype).eps:
        R = np.eye(3, dtype=dtype) + K
    else:
        R = (np.eye(3, dtype=dtype) + (np.sin(th) / th).astype(dtype) * K
             + ((dtype(1) - np.cos(th)) / (th * th)).astype(dtype) * (K @ K)).astype(dtype)
    Pr1 = np.array(P1, dtype).T   # 3 x 3, columns = points
    Pr2 = np.array(P2, dtype).T
    P3 = (R @ Pr2).astype(dtype)
    s = dtype(1) if fix_scale else dtype((Pr1 * P3).sum(dtype=dtype) / (P3 * P3).sum(dtype=dtype))
    t = (np.array(O1, dtype) - s * (R @ np.array(O2, dtype))).astype(dtype)
    return R, s, t


# ---- the parity scenes ----
PARITY_CASES = ((257, 0.6, 6), (100, 0.85, 3), (30, 0.4, 2), (20, 0.3, 3))   # (n, outlier fraction, seed)
PARITY_H = 300
PARITY_MIN_INLIERS = 15


@functools.lru_cache(maxsize=None)
def parity_scene(k, fix_scale):
    """Scene k of the set with its expected result (computed once, shared; treat as read-only)."""
    from orb_slam3_ros2_amd.synthetic import synthetic_sim3_solver_scene
    n, frac, seed = PARITY_CASES[k]
    s = synthetic_sim3_solver_scene(n, frac, seed, bool(fix_scale), n_hyp=PARITY_H, min_inliers=PARITY_MIN_INLIERS)
    s["expected"] = solve_scene(s)
    return s


def solve_scene(s, triples=None, min_inliers=None):
    return solve(s["X1"], s["X2"], s["max_err1"], s["max_err2"], s["cam1"], s["cam2"], s["fix_scale"],
                 s["min_inliers"] if min_inliers is None else min_inliers, s["triples"] if triples is None else triples)
