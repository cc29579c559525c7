"""TwoViewReconstruction restated in numpy (DESIGN.md "TwoViewReconstruction"), the yardstick of
orbhip_two_view_reconstruct_batch: the device must equal it bit for bit (parallax up to acosf).

The fp32 parts are np.float32 operations, one rounding per operation in the written order,
elementwise over the hypotheses or over the matches (the same IEEE operations as one scalar after
the other). The Jacobi iterations run in np.float64, elementwise over the batch, with the kernels'
rotation formulas and pair order. Also here: upstream's literal loop with its fp32 running score
(LiteralSolver), the order-free selection, and np.linalg.svd solutions the accuracy test measures
against."""
import functools
import math

import numpy as np

F = np.float32
D = np.float64
SWEEPS9 = 9          # what the library ships for the 9x9 null vector: SWEEPS9_NEEDED + 1
SWEEPS9_NEEDED = 8
SWEEPS3 = 5          # the 3x3 SVDs: SWEEPS3_NEEDED + 1
SWEEPS3_NEEDED = 4
SWEEPS4 = 6          # the triangulation's 4x4, as CreateNewMapPoints
TH_H = F(5.991)
TH_F = F(3.841)
TH_SCORE = F(5.991)
COS_LIMIT = F(0.99998)
MIN_PARALLAX = F(1.0)
MIN_TRIANGULATED = 50


def _quiet():
    return np.errstate(all="ignore")


# ---- fp32 3x3 helpers: entry (i, j) = (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j ----
def mm3(A, B):
    A, B = np.asarray(A, F), np.asarray(B, F)
    out = np.empty(np.broadcast_shapes(A.shape, B.shape), F)
    for i in range(3):
        for j in range(3):
            out[..., i, j] = (A[..., i, 0] * B[..., 0, j] + A[..., i, 1] * B[..., 1, j]) + A[..., i, 2] * B[..., 2, j]
    return out


def mv3(A, v):
    A, v = np.asarray(A, F), np.asarray(v, F)
    return np.stack([(A[..., i, 0] * v[..., 0] + A[..., i, 1] * v[..., 1]) + A[..., i, 2] * v[..., 2]
                     for i in range(3)], -1)


def det3(M):
    M = np.asarray(M, F)
    c0 = M[..., 1, 1] * M[..., 2, 2] - M[..., 1, 2] * M[..., 2, 1]
    c1 = M[..., 1, 2] * M[..., 2, 0] - M[..., 1, 0] * M[..., 2, 2]
    c2 = M[..., 1, 0] * M[..., 2, 1] - M[..., 1, 1] * M[..., 2, 0]
    return (M[..., 0, 0] * c0 + M[..., 0, 1] * c1) + M[..., 0, 2] * c2


def inv3(M):
    """The adjugate over the determinant (first-row expansion); a singular M gives inf / NaN."""
    M = np.asarray(M, F)
    m = lambda i, j: M[..., i, j]
    c0 = m(1, 1) * m(2, 2) - m(1, 2) * m(2, 1)
    c1 = m(1, 2) * m(2, 0) - m(1, 0) * m(2, 2)
    c2 = m(1, 0) * m(2, 1) - m(1, 1) * m(2, 0)
    det = (m(0, 0) * c0 + m(0, 1) * c1) + m(0, 2) * c2
    with _quiet():
        d = F(1) / det
        out = np.empty(M.shape, F)
        out[..., 0, 0] = c0 * d
        out[..., 0, 1] = (m(0, 2) * m(2, 1) - m(0, 1) * m(2, 2)) * d
        out[..., 0, 2] = (m(0, 1) * m(1, 2) - m(0, 2) * m(1, 1)) * d
        out[..., 1, 0] = c1 * d
        out[..., 1, 1] = (m(0, 0) * m(2, 2) - m(0, 2) * m(2, 0)) * d
        out[..., 1, 2] = (m(0, 2) * m(1, 0) - m(0, 0) * m(1, 2)) * d
        out[..., 2, 0] = c2 * d
        out[..., 2, 1] = (m(0, 1) * m(2, 0) - m(0, 0) * m(2, 1)) * d
        out[..., 2, 2] = (m(0, 0) * m(1, 1) - m(0, 1) * m(1, 0)) * d
    return out


# ---- Normalize ----
def _seq_sum(v):
    """upstream's running fp32 sum in index order"""
    return np.cumsum(np.asarray(v, F), dtype=F)[-1]


def normalize(x, y):
    """-> (xn, yn, T 3x3, Tinv 3x3) in fp32; Tinv in closed form (1/sX, 0, meanX; ...)"""
    x, y = np.asarray(x, F), np.asarray(y, F)
    n = F(len(x))
    with _quiet():
        mx, my = _seq_sum(x) / n, _seq_sum(y) / n
        xn, yn = x - mx, y - my
        dx, dy = _seq_sum(np.abs(xn)) / n, _seq_sum(np.abs(yn)) / n
        sx, sy = F(1) / dx, F(1) / dy
        xn, yn = xn * sx, yn * sy
        T = np.array([[sx, 0, -mx * sx], [0, sy, -my * sy], [0, 0, 1]], F)
        Ti = np.array([[F(1) / sx, 0, mx], [0, F(1) / sy, my], [0, 0, 1]], F)
    return xn, yn, T, Ti


# ---- Jacobi iterations (fp64, batched over the leading axis) ----
def _rotation(a, b, g):
    """tri_jacobi_pair's / sim3_jacobi_pair's rotation for diagonal (a, b) and off-diagonal g"""
    zeta = (b - a) / (2.0 * g)
    t = 1.0 / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
    t = np.where(zeta < 0.0, -t, t)
    c = 1.0 / np.sqrt(1.0 + t * t)
    return t, c, c * t


def jacobi_sym(G, sweeps):
    """Two-sided cyclic Jacobi on the symmetric G (batch, n, n; the upper triangle is kept) ->
    (diagonal (batch, n), V (batch, n, n) with the eigenvectors in its columns)."""
    A = np.array(G, D)
    B, n = A.shape[0], A.shape[1]
    V = np.broadcast_to(np.eye(n), A.shape).copy()
    with _quiet():
        for _ in range(sweeps):
            for p in range(n):
                for q in range(p + 1, n):
                    g = A[:, p, q].copy()
                    act = g != 0.0
                    t, c, s = _rotation(A[:, p, p], A[:, q, q], g)
                    A[:, p, p] = np.where(act, A[:, p, p] - t * g, A[:, p, p])
                    A[:, q, q] = np.where(act, A[:, q, q] + t * g, A[:, q, q])
                    A[:, p, q] = np.where(act, 0.0, g)
                    for r in range(n):
                        if r != p and r != q:
                            ip = (r, p) if r < p else (p, r)
                            iq = (r, q) if r < q else (q, r)
                            x, y = A[:, ip[0], ip[1]].copy(), A[:, iq[0], iq[1]].copy()
                            A[:, ip[0], ip[1]] = np.where(act, c * x - s * y, x)
                            A[:, iq[0], iq[1]] = np.where(act, s * x + c * y, y)
                        vx, vy = V[:, r, p].copy(), V[:, r, q].copy()
                        V[:, r, p] = np.where(act, c * vx - s * vy, vx)
                        V[:, r, q] = np.where(act, s * vx + c * vy, vy)
    return np.stack([A[:, k, k] for k in range(n)], 1), V


def null_vector(rows, sweeps=SWEEPS9):
    """rows: (batch, m, 9) fp32 -> the eigenvector (batch, 9, fp64) of the smallest eigenvalue of
    the Gram matrix sum_r a_r a_r^T (fp64, rows added in order), the lowest column among equals."""
    a = np.asarray(rows, F).astype(D)
    G = np.zeros((a.shape[0], 9, 9), D)
    with _quiet():
        for r in range(a.shape[1]):
            G = G + a[:, r, :, None] * a[:, r, None, :]
        d, V = jacobi_sym(G, sweeps)
        k = np.zeros(a.shape[0], np.int64)
        best = d[:, 0].copy()
        for j in range(1, 9):
            less = d[:, j] < best
            best = np.where(less, d[:, j], best)
            k = np.where(less, j, k)
    return V[np.arange(a.shape[0]), :, k]


def onesided(M, sweeps, n):
    """One-sided cyclic Jacobi on the columns of M (batch, n, n) -> (U = M W with orthogonal
    columns, W); tri_jacobi_pair's order."""
    U = np.array(M, D)
    W = np.broadcast_to(np.eye(n), U.shape).copy()
    with _quiet():
        for _ in range(sweeps):
            for p in range(n):
                for q in range(p + 1, n):
                    a = U[:, 0, p] * U[:, 0, p] + U[:, 1, p] * U[:, 1, p]
                    b = U[:, 0, q] * U[:, 0, q] + U[:, 1, q] * U[:, 1, q]
                    g = U[:, 0, p] * U[:, 0, q] + U[:, 1, p] * U[:, 1, q]
                    for r in range(2, n):
                        a = a + U[:, r, p] * U[:, r, p]
                        b = b + U[:, r, q] * U[:, r, q]
                        g = g + U[:, r, p] * U[:, r, q]
                    act = g != 0.0
                    _, c, s = _rotation(a, b, g)
                    for X in (U, W):
                        for i in range(n):
                            x, y = X[:, i, p].copy(), X[:, i, q].copy()
                            X[:, i, p] = np.where(act, c * x - s * y, x)
                            X[:, i, q] = np.where(act, s * x + c * y, y)
    return U, W


def svd3(M, sweeps=SWEEPS3):
    """M (batch, 3, 3) = Q diag(sig) W^T in fp64 -> (Q, sig, W, C, order): W's columns are the
    accumulated rotations in the order of descending column norm of C = M W (the first of equals
    first, the last of equals last), sig the norms, Q's first two columns the normalised columns of
    C, its third their cross product with the sign of its product with C's third column. C and
    order are the unsorted columns and the permutation."""
    C, W = onesided(np.asarray(M, D), sweeps, 3)
    B = C.shape[0]
    with _quiet():
        n = np.stack([(C[:, 0, k] * C[:, 0, k] + C[:, 1, k] * C[:, 1, k]) + C[:, 2, k] * C[:, 2, k] for k in range(3)], 1)
        i0 = np.zeros(B, np.int64)
        best = n[:, 0].copy()
        for k in (1, 2):
            m = n[:, k] > best
            best, i0 = np.where(m, n[:, k], best), np.where(m, k, i0)
        i2 = np.zeros(B, np.int64)
        best = n[:, 0].copy()
        for k in (1, 2):
            m = n[:, k] <= best
            best, i2 = np.where(m, n[:, k], best), np.where(m, k, i2)
        same = i0 == i2
        i0, i2 = np.where(same, 0, i0), np.where(same, 2, i2)
        i1 = 3 - i0 - i2
        order = np.stack([i0, i1, i2], 1)
        ar = np.arange(B)[:, None]
        Cs = np.stack([C[ar[:, 0], :, order[:, k]] for k in range(3)], 2)
        Ws = np.stack([W[ar[:, 0], :, order[:, k]] for k in range(3)], 2)
        sig = np.sqrt(np.stack([n[ar[:, 0], order[:, k]] for k in range(3)], 1))
        q0 = Cs[:, :, 0] / sig[:, 0:1]
        q1 = Cs[:, :, 1] / sig[:, 1:2]
        q2 = np.stack([q0[:, 1] * q1[:, 2] - q0[:, 2] * q1[:, 1], q0[:, 2] * q1[:, 0] - q0[:, 0] * q1[:, 2],
                       q0[:, 0] * q1[:, 1] - q0[:, 1] * q1[:, 0]], 1)
        dot = (q2[:, 0] * Cs[:, 0, 2] + q2[:, 1] * Cs[:, 1, 2]) + q2[:, 2] * Cs[:, 2, 2]
        q2 = np.where((dot < 0.0)[:, None], -q2, q2)
    return np.stack([q0, q1, q2], 2), sig, Ws, Cs


# ---- the two solvers, for all hypotheses at once ----
def rows_h(u1, v1, u2, v2):
    """(batch, 8) normalised coordinates -> (batch, 16, 9) fp32"""
    z, one = np.zeros_like(u1), np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -one, v2 * u1, v2 * v1, v2], -1)
    r1 = np.stack([u1, v1, one, z, z, z, -(u2 * u1), -(u2 * v1), -u2], -1)
    return np.stack([r0, r1], 2).reshape(u1.shape[0], 16, 9)


def rows_f(u1, v1, u2, v2):
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1)


def compute_h21(pn, sets, T1, T2inv, sweeps=SWEEPS9):
    """-> (H21, H12) (batch, 3, 3) fp32"""
    u1, v1, u2, v2 = (p[sets] for p in pn)
    Hn = null_vector(rows_h(u1, v1, u2, v2), sweeps).astype(F).reshape(-1, 3, 3)
    H21 = mm3(mm3(T2inv, Hn), T1)
    return H21, inv3(H21)


def compute_f21(pn, sets, T1, T2, sweeps=SWEEPS9, sweeps3=SWEEPS3):
    u1, v1, u2, v2 = (p[sets] for p in pn)
    Fpre = null_vector(rows_f(u1, v1, u2, v2), sweeps).astype(F).reshape(-1, 3, 3)
    _, _, W, C = svd3(Fpre.astype(D), sweeps3)
    with _quiet():
        Fn = (C[:, :, None, 0] * W[:, None, :, 0] + C[:, :, None, 1] * W[:, None, :, 1]).astype(F)
    return mm3(mm3(T2.T.copy(), Fn), T1)


def homography_terms(H21, H12, pts, inv_sigma2):
    """CheckHomography for one hypothesis over all matches -> (terms (2, N) fp32, inlier (N,))"""
    u1, v1, u2, v2 = pts
    with _quiet():
        w = F(1) / ((H12[2, 0] * u2 + H12[2, 1] * v2) + H12[2, 2])
        a = ((H12[0, 0] * u2 + H12[0, 1] * v2) + H12[0, 2]) * w
        b = ((H12[1, 0] * u2 + H12[1, 1] * v2) + H12[1, 2]) * w
        chi1 = ((u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)) * inv_sigma2
        w = F(1) / ((H21[2, 0] * u1 + H21[2, 1] * v1) + H21[2, 2])
        a = ((H21[0, 0] * u1 + H21[0, 1] * v1) + H21[0, 2]) * w
        b = ((H21[1, 0] * u1 + H21[1, 1] * v1) + H21[1, 2]) * w
        chi2 = ((u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)) * inv_sigma2
        out1, out2 = chi1 > TH_H, chi2 > TH_H
        terms = np.stack([np.where(out1, F(0), TH_H - chi1), np.where(out2, F(0), TH_H - chi2)])
    assert terms.dtype == F
    return terms, ~out1 & ~out2


def fundamental_terms(F21, pts, inv_sigma2):
    u1, v1, u2, v2 = pts
    f = F21
    with _quiet():
        a2 = (f[0, 0] * u1 + f[0, 1] * v1) + f[0, 2]
        b2 = (f[1, 0] * u1 + f[1, 1] * v1) + f[1, 2]
        c2 = (f[2, 0] * u1 + f[2, 1] * v1) + f[2, 2]
        num2 = (a2 * u2 + b2 * v2) + c2
        chi1 = ((num2 * num2) / (a2 * a2 + b2 * b2)) * inv_sigma2
        a1 = (f[0, 0] * u2 + f[1, 0] * v2) + f[2, 0]
        b1 = (f[0, 1] * u2 + f[1, 1] * v2) + f[2, 1]
        c1 = (f[0, 2] * u2 + f[1, 2] * v2) + f[2, 2]
        num1 = (a1 * u1 + b1 * v1) + c1
        chi2 = ((num1 * num1) / (a1 * a1 + b1 * b1)) * inv_sigma2
        out1, out2 = chi1 > TH_F, chi2 > TH_F
        terms = np.stack([np.where(out1, F(0), TH_SCORE - chi1), np.where(out2, F(0), TH_SCORE - chi2)])
    assert terms.dtype == F
    return terms, ~out1 & ~out2


def score_of(terms):
    """The order-free score: the terms added in fp64 (exact, tests/test_two_view.py), one rounding"""
    with _quiet():
        return F(terms.astype(D).sum())


def literal_score(terms):
    """upstream's running fp32 sum in match order: term 1 then term 2 of a match"""
    with _quiet():
        return _seq_sum(terms.T.reshape(-1))


def select_first_max(scores):
    """-> (best index or -1, score): upstream's `currentScore > score` walk from 0"""
    best, score = -1, F(0)
    for h, s in enumerate(scores):
        if s > score:
            best, score = h, F(s)
    return best, score


# ---- CheckRT ----
def triangulate(P1, P2, pts):
    """Triangulate for all given matches -> (n, 3) fp32 (inf / NaN where the fourth component is 0)"""
    u1, v1, u2, v2 = pts
    n = len(u1)
    A = np.empty((n, 4, 4), F)
    for j in range(4):
        A[:, 0, j] = u1 * P1[2, j] - P1[0, j]
        A[:, 1, j] = v1 * P1[2, j] - P1[1, j]
        A[:, 2, j] = u2 * P2[2, j] - P2[0, j]
        A[:, 3, j] = v2 * P2[2, j] - P2[1, j]
    U, V = onesided(A.astype(D), SWEEPS4, 4)
    with _quiet():
        nk = np.stack([((U[:, 0, k] * U[:, 0, k] + U[:, 1, k] * U[:, 1, k]) + U[:, 2, k] * U[:, 2, k]) + U[:, 3, k] * U[:, 3, k]
                       for k in range(4)], 1)
        k = np.zeros(n, np.int64)
        best = nk[:, 0].copy()
        for j in range(1, 4):
            less = nk[:, j] < best
            best, k = np.where(less, nk[:, j], best), np.where(less, j, k)
        v = V[np.arange(n), :, k]
        return (v[:, :3] / v[:, 3:4]).astype(F)


def kth_smallest(c, k):
    """The value with at most k values below it and more than k not above it (no sort)"""
    for v in c:
        if (c < v).sum() <= k < (c <= v).sum():
            return F(v)
    return F(0)


def parallax_deg(c):
    with _quiet():
        return F(D(np.arccos(F(c)) * F(180)) / math.pi)


def check_rt(R, t, pts, inl, K, th2):
    """-> dict(n_good, good (N,) counted, tri (N,) vbGood, p3d (N, 3), cos (N,), cos_sel, parallax)"""
    fx, fy, cx, cy = (F(k) for k in K)
    R, t = np.asarray(R, F), np.asarray(t, F)
    u1, v1, u2, v2 = pts
    N = len(u1)
    P1 = np.array([[fx, 0, cx, 0], [0, fy, cy, 0], [0, 0, 1, 0]], F)
    Rt = np.concatenate([R, t[:, None]], 1)
    P2 = np.stack([fx * Rt[0] + cx * Rt[2], fy * Rt[1] + cy * Rt[2], Rt[2]])
    O2 = np.array([-((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) for i in range(3)], F)
    with _quiet():
        X = triangulate(P1, P2, pts)
        x, y, z = X[:, 0], X[:, 1], X[:, 2]
        ok = inl & np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        d1 = np.sqrt((x * x + y * y) + z * z)
        nx, ny, nz = x - O2[0], y - O2[1], z - O2[2]
        d2 = np.sqrt((nx * nx + ny * ny) + nz * nz)
        cosp = ((x * nx + y * ny) + z * nz) / (d1 * d2)
        ok &= ~((z <= 0) & (cosp < COS_LIMIT))
        X2 = np.stack([((R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z) + t[i] for i in range(3)], 1)
        ok &= ~((X2[:, 2] <= 0) & (cosp < COS_LIMIT))
        iz = F(1) / z
        ex, ey = ((fx * x) * iz + cx) - u1, ((fy * y) * iz + cy) - v1
        err1 = ex * ex + ey * ey
        ok &= ~(err1 > th2)
        iz = F(1) / X2[:, 2]
        ex, ey = ((fx * X2[:, 0]) * iz + cx) - u2, ((fy * X2[:, 1]) * iz + cy) - v2
        err2 = ex * ex + ey * ey
        ok &= ~(err2 > th2)
        tri = ok & (cosp < COS_LIMIT)
    n_good = int(ok.sum())
    cos_sel, par = F(0), F(0)
    if n_good > 0:
        c = cosp[ok]
        assert not np.isnan(c).any()
        cos_sel = kth_smallest(c, min(50, n_good - 1))
        assert cos_sel == np.sort(c)[min(50, n_good - 1)]
        par = parallax_deg(cos_sel)
    return dict(n_good=n_good, good=ok, tri=tri, p3d=X, cos=cosp, cos_sel=cos_sel, parallax=par, err1=err1, err2=err2)


# ---- the motion hypotheses ----
def _normalised(v):
    with _quiet():
        return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def motions_f(F21, K):
    """ReconstructF's four (R, t): E21 = K^T F21 K, DecomposeE"""
    fx, fy, cx, cy = (F(k) for k in K)
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
    E = mm3(mm3(Km.T.copy(), F21), Km)
    Q, _, W, _ = svd3(E.T.astype(D)[None])    # E^T = Q sig W^T: U of E = W, V of E = Q
    U, V = W[0].astype(F), Q[0].astype(F)
    t = _normalised(U[:, 2].copy())
    Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)
    Vt = V.T.copy()
    R1 = mm3(mm3(U, Wm), Vt)
    if det3(R1) < 0:
        R1 = -R1
    R2 = mm3(mm3(U, Wm.T.copy()), Vt)
    if det3(R2) < 0:
        R2 = -R2
    return [(R1, t), (R2, t), (R1, -t), (R2, -t)]


def motions_h(H21, K):
    """ReconstructH's eight (R, t), or [] at the d1/d2, d2/d3 exit -> (list, (d1, d2, d3))"""
    fx, fy, cx, cy = (F(k) for k in K)
    Km = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F)
    with _quiet():
        Ki = np.array([[F(1) / fx, 0, -cx / fx], [0, F(1) / fy, -cy / fy], [0, 0, 1]], F)
        A = mm3(mm3(Ki, H21), Km)
        Q, sig, W, _ = svd3(A.astype(D)[None])
        U, V, w = Q[0].astype(F), W[0].astype(F), sig[0].astype(F)
        Vt = V.T.copy()
        s = det3(U) * det3(Vt)
        d1, d2, d3 = w
        if d1 / d2 < F(1.00001) or d2 / d3 < F(1.00001):
            return [], (d1, d2, d3)
        den = d1 * d1 - d3 * d3
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / den)
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / den)
        x1 = [aux1, aux1, -aux1, -aux1]
        x3 = [aux3, -aux3, aux3, -aux3]
        prod = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3))
        ast = prod / ((d1 + d3) * d2)
        ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        st = [ast, -ast, -ast, ast]
        sU = s * U
        out = []
        for i in range(4):
            Rp = np.array([[ct, 0, -st[i]], [0, 1, 0], [st[i], 0, ct]], F)
            R = mm3(mm3(sU, Rp), Vt)
            tp = np.array([x1[i] * (d1 - d3), F(0), (-x3[i]) * (d1 - d3)], F)
            out.append((R, _normalised(mv3(U, tp))))
        asp = prod / ((d1 - d3) * d2)
        cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sp = [asp, -asp, -asp, asp]
        for i in range(4):
            Rp = np.array([[cp, 0, sp[i]], [0, -1, 0], [sp[i], 0, -cp]], F)
            R = mm3(mm3(sU, Rp), Vt)
            tp = np.array([x1[i] * (d1 + d3), F(0), x3[i] * (d1 + d3)], F)
            out.append((R, _normalised(mv3(U, tp))))
    return out, (d1, d2, d3)


def accept_f(n_good, parallax, n_inl):
    """-> chosen index or -1; margins (for the decision test) in the dict"""
    max_good = max(n_good[:4])
    n_min = max(int(0.9 * n_inl), MIN_TRIANGULATED)
    nsimilar = sum(1 for g in n_good[:4] if g > 0.7 * max_good)
    if max_good < n_min or nsimilar > 1:
        return -1
    k = [g for g in n_good[:4]].index(max_good)
    return k if parallax[k] > MIN_PARALLAX else -1


def accept_h(n_good, parallax, n_inl, n_mot):
    if n_mot == 0:
        return -1
    best = second = 0
    k, par = -1, F(-1)
    for i in range(8):
        if n_good[i] > best:
            second, best, k, par = best, n_good[i], i, parallax[i]
        elif n_good[i] > second:
            second = n_good[i]
    ok = second < 0.75 * best and par >= MIN_PARALLAX and best > MIN_TRIANGULATED and best > 0.9 * n_inl
    return k if ok else -1


# ---- the whole call ----
def match_list(matches12):
    m = np.asarray(matches12, np.int64)
    first = np.nonzero(m >= 0)[0]
    return first, m[first]


def inv_sigma2_of(sigma):
    return F(1.0 / D(F(sigma) * F(sigma)))


def prepare(p):
    first, second = match_list(p["matches12"])
    k1, k2 = np.asarray(p["kps1"], F), np.asarray(p["kps2"], F)
    pts = (k1[first, 0].copy(), k1[first, 1].copy(), k2[second, 0].copy(), k2[second, 1].copy())
    xn1, yn1, T1, _ = normalize(pts[0], pts[1])
    xn2, yn2, T2, T2i = normalize(pts[2], pts[3])
    return first, pts, (xn1, yn1, xn2, yn2), T1, T2, T2i


def ransac(p, literal=False, sweeps9=SWEEPS9, sweeps3=SWEEPS3):
    """Both models' hypotheses -> dict(first, pts, H21 (H, 3, 3), F21, scoreH (H,), scoreF, maskH
    (H, N), maskF); literal: the scores by upstream's running fp32 sum"""
    first, pts, pn, T1, T2, T2i = prepare(p)
    sets = np.asarray(p["sets"], np.int64).reshape(-1, 8)
    isg = inv_sigma2_of(p.get("sigma", 1.0))
    H21, H12 = compute_h21(pn, sets, T1, T2i, sweeps9)
    F21 = compute_f21(pn, sets, T1, T2, sweeps9, sweeps3)
    nh, N = len(sets), len(first)
    sH, sF = np.zeros(nh, F), np.zeros(nh, F)
    mH, mF = np.zeros((nh, N), bool), np.zeros((nh, N), bool)
    score = literal_score if literal else score_of
    for h in range(nh):
        th, mH[h] = homography_terms(H21[h], H12[h], pts, isg)
        tf, mF[h] = fundamental_terms(F21[h], pts, isg)
        sH[h], sF[h] = score(th), score(tf)
    return dict(first=first, pts=pts, H21=H21, F21=F21, scoreH=sH, scoreF=sF, maskH=mH, maskF=mF)


def reconstruct(p, literal=False, r=None):
    """What orbhip_two_view_reconstruct computes, as a dict of its outputs (masks and p3d by match:
    `first` maps a match to its keypoint in frame 1) plus the intermediate values the decision test
    reads."""
    r = ransac(p, literal) if r is None else r
    first, pts = r["first"], r["pts"]
    N, n1 = len(first), len(p["matches12"])
    K = np.asarray(p["K"], F)
    sg = F(p.get("sigma", 1.0))
    th2 = F(4) * (sg * sg)
    bh, SH = select_first_max(r["scoreH"])
    bf, SF = select_first_max(r["scoreF"])
    out = dict(success=0, model=-1, best_h=bh, best_f=bf, SH=SH, SF=SF,
               H21=r["H21"][bh] if bh >= 0 else np.zeros((3, 3), F),
               F21=r["F21"][bf] if bf >= 0 else np.zeros((3, 3), F),
               inl_h=r["maskH"][bh] if bh >= 0 else np.zeros(N, bool),
               inl_f=r["maskF"][bf] if bf >= 0 else np.zeros(N, bool),
               n_good=np.zeros(8, np.int32), parallax=np.zeros(8, F), cos_sel=np.zeros(8, F), chosen=-1,
               R21=np.zeros((3, 3), F), t21=np.zeros(3, F), p3d=np.zeros((n1, 3), F),
               triangulated=np.zeros(n1, bool), first=first, RH=F(np.nan), n_mot=0, n_inl=0, d=None)
    with _quiet():
        if SH + SF == 0:
            return out
        RH = SH / (SH + SF)
    out["RH"] = RH
    if RH > F(0.5):
        out["model"], inl = 0, out["inl_h"]
        mots, out["d"] = motions_h(out["H21"], K)
    else:
        out["model"], inl = 1, out["inl_f"]
        mots = motions_f(out["F21"], K)
    out["n_mot"], out["n_inl"] = len(mots), int(inl.sum())
    checks = [check_rt(R, t, pts, inl, K, th2) for R, t in mots]
    for i, c in enumerate(checks):
        out["n_good"][i], out["parallax"][i], out["cos_sel"][i] = c["n_good"], c["parallax"], c["cos_sel"]
    k = (accept_h(out["n_good"], out["parallax"], out["n_inl"], len(mots)) if out["model"] == 0
         else accept_f(out["n_good"], out["parallax"], out["n_inl"]))
    out["chosen"] = k
    out["checks"] = checks
    if k >= 0:
        c = checks[k]
        out["success"] = 1
        out["R21"], out["t21"] = mots[k][0], mots[k][1]
        out["p3d"][first[c["good"]]] = c["p3d"][c["good"]]
        out["triangulated"][first[c["tri"]]] = True
    return out


class LiteralSolver:
    """Upstream's Reconstruct with its sequential loop: one hypothesis after the other, the score a
    running fp32 sum in match order, `currentScore > score` from 0."""

    def __init__(self, p):
        self.p = p

    def Reconstruct(self):
        o = reconstruct(self.p, literal=True)
        T = np.eye(4, dtype=F)
        T[:3, :3], T[:3, 3] = o["R21"], o["t21"]
        return bool(o["success"]), T, o["p3d"], o["triangulated"], o


# ---- np.linalg.svd solutions (accuracy yardstick) ----
def svd_null(rows):
    return np.linalg.svd(np.asarray(rows, D))[2][-1]


def literal_draw_sets(N, H, randint):
    out = []
    for _ in range(H):
        avail = list(range(N))
        row = []
        for _ in range(8):
            r = randint(0, len(avail) - 1)
            row.append(avail[r])
            avail[r] = avail[-1]
            avail.pop()
        out.append(row)
    return np.array(out, np.int32)


@functools.lru_cache(maxsize=None)
def expected(name):
    """The restatement's result of a named scene of tests/two_view_cases.py (computed once, shared;
    treat as read-only) -> (problem, ransac dict, result dict)"""
    import two_view_cases as C
    p = C.scene(name)
    r = ransac(p)
    return p, r, reconstruct(p, r=r)
