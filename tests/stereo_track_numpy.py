"""numpy restatement of the rectified-stereo tracking calls: Optimizer::PoseOptimization with
EdgeStereoSE3ProjectXYZOnlyPose edges mixed with monocular ones (fp64), and the stereo branches of
SearchByProjection(CurrentFrame, LastFrame, th, bMono = false) and Tracking::SearchLocalPoints
(float32 semantics, every operation in the order the reference writes it).

With u_right all -1 the three functions are the monocular rules of oracle/ba_oracle.cpp and
oracle/proj_oracle.cpp; tests/test_stereo_track.py pins them to the oracle there before the device
is compared with them.
"""
import math

import numpy as np

from helpers import HISTO_LENGTH, rotation_bin, three_maxima

F32 = np.float32
CHI2_MONO, CHI2_STEREO = float(F32(5.991)), float(F32(7.815))
DELTA_MONO, DELTA_STEREO = float(F32(np.sqrt(5.991))), float(F32(np.sqrt(7.815)))


# ------------------------------------------------------------------ SE3 (g2o SE3Quat, fp64)
def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _qrot(q, v):
    """Eigen _transformVector; v (..., 3)."""
    u = q[:3]
    uv = np.cross(u, v)
    uv = uv + uv
    return v + q[3] * uv + np.cross(u, uv)


def _normalize(q):
    if q[3] < 0:
        q = -q
    return q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])


def _mat_to_q(m):
    m = m.reshape(9)
    t = m[0] + m[4] + m[8]
    if t > 0:
        t = np.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        return np.array([(m[7] - m[5]) * t, (m[2] - m[6]) * t, (m[3] - m[1]) * t, w])
    i = 0
    if m[4] > m[0]:
        i = 1
    if m[8] > m[3 * i + i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0)
    c = np.zeros(3)
    c[i] = 0.5 * t
    t = 0.5 / t
    w = (m[3 * k + j] - m[3 * j + k]) * t
    c[j] = (m[3 * j + i] + m[3 * i + j]) * t
    c[k] = (m[3 * k + i] + m[3 * i + k]) * t
    return np.array([c[0], c[1], c[2], w])


def _se3_exp(u):
    ox, oy, oz = u[0], u[1], u[2]
    theta = float(np.sqrt(ox * ox + oy * oy + oz * oz))
    O = np.array([[0, -oz, oy], [oz, 0, -ox], [-oy, ox, 0]])
    O2 = np.zeros((3, 3))                # (explicit loops: a BLAS product may fuse multiply-adds)
    for r in range(3):
        for c in range(3):
            s = 0.0
            for k in range(3):
                s += O[r, k] * O[k, c]
            O2[r, c] = s
    I = np.eye(3)
    if theta < 0.00001:
        R = I + O + O2
        V = R
    else:
        # (libm's sin / cos / pow, as the oracle calls them)
        a, b = math.sin(theta) / theta, (1 - math.cos(theta)) / (theta * theta)
        c = (theta - math.sin(theta)) / math.pow(theta, 3)
        R = I + a * O + b * O2
        V = I + b * O + c * O2
    t = np.array([V[r, 0] * u[3] + V[r, 1] * u[4] + V[r, 2] * u[5] for r in range(3)])
    return _normalize(_mat_to_q(R)), t


def _se3_mul(a, b):
    return _normalize(_qmul(a[0], b[0])), a[1] + _qrot(a[0], b[1])


def _ldlt_solve(S, b):
    n = len(b)
    S = S.copy()
    d = np.zeros(n)
    for j in range(n):
        dj = S[j, j]
        for k in range(j):
            dj -= S[j, k] * S[j, k] * d[k]
        if dj == 0.0 or not np.isfinite(dj):
            return None
        d[j] = dj
        for i in range(j + 1, n):
            s = S[i, j]
            for k in range(j):
                s -= S[i, k] * S[j, k] * d[k]
            S[i, j] = s / dj
    x = b.copy()
    for i in range(n):
        for k in range(i):
            x[i] -= S[i, k] * x[k]
    x /= d
    for i in range(n - 1, -1, -1):
        for k in range(i + 1, n):
            x[i] -= S[k, i] * x[k]
    return x


def _seq_sum(a):
    """Sum over axis 0 in index order (the oracle's loop), not numpy's pairwise order."""
    return np.cumsum(a, axis=0)[-1] if a.shape[0] else np.zeros(a.shape[1:])


# ------------------------------------------------------------------ PoseOptimization
class _Edges:
    def __init__(self, p):
        n = p.points.shape[0]
        self.n = n
        self.X = p.points.astype(np.float64)
        self.u, self.v = p.uv[:, 0].astype(np.float64), p.uv[:, 1].astype(np.float64)
        self.info = p.inv_sigma2[p.octave].astype(np.float64)
        ur = np.full(n, -1.0, F32) if p.u_right is None else p.u_right
        self.stereo = ur >= 0            # upstream's monocular branch tests mvuRight[i] < 0: 0.0f is stereo
        self.ur = ur.astype(np.float64)
        self.fx, self.fy, self.cx, self.cy = (float(F32(v)) for v in (p.fx, p.fy, p.cx, p.cy))
        self.bf = float(F32(p.bf))
        self.delta = np.where(self.stereo, DELTA_STEREO, DELTA_MONO)
        self.th = np.where(self.stereo, CHI2_STEREO, CHI2_MONO)

    def error(self, T, idx):
        """(e (m, 3), chi2 (m,), Xc (m, 3)) of the edges idx at the pose T."""
        Xc = _qrot(T[0], self.X[idx]) + T[1]
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        st = self.stereo[idx]
        with np.errstate(all="ignore"):
            pu = self.fx * x / z + self.cx
            e0 = self.u[idx] - pu
            e1 = self.v[idx] - (self.fy * y / z + self.cy)
            e2 = np.where(st, self.ur[idx] - (pu - self.bf / z), 0.0)
            chi2 = self.info[idx] * (e0 * e0 + e1 * e1 + e2 * e2)
        return np.stack([e0, e1, e2], 1), chi2, Xc

    def jacobian(self, Xc, st):
        """(m, 3, 6): a monocular edge as the oracle forms it, -projectJac(Xc) [-Xc^ | I]; a stereo
        edge by EdgeStereoSE3ProjectXYZOnlyPose::linearizeOplus' closed form."""
        x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
        m = len(x)
        fx, fy, bf = self.fx, self.fy, self.bf
        zero, one = np.zeros(m), np.ones(m)
        with np.errstate(all="ignore"):
            J = np.stack([np.stack([-(fx / z), -zero, -(-fx * x / (z * z))], 1),
                          np.stack([-zero, -(fy / z), -(-fy * y / (z * z))], 1)], 1)        # (m, 2, 3)
            D = np.stack([np.stack([zero, z, -y, one, zero, zero], 1), np.stack([-z, zero, x, zero, one, zero], 1),
                          np.stack([y, -x, zero, zero, zero, one], 1)], 1)                   # (m, 3, 6)
            B = np.zeros((m, 3, 6))
            for r in range(2):
                for c in range(6):
                    B[:, r, c] = J[:, r, 0] * D[:, 0, c] + J[:, r, 1] * D[:, 1, c] + J[:, r, 2] * D[:, 2, c]
            iz = 1.0 / z
            iz2 = iz * iz
            S = np.zeros((m, 3, 6))
            S[:, 0] = np.stack([x * y * iz2 * fx, -(1 + x * x * iz2) * fx, y * iz * fx, -iz * fx, zero, x * iz2 * fx], 1)
            S[:, 1] = np.stack([(1 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * iz * fy, zero, -iz * fy, y * iz2 * fy], 1)
            S[:, 2] = np.stack([S[:, 0, 0] - bf * y * iz2, S[:, 0, 1] + bf * x * iz2, S[:, 0, 2], S[:, 0, 3], zero,
                                S[:, 0, 5] - bf * iz2], 1)
        return np.where(st[:, None, None], S, B)


def _robustify(chi2, delta, robust):
    rho0, rho1 = chi2.copy(), np.ones_like(chi2)
    if robust:
        with np.errstate(all="ignore"):
            big = chi2 > delta * delta
            sq = np.sqrt(np.where(big, chi2, 1.0))
            rho0 = np.where(big, 2 * sq * delta - delta * delta, rho0)
            rho1 = np.where(big, delta / sq, rho1)
    return rho0, rho1


def _optimize(E, T, level, robust, chi2_last, iterations=10):
    """g2o optimize(iterations) on the level-0 edges; returns (T, trials)."""
    act = np.nonzero(level == 0)[0]
    trials = 0
    if act.size == 0:
        return T, trials
    delta, info, st = E.delta[act], E.info[act], E.stereo[act]

    def errors(Tc):
        _, c2, _ = E.error(Tc, act)
        chi2_last[act] = c2
        return float(_seq_sum(_robustify(c2, delta, robust)[0]))

    lam, ni = 0.0, 2.0
    for it in range(iterations):
        current = errors(T)
        e, c2, Xc = E.error(T, act)
        _, r1 = _robustify(c2, delta, robust)
        B = E.jacobian(Xc, st)
        w = r1 * info
        with np.errstate(all="ignore"):
            om = -info[:, None] * e * r1[:, None]                                          # (m, 3)
            Hk = B[:, 0, :, None] * B[:, 0, None, :] + B[:, 1, :, None] * B[:, 1, None, :]
            Hk = np.where(st[:, None, None], Hk + B[:, 2, :, None] * B[:, 2, None, :], Hk)
            bk = B[:, 0] * om[:, 0, None] + B[:, 1] * om[:, 1, None]
            bk = np.where(st[:, None], bk + B[:, 2] * om[:, 2, None], bk)
            H = _seq_sum(w[:, None, None] * Hk)
            b = _seq_sum(bk)
        if it == 0:
            md = 0.0
            for j in range(6):
                if md < abs(H[j, j]):    # std::max(md, fabs(H[jj]))
                    md = abs(H[j, j])
            lam = 1e-5 * md
            ni = 2.0
        rho, qmax = 0.0, 0
        while True:
            Tbak = T
            x = _ldlt_solve(H + lam * np.eye(6), b)
            ok = x is not None
            if not ok:
                x = np.zeros(6)
            T = _se3_mul(_se3_exp(x), T)
            temp = errors(T)
            if not ok:
                temp = np.finfo(np.float64).max
            scale = 1e-3
            for j in range(6):
                scale += x[j] * (lam * x[j] + b[j])
            with np.errstate(all="ignore"):
                rho = (current - temp) / scale
            if rho > 0 and np.isfinite(temp):
                alpha = min(1.0 - math.pow(2 * rho - 1, 3), 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                current = temp
            else:
                lam *= ni
                ni *= 2
                T = Tbak
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        if qmax == 10 or rho == 0:
            break
    return T, trials


def pose_optimization(prob):
    """Optimizer::PoseOptimization of an optimizer.PoseProblem (u_right None: all monocular).
    Returns dict(pose_q, pose_t (float32), outlier, n_inliers, lm_trials)."""
    p = prob.normalized()
    E = _Edges(p)
    n = E.n
    T0 = (_normalize(p.pose_q.astype(np.float64)), p.pose_t.astype(np.float64))
    outlier = np.zeros(n, np.uint8)
    trials = 0
    T = T0
    if n < 3:
        return dict(pose_q=T0[0].astype(F32), pose_t=T0[1].astype(F32), outlier=outlier, n_inliers=0, lm_trials=0)
    level = np.zeros(n, np.uint8)
    chi2_last = np.zeros(n)
    robust = True
    nbad = 0
    for it in range(4):
        T, tr = _optimize(E, T0, level, robust, chi2_last)
        trials += tr
        out = np.nonzero(outlier)[0]
        if out.size:                     # level-1 edges: computeError() at the current estimate
            chi2_last[out] = E.error(T, out)[1]
        with np.errstate(invalid="ignore"):
            bad = chi2_last > E.th
        outlier = bad.astype(np.uint8)
        level = outlier.copy()
        nbad = int(bad.sum())
        if it == 2:
            robust = False
        if n < 10:
            break
    return dict(pose_q=T[0].astype(F32), pose_t=T[1].astype(F32), outlier=outlier, n_inliers=n - nbad,
                lm_trials=trials)


# ------------------------------------------------------------------ the frame grid (float32)
COLS, ROWS, TH_HIGH = 64, 48, 100
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def _round_half_away(v):
    """std::round of non-negative-or-not float32 values, exactly (in float64)."""
    v = v.astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def _qrot32(q, v):
    """Eigen _transformVector in float32; v (m, 3)."""
    q = q.astype(F32)
    v = v.astype(F32)

    def cross(a, b):
        return np.stack([a[1] * b[:, 2] - a[2] * b[:, 1], a[2] * b[:, 0] - a[0] * b[:, 2],
                         a[0] * b[:, 1] - a[1] * b[:, 0]], 1)
    uv = cross(q, v)
    uv = uv + uv
    c = cross(q, uv)
    return v + q[3] * uv + c


def _qtomat32(q):
    x, y, z, w = (F32(a) for a in q)
    two = F32(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = F32(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], F32)


class _Grid:
    def __init__(self, frame):
        self.kps = frame.kps
        self.n = self.kps.shape[0]
        self.x, self.y = self.kps["x"].astype(F32), self.kps["y"].astype(F32)
        self.oct = self.kps["octave"].astype(np.int64)
        self.minx, self.maxx, self.miny, self.maxy = (F32(b) for b in frame.bounds)
        self.invw = F32(COLS) / (self.maxx - self.minx)
        self.invh = F32(ROWS) / (self.maxy - self.miny)
        px = _round_half_away((self.x - self.minx) * self.invw)
        py = _round_half_away((self.y - self.miny) * self.invh)
        self.px, self.py = px, py
        self.ingrid = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
        self.key = (px * ROWS + py) * 65536 + np.arange(self.n)      # the walk order of GetFeaturesInArea

    def area(self, u, v, r, min_level, max_level):
        """GetFeaturesInArea(u, v, r, minLevel, maxLevel): keypoint indices in walk order."""
        if self.n == 0:
            return np.zeros(0, np.int64)
        x0 = max(0, int(np.floor((u - self.minx - r) * self.invw)))
        x1 = min(COLS - 1, int(np.ceil((u - self.minx + r) * self.invw)))
        y0 = max(0, int(np.floor((v - self.miny - r) * self.invh)))
        y1 = min(ROWS - 1, int(np.ceil((v - self.miny + r) * self.invh)))
        if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
            return np.zeros(0, np.int64)
        ok = self.ingrid & (self.px >= x0) & (self.px <= x1) & (self.py >= y0) & (self.py <= y1)
        if min_level > 0 or max_level >= 0:
            ok &= self.oct >= min_level
            if max_level >= 0:
                ok &= self.oct <= max_level
        ok &= (np.abs(self.x - u) < r) & (np.abs(self.y - v) < r)
        idx = np.nonzero(ok)[0]
        return idx[np.argsort(self.key[idx], kind="stable")]


def _hamming(d, D):
    return _POP[np.bitwise_xor(D, d[None, :])].sum(1)


def direction(frame, last_pose, b):
    """1 forward (tlc.z > b), -1 backward (-tlc.z > b), 0 neither; (dir, tlc.z)."""
    Rc, Rl = _qtomat32(frame.pose_q), _qtomat32(last_pose[0])
    t = np.asarray(frame.pose_t, F32)
    tl = np.asarray(last_pose[1], F32)
    twc = [-(Rc[0, j] * t[0] + Rc[1, j] * t[1] + Rc[2, j] * t[2]) for j in range(3)]
    z = Rl[2, 0] * twc[0] + Rl[2, 1] * twc[1] + Rl[2, 2] * twc[2] + tl[2]
    return (1 if z > F32(b) else (-1 if -z > F32(b) else 0)), float(z)


def search_by_projection_last(frame, points, mp_desc, last_octave, last_angle, th=15.0, check_orientation=True,
                              u_right=None, bf=0.0, b=0.0, last_pose=None, stats=None):
    """SearchByProjection(CurrentFrame, LastFrame, th, bMono = false). u_right (per keypoint) /
    bf / b / last_pose default to the frame's; last_pose = (q, t) of the last frame. stats (a dict)
    receives gated = the (query, candidate) pairs the stereo gate alone rejected.
    Returns (nmatches, match, direction)."""
    u_right = frame.u_right if u_right is None else u_right
    bf = F32(bf if bf else frame.bf)
    b = b if b else frame.b
    G = _Grid(frame)
    ur_k = np.asarray(u_right, F32)
    pts = np.ascontiguousarray(points, F32).reshape(-1, 3)
    nq = pts.shape[0]
    desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
    kd = frame.desc
    fx, fy, cx, cy = (F32(a) for a in (frame.fx, frame.fy, frame.cx, frame.cy))
    th = F32(th)
    dirn, _ = direction(frame, last_pose, b)
    taken = np.zeros(G.n, bool) if frame.claimed is None else frame.claimed[:G.n].astype(bool).copy()
    match = np.full(nq, -1, np.int32)
    bins = np.full(nq, -1)
    hist = np.zeros(HISTO_LENGTH, np.int64)
    Xc = _qrot32(np.asarray(frame.pose_q, F32), pts) + np.asarray(frame.pose_t, F32)
    gated = 0
    for i in range(nq):
        xc, yc, zc = Xc[i]
        with np.errstate(all="ignore"):
            invzc = F32(1.0 / np.float64(zc))
            if invzc < 0:
                continue
            u, v = fx * xc / zc + cx, fy * yc / zc + cy
        if u < G.minx or u > G.maxx or v < G.miny or v > G.maxy:
            continue
        lo = int(last_octave[i])
        radius = th * frame.scale_factors[lo]
        if dirn > 0:
            cand = G.area(u, v, radius, lo, -1)
        elif dirn < 0:
            cand = G.area(u, v, radius, 0, lo)
        else:
            cand = G.area(u, v, radius, lo - 1, lo + 1)
        cand = cand[~taken[cand]]
        if cand.size:
            ur = u - bf * invzc
            urc = ur_k[cand]
            rej = (urc > 0) & (np.abs(ur - urc) > radius)
            gated += int(rej.sum())
            cand = cand[~rej]
        if cand.size == 0:
            continue
        d = _hamming(desc[i], kd[cand])
        j = int(np.argmin(d))            # strict <: the first of equal distances in walk order
        if d[j] < 256 and d[j] <= TH_HIGH:
            k = int(cand[j])
            taken[k] = True
            match[i] = k
            if check_orientation:
                bb = rotation_bin(last_angle[i], G.kps["angle"][k])
                bins[i] = bb
                hist[bb] += 1
    if check_orientation:
        keep = three_maxima(hist)
        for i in range(nq):
            if match[i] >= 0 and bins[i] not in keep:
                match[i] = -1
    if stats is not None:
        stats["gated"] = gated
    return int((match >= 0).sum()), match, dirn


def search_local_points(frame, points, normals, min_dist, max_dist, mp_desc, skip=None, th=1.0, nnratio=0.8,
                        view_cos_limit=0.5, far_points=False, th_far=0.0, u_right=None, bf=0.0, stats=None):
    """Frame::isInFrustum (with mTrackProjXR) + SearchByProjection(F, vpMapPoints, th, bFarPoints,
    thFarPoints) with the stereo gate. Returns (nmatches, match, in_view, level, proj_xr); proj_xr is
    NaN where not in view."""
    u_right = frame.u_right if u_right is None else u_right
    bf = F32(bf if bf else frame.bf)
    G = _Grid(frame)
    ur_k = np.asarray(u_right, F32)
    P = np.ascontiguousarray(points, F32).reshape(-1, 3)
    m = P.shape[0]
    N = np.ascontiguousarray(normals, F32).reshape(-1, 3)
    mind, maxd = np.asarray(min_dist, F32), np.asarray(max_dist, F32)
    desc = np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32)
    kd = frame.desc
    fx, fy, cx, cy = (F32(a) for a in (frame.fx, frame.fy, frame.cx, frame.cy))
    q = np.asarray(frame.pose_q, F32)
    t = np.asarray(frame.pose_t, F32)
    R = _qtomat32(q)
    Ow = _qrot32(np.array([-q[0], -q[1], -q[2], q[3]], F32), (t * F32(-1.0))[None, :])[0]
    log_sf = F32(frame.log_scale_factor)
    n_levels = len(frame.scale_factors)
    match = np.full(m, -1, np.int32)
    in_view = np.zeros(m, np.uint8)
    level = np.full(m, -1, np.int32)
    proj_xr = np.full(m, np.nan, F32)
    pu, pv, vcos, depth = np.zeros(m, F32), np.zeros(m, F32), np.zeros(m, F32), np.zeros(m, F32)
    with np.errstate(all="ignore"):
        for i in range(m):
            if skip is not None and skip[i]:
                continue
            p = P[i]
            Pc = [R[r, 0] * p[0] + R[r, 1] * p[1] + R[r, 2] * p[2] + t[r] for r in range(3)]
            Pc_dist = np.sqrt(Pc[0] * Pc[0] + Pc[1] * Pc[1] + Pc[2] * Pc[2])
            if Pc[2] < F32(0.0):
                continue
            u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
            if u < G.minx or u > G.maxx:
                continue
            if v < G.miny or v > G.maxy:
                continue
            PO = p - Ow
            dist = np.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2])
            if dist < F32(0.8) * mind[i] or dist > F32(1.2) * maxd[i]:
                continue
            vc = (PO[0] * N[i, 0] + PO[1] * N[i, 1] + PO[2] * N[i, 2]) / dist
            if vc < F32(view_cos_limit):
                continue
            ratio = maxd[i] / dist
            ns = int(np.ceil(F32(np.log(np.float64(ratio))) / log_sf))
            ns = 0 if ns < 0 else (n_levels - 1 if ns >= n_levels else ns)
            in_view[i], level[i] = 1, ns
            pu[i], pv[i], vcos[i], depth[i] = u, v, vc, Pc_dist
            invz = F32(1.0) / Pc[2]
            proj_xr[i] = u - bf * invz
    taken = np.zeros(G.n, bool) if frame.claimed is None else frame.claimed[:G.n].astype(bool).copy()
    th32 = F32(th)
    nn = F32(nnratio)
    gated = 0
    for i in range(m):
        if not in_view[i]:
            continue
        if far_points and depth[i] > F32(th_far):
            continue
        lv = int(level[i])
        r = F32(2.5) if np.float64(vcos[i]) > 0.998 else F32(4.0)
        if th != 1.0:
            r = r * th32
        radius = r * frame.scale_factors[lv]
        cand = G.area(pu[i], pv[i], radius, lv - 1, lv)
        cand = cand[~taken[cand]]
        if cand.size:
            urc = ur_k[cand]
            rej = (urc > 0) & (np.abs(proj_xr[i] - urc) > radius)
            gated += int(rej.sum())
            cand = cand[~rej]
        if cand.size == 0:
            continue
        best, best2, lvl1, lvl2, bi = 256, 256, -1, -1, -1
        for k, d in zip(cand.tolist(), _hamming(desc[i], kd[cand]).tolist()):
            if d < best:
                best2, best, lvl2, lvl1, bi = best, d, lvl1, int(G.oct[k]), k
            elif d < best2:
                lvl2, best2 = int(G.oct[k]), d
        if best <= TH_HIGH:
            if lvl1 == lvl2 and F32(best) > nn * F32(best2):
                continue
            if lvl1 != lvl2 or F32(best) <= nn * F32(best2):
                taken[bi] = True
                match[i] = bi
    if stats is not None:
        stats["gated"] = gated
    return int((match >= 0).sum()), match, in_view, level, proj_xr
