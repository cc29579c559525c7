"""Test infrastructure: the restatement of the triangulation of U:src/LocalMapping.cc::
CreateNewMapPoints (monocular, one pinhole camera per keyframe) that DESIGN.md "CreateNewMapPoints"
writes down. The fp32 part is explicit np.float32 scalar operations, one IEEE operation each in the
order the library performs them; the fp64 Jacobi runs on Python floats (IEEE double: +, -, *, / and
math.sqrt are correctly rounded, as fp64 is on the device), so the library's results can be compared
bit for bit. Not used by the product.

Status codes: 0 no match, 1 accepted, 2 cosParallax <= 0, 3 parallax too low, 4 null vector with
w == 0, 5 / 6 not in front of KF1 / KF2, 7 / 8 reprojection error in KF1 / KF2, 9 on a camera centre,
10 beyond the far threshold, 11 scale ratio."""
import math

import numpy as np

import triangulation_numpy as T

f32 = np.float32
f64 = np.float64
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
SWEEPS = 6


class Camera:
    """R (row-major list of 9), t, Ow (lists of 3) and the intrinsics of a keyframe, all np.float32."""

    def __init__(self, kf):
        self.R = T._rot(kf.pose_q)
        self.t = [f32(v) for v in kf.pose_t]
        R, t = self.R, self.t
        self.Ow = [-((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]) for i in range(3)]
        self.fx, self.fy, self.cx, self.cy = f32(kf.fx), f32(kf.fy), f32(kf.cx), f32(kf.cy)


def gated(cam1, cam2, median_depth):
    """The baseline gate of one neighbour."""
    with np.errstate(all="ignore"):
        d = [cam2.Ow[i] - cam1.Ow[i] for i in range(3)]
        baseline = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        r = baseline / f32(median_depth)
        return bool(f64(r) < f64(0.01))


def system(cam1, cam2, xn1, xn2):
    """A (4 x 4 nested list of np.float32)."""
    rows = []
    for cam, xn in ((cam1, xn1), (cam2, xn2)):
        Tm = [[cam.R[3 * i + j] for j in range(3)] + [cam.t[i]] for i in range(3)]
        rows.append([xn[0] * Tm[2][j] - Tm[0][j] for j in range(4)])
        rows.append([xn[1] * Tm[2][j] - Tm[1][j] for j in range(4)])
    return rows


def null_vector(A, sweeps=SWEEPS):
    """The fp64 one-sided Jacobi: V's column of least |U column|^2 (ties: the lowest), as 4 Python floats."""
    U = [[float(A[i][j]) for j in range(4)] for i in range(4)]
    V = [[1.0 if i == j else 0.0 for j in range(4)] for i in range(4)]
    for _ in range(sweeps):
        for p, q in PAIRS:
            a = ((U[0][p] * U[0][p] + U[1][p] * U[1][p]) + U[2][p] * U[2][p]) + U[3][p] * U[3][p]
            b = ((U[0][q] * U[0][q] + U[1][q] * U[1][q]) + U[2][q] * U[2][q]) + U[3][q] * U[3][q]
            g = ((U[0][p] * U[0][q] + U[1][p] * U[1][q]) + U[2][p] * U[2][q]) + U[3][p] * U[3][q]
            if g == 0.0:
                continue
            zeta = (b - a) / (2.0 * g)
            t = 1.0 / (abs(zeta) + math.sqrt(1.0 + zeta * zeta))
            if zeta < 0.0:
                t = -t
            c = 1.0 / math.sqrt(1.0 + t * t)
            s = c * t
            for M in (U, V):
                for i in range(4):
                    x, y = M[i][p], M[i][q]
                    M[i][p] = c * x - s * y
                    M[i][q] = s * x + c * y
    k, best = 0, ((U[0][0] * U[0][0] + U[1][0] * U[1][0]) + U[2][0] * U[2][0]) + U[3][0] * U[3][0]
    for j in range(1, 4):
        nj = ((U[0][j] * U[0][j] + U[1][j] * U[1][j]) + U[2][j] * U[2][j]) + U[3][j] * U[3][j]
        if nj < best:
            k, best = j, nj
    return [V[i][k] for i in range(4)]


def _mul3(row, X, t):
    return ((row[0] * X[0] + row[1] * X[1]) + row[2] * X[2]) + t


def triangulate_pair(cam1, cam2, kp1, kp2, scale_factors, level_sigma2, cos_max=0.9998, ratio_factor=None,
                     far=0.0, detail=None):
    """(status, x3D (3,) float32; zeros when the point was not reached). kp1 / kp2: records with x, y,
    octave. detail: a dict that receives cosP, A, v (the null vector before the division), dist1."""
    sf = np.asarray(scale_factors, f32)
    s2 = np.asarray(level_sigma2, f32)
    ratio_factor = f32(1.5) * sf[1] if ratio_factor is None else f32(ratio_factor)
    far = f32(far)
    zero = np.zeros(3, f32)
    with np.errstate(all="ignore"):
        u1, v1, o1 = f32(kp1["x"]), f32(kp1["y"]), int(kp1["octave"])
        u2, v2, o2 = f32(kp2["x"]), f32(kp2["y"]), int(kp2["octave"])
        xn1 = ((u1 - cam1.cx) / cam1.fx, (v1 - cam1.cy) / cam1.fy)
        xn2 = ((u2 - cam2.cx) / cam2.fx, (v2 - cam2.cy) / cam2.fy)
        r1 = [(cam1.R[i] * xn1[0] + cam1.R[3 + i] * xn1[1]) + cam1.R[6 + i] for i in range(3)]
        r2 = [(cam2.R[i] * xn2[0] + cam2.R[3 + i] * xn2[1]) + cam2.R[6 + i] for i in range(3)]
        dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2]
        nn1 = (r1[0] * r1[0] + r1[1] * r1[1]) + r1[2] * r1[2]
        nn2 = (r2[0] * r2[0] + r2[1] * r2[1]) + r2[2] * r2[2]
        cosP = dot / (np.sqrt(nn1) * np.sqrt(nn2))
        if detail is not None:
            detail["cosP"] = cosP
        if not (cosP > f32(0)):
            return 2, zero
        if not (f64(cosP) < f64(cos_max)):
            return 3, zero
        A = system(cam1, cam2, xn1, xn2)
        v = null_vector(A)
        if detail is not None:
            detail["A"], detail["v"] = A, v
        if v[3] == 0.0:
            return 4, zero
        X = [f32(v[i] / v[3]) for i in range(3)]
        x3d = np.array(X, f32)
        z1 = _mul3(cam1.R[6:9], X, cam1.t[2])
        if z1 <= f32(0):
            return 5, x3d
        z2 = _mul3(cam2.R[6:9], X, cam2.t[2])
        if z2 <= f32(0):
            return 6, x3d
        for code, cam, z, u, v_, o in ((7, cam1, z1, u1, v1, o1), (8, cam2, z2, u2, v2, o2)):
            px = _mul3(cam.R[0:3], X, cam.t[0])
            py = _mul3(cam.R[3:6], X, cam.t[1])
            e = ((cam.fx * px) / z + cam.cx) - u
            f = ((cam.fy * py) / z + cam.cy) - v_
            if f64(e * e + f * f) > f64(5.991) * f64(s2[o]):
                return code, x3d
        d1 = [X[i] - cam1.Ow[i] for i in range(3)]
        d2 = [X[i] - cam2.Ow[i] for i in range(3)]
        dist1 = np.sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2])
        dist2 = np.sqrt((d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2])
        if detail is not None:
            detail["dist1"] = dist1
        if dist1 == f32(0) or dist2 == f32(0):
            return 9, x3d
        if far > f32(0) and (dist1 >= far or dist2 >= far):
            return 10, x3d
        ratio_dist = dist2 / dist1
        ratio_octave = sf[o1] / sf[o2]
        if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
            return 11, x3d
        return 1, x3d


class Result:
    pass


def triangulate_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max=0.9998, ratio_factor=None,
                        far=0.0, details=None):
    """status (B, n1) uint8 and x3d_all (B, n1, 3) float32 of given matches; details: a list that
    receives (b, idx1, detail dict) of every matched pair."""
    B, n1 = len(neighbours), kf1.n
    status = np.zeros((B, n1), np.uint8)
    x3d = np.zeros((B, n1, 3), f32)
    cam1 = Camera(kf1)
    for b, kf2 in enumerate(neighbours):
        row = match12[b]
        if not (row >= 0).any():
            continue
        cam2 = Camera(kf2)
        for idx1 in np.nonzero(row >= 0)[0]:
            det = {} if details is not None else None
            status[b, idx1], x3d[b, idx1] = triangulate_pair(cam1, cam2, kf1.kps[idx1], kf2.kps[row[idx1]],
                                                             scale_factors, level_sigma2, cos_max, ratio_factor, far,
                                                             det)
            if details is not None:
                details.append((b, int(idx1), det))
    return status, x3d


def claim(status, match12, x3d_all):
    """first (n1,), nnew (B,), and the list (nbr, idx1, idx2, x3d) in (neighbour, idx1) order."""
    B, n1 = status.shape
    ok = status == 1
    first = np.where(ok.any(0), ok.argmax(0), -1).astype(np.int32) if B else np.full(n1, -1, np.int32)
    nnew = np.array([(first == b).sum() for b in range(B)], np.int32)
    nbr, idx1 = [], []
    for b in range(B):
        for i in np.nonzero(first == b)[0]:
            nbr.append(b); idx1.append(int(i))
    nbr = np.array(nbr, np.int32); idx1 = np.array(idx1, np.int32)
    idx2 = match12[nbr, idx1].astype(np.int32) if nbr.size else np.zeros(0, np.int32)
    x3d = x3d_all[nbr, idx1] if nbr.size else np.zeros((0, 3), f32)
    return first, nnew, nbr, idx1, idx2, x3d


def _finish(r, status, x3d_all, match12, nmatches, gate):
    r.status, r.x3d_all, r.match12 = status, x3d_all, match12
    r.nmatches, r.gated = np.asarray(nmatches, np.int32), np.asarray(gate, np.uint8)
    r.first, r.nnew, r.new_nbr, r.new_idx1, r.new_idx2, r.new_x3d = claim(status, match12, x3d_all)
    r.n = int(r.new_nbr.size)
    return r


def create_new_map_points(kf1, neighbours, scale_factors, level_sigma2, check_orientation, median_depth=None,
                          cos_max=0.9998, ratio_factor=None, far=0.0, geoms=None, details=None):
    """The batched rule: gate, search (tests/triangulation_numpy.py) and triangulate every neighbour
    as it is at call time, then claim. geoms: per neighbour (F12, ep) for the search or None."""
    B, n1 = len(neighbours), kf1.n
    cam1 = Camera(kf1)
    gate = [median_depth is not None and gated(cam1, Camera(k), median_depth[b]) for b, k in enumerate(neighbours)]
    match12 = np.full((B, n1), -1, np.int32)
    nmatches = np.zeros(B, np.int32)
    for b, kf2 in enumerate(neighbours):
        if gate[b]:
            continue
        F, ep = geoms[b] if geoms is not None else (None, None)
        nmatches[b], match12[b], _ = T.search_pair(kf1, kf2, scale_factors, level_sigma2, check_orientation, F, ep)
    status, x3d_all = triangulate_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max,
                                          ratio_factor, far, details)
    return _finish(Result(), status, x3d_all, match12, nmatches, gate)


def from_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max=0.9998, ratio_factor=None, far=0.0):
    """orbhip_triangulate_matches: no search, no gating."""
    match12 = np.asarray(match12, np.int32)
    status, x3d_all = triangulate_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max,
                                          ratio_factor, far)
    return _finish(Result(), status, x3d_all, match12, (match12 >= 0).sum(1), np.zeros(len(neighbours), np.uint8))


def sequential(kf1, neighbours, scale_factors, level_sigma2, check_orientation, median_depth=None, cos_max=0.9998,
               ratio_factor=None, far=0.0):
    """Upstream's loop in plain Python: neighbour after neighbour, search with KF1's MapPoints as they
    are by then, triangulate, give every accepted feature a MapPoint, go on. Returns the list
    (nbr, idx1, idx2, x3d) in creation order."""
    import copy
    k1 = copy.copy(kf1)
    k1.has_mp = np.array(kf1.has_mp, np.uint8).copy()
    cam1 = Camera(kf1)
    nbr, idx1s, idx2s, pts = [], [], [], []
    for b, kf2 in enumerate(neighbours):
        cam2 = Camera(kf2)
        if median_depth is not None and gated(cam1, cam2, median_depth[b]):
            continue
        _, m, _ = T.search_pair(k1, kf2, scale_factors, level_sigma2, check_orientation)
        for idx1 in np.nonzero(m >= 0)[0]:
            st, X = triangulate_pair(cam1, cam2, k1.kps[idx1], kf2.kps[m[idx1]], scale_factors, level_sigma2, cos_max,
                                     ratio_factor, far)
            if st == 1:
                k1.has_mp[idx1] = 1
                nbr.append(b); idx1s.append(int(idx1)); idx2s.append(int(m[idx1])); pts.append(X)
    return (np.array(nbr, np.int32), np.array(idx1s, np.int32), np.array(idx2s, np.int32),
            np.array(pts, f32).reshape(-1, 3))
