"""Test infrastructure: the stereo branches of U:src/ORBmatcher.cc::SearchForTriangulation
(bOnlyStereo = false, bCoarse = false) and of U:src/LocalMapping.cc::CreateNewMapPoints as DESIGN.md
"Stereo LocalMapping" writes them down. Only the changed steps are restated here (fp32 in explicit
np.float32 scalars, fp64 in Python floats); the geometry, the 4x4 system, the Jacobi, the claim and
the counters' meaning are those of tests/triangulation_numpy.py and tests/create_points_numpy.py,
imported. Not used by the product.

Keyframes are orb_slam3_ros2_amd.matcher.TriKeyFrame objects that carry u_right (mvuRight; >= 0: a
stereo feature), depth (mvDepth), bf (mbf) and b (mb).
Status 12: a feature chosen for UnprojectStereo has depth <= 0 (or NaN). source: 0 no point, 1
triangulated, 2 / 3 unprojected from KF1 / the neighbour."""
import numpy as np

import create_points_numpy as C
import triangulation_numpy as T

f32 = np.float32
f64 = np.float64


def stereo_cos(b, d):
    """Decision 4: cos(2 atan2(b / 2, d)) as (D^2 - h^2) / (D^2 + h^2) in fp64, each operation rounded
    once, then rounded once to fp32."""
    with np.errstate(all="ignore"):
        h = float(f32(b)) * 0.5
        D = float(f32(d))
        DD, hh = f64(D * D), f64(h * h)
        return f32((DD - hh) / (DD + hh))


def is_stereo(ur) -> bool:
    return bool(f32(ur) >= f32(0))


# ---- SearchForTriangulation: the epipole exclusion only when neither feature is stereo ----
def search_pair(kf1, kf2, scale_factors, level_sigma2, check_orientation, F12=None, ep=None):
    """triangulation_numpy.search_pair with the one changed gate. counters as there, plus
    `epipole_radius`: candidates inside the epipole radius that the stereo rule let through (they may
    still fail the epipolar-line gate), and `epi_matches`: final matches inside the radius."""
    if F12 is None or ep is None:
        F12, ep = T.geometry(kf1, kf2)
    F = np.asarray(F12, f32).reshape(3, 3)
    ex, ey = f32(ep[0]), f32(ep[1])
    sf = np.asarray(scale_factors, f32)
    s2 = np.asarray(level_sigma2, f32)
    n1 = kf1.n
    match = np.full(n1, -1, np.int32)
    cnt = dict(epipole=0, epiline=0, ties=0, shared=0, pruned=0, epipole_radius=0, epi_matches=0)
    fv1, fv2 = T._feature_vector(kf1), T._feature_vector(kf2)
    d2all = np.asarray(kf2.desc, np.uint8).reshape(-1, 32)
    rot_hist = [[] for _ in range(T.HISTO_LENGTH)]
    with np.errstate(all="ignore"):
        for node in sorted(set(fv1) & set(fv2)):
            cand = np.array(fv2[node], np.int64)
            for idx1 in fv1[node]:
                if kf1.has_mp[idx1]:
                    continue
                stereo1 = is_stereo(kf1.u_right[idx1])
                dists = T._POP[np.bitwise_xor(d2all[cand], np.asarray(kf1.desc[idx1], np.uint8).reshape(1, 32))].sum(1)
                x1, y1 = f32(kf1.kps["x"][idx1]), f32(kf1.kps["y"][idx1])
                a = (x1 * F[0, 0] + y1 * F[1, 0]) + F[2, 0]
                b = (x1 * F[0, 1] + y1 * F[1, 1]) + F[2, 1]
                c = (x1 * F[0, 2] + y1 * F[1, 2]) + F[2, 2]
                den = a * a + b * b
                best_dist, best_idx2, best_inside = T.TH_LOW, -1, False
                for k, idx2 in enumerate(cand):
                    idx2 = int(idx2)
                    if kf2.has_mp[idx2]:
                        continue
                    dist = int(dists[k])
                    if dist > T.TH_LOW or dist > best_dist:
                        continue
                    x2, y2 = f32(kf2.kps["x"][idx2]), f32(kf2.kps["y"][idx2])
                    o2 = int(kf2.kps["octave"][idx2])
                    dex, dey = ex - x2, ey - y2
                    inside = bool(dex * dex + dey * dey < f32(100) * sf[o2])
                    if inside:
                        if not (stereo1 or is_stereo(kf2.u_right[idx2])):      # the changed gate
                            cnt["epipole"] += 1
                            continue
                        cnt["epipole_radius"] += 1
                    num = (a * x2 + b * y2) + c
                    if den == f32(0):
                        cnt["epiline"] += 1
                        continue
                    dsqr = (num * num) / den
                    if not (f64(dsqr) < f64(3.84) * f64(s2[o2])):
                        cnt["epiline"] += 1
                        continue
                    if best_idx2 >= 0 and dist == best_dist:
                        cnt["ties"] += 1
                    best_idx2, best_dist, best_inside = idx2, dist, inside
                if best_idx2 >= 0:
                    match[idx1] = best_idx2
                    cnt["epi_matches"] += best_inside
                    if check_orientation:
                        bin_ = T.rotation_bin(kf1.kps["angle"][idx1], kf2.kps["angle"][best_idx2])
                        rot_hist[bin_].append(idx1)
    targets = match[match >= 0]
    cnt["shared"] = int((np.bincount(targets, minlength=1) > 1).sum()) if targets.size else 0
    if check_orientation:
        keep = T.three_maxima([len(h) for h in rot_hist])
        for i in range(T.HISTO_LENGTH):
            if i not in keep:
                for idx1 in rot_hist[i]:
                    match[idx1] = -1
                    cnt["pruned"] += 1
    return int((match >= 0).sum()), match, cnt


def search_for_triangulation(kf1, neighbours, scale_factors, level_sigma2, check_orientation, geoms=None):
    nm, rows, per = [], [], []
    for b, kf2 in enumerate(neighbours):
        F, ep = geoms[b] if geoms is not None else (None, None)
        n, m, c = search_pair(kf1, kf2, scale_factors, level_sigma2, check_orientation, F, ep)
        nm.append(n); rows.append(m); per.append(c)
    m12 = np.stack(rows) if rows else np.zeros((0, kf1.n), np.int32)
    return np.array(nm, np.int32), m12, per


# ---- CreateNewMapPoints ----
def gated(cam1, cam2, b_nbr):
    """The per-neighbour gate: baseline < the neighbour's mb (fp32)."""
    with np.errstate(all="ignore"):
        d = [cam2.Ow[i] - cam1.Ow[i] for i in range(3)]
        baseline = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        return bool(baseline < f32(b_nbr))


def unproject(cam, kp, z):
    """KeyFrame::UnprojectStereo for a depth z > 0."""
    u, v = f32(kp["x"]), f32(kp["y"])
    x = ((u - cam.cx) * z) * (f32(1.0) / cam.fx)
    y = ((v - cam.cy) * z) * (f32(1.0) / cam.fy)
    return [((cam.R[j] * x + cam.R[3 + j] * y) + cam.R[6 + j] * z) + cam.Ow[j] for j in range(3)]


def feature(kf, i):
    """(ur, depth, bf, b) of feature i."""
    return f32(kf.u_right[i]), f32(kf.depth[i]), f32(kf.bf), f32(kf.b)


MONO = (f32(-1), f32(0), f32(0), f32(0))


def triangulate_pair(cam1, cam2, kp1, kp2, f1, f2, scale_factors, level_sigma2, cos_max=0.9998, ratio_factor=None,
                     far=0.0, detail=None):
    """(status, x3D (3,) float32, source). f1 / f2: feature() of the two features. detail: a dict that
    receives cosP, cosS1, cosS2 and mono7 / mono8 (whether the monocular reprojection test of that
    image would have passed, where the stereo one was applied)."""
    sf = np.asarray(scale_factors, f32)
    s2 = np.asarray(level_sigma2, f32)
    ratio_factor = f32(1.5) * sf[1] if ratio_factor is None else f32(ratio_factor)
    far = f32(far)
    zero = np.zeros(3, f32)
    ur1, dep1, bf1, b1 = f1
    ur2, dep2, bf2, b2 = f2
    st1, st2 = is_stereo(ur1), is_stereo(ur2)
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
        # step 2: only one of the two is replaced (upstream's else-if)
        cosS1 = cosS2 = cosP + f32(1.0)
        if st1:
            cosS1 = stereo_cos(b1, dep1)
        elif st2:
            cosS2 = stereo_cos(b2, dep2)
        cosS = cosS2 if cosS2 < cosS1 else cosS1
        if detail is not None:
            detail.update(cosP=cosP, cosS1=cosS1, cosS2=cosS2)
        # step 4
        if cosP < cosS and cosP > f32(0) and (st1 or st2 or f64(cosP) < f64(cos_max)):
            source = 1
            v = C.null_vector(C.system(cam1, cam2, xn1, xn2))
            if v[3] == 0.0:
                return 4, zero, source
            X = [f32(v[i] / v[3]) for i in range(3)]
        elif st1 and cosS1 < cosS2:
            source = 2
            if not (dep1 > f32(0)):
                return 12, zero, source
            X = unproject(cam1, kp1, dep1)
        elif st2 and cosS2 < cosS1:
            source = 3
            if not (dep2 > f32(0)):
                return 12, zero, source
            X = unproject(cam2, kp2, dep2)
        else:
            return (2 if not (cosP > f32(0)) else 3), zero, 0
        x3d = np.array(X, f32)
        z1 = C._mul3(cam1.R[6:9], X, cam1.t[2])
        if z1 <= f32(0):
            return 5, x3d, source
        z2 = C._mul3(cam2.R[6:9], X, cam2.t[2])
        if z2 <= f32(0):
            return 6, x3d, source
        for code, cam, z, u, v_, o, st, ur, bf in ((7, cam1, z1, u1, v1, o1, st1, ur1, bf1),
                                                   (8, cam2, z2, u2, v2, o2, st2, ur2, bf2)):
            px = C._mul3(cam.R[0:3], X, cam.t[0])
            py = C._mul3(cam.R[3:6], X, cam.t[1])
            e = ((cam.fx * px) / z + cam.cx) - u
            f = ((cam.fy * py) / z + cam.cy) - v_
            mono_ok = not f64(e * e + f * f) > f64(5.991) * f64(s2[o])
            if st:
                invz = f32(1.0) / z
                pu = ((cam.fx * px) * invz) + cam.cx
                pv = ((cam.fy * py) * invz) + cam.cy
                pr = pu - bf * invz
                eX, eY, eR = pu - u, pv - v_, pr - ur
                if f64((eX * eX + eY * eY) + eR * eR) > f64(7.8) * f64(s2[o]):
                    if detail is not None:
                        detail["mono%d" % code] = mono_ok
                    return code, x3d, source
            elif not mono_ok:
                return code, x3d, source
        d1 = [X[i] - cam1.Ow[i] for i in range(3)]
        d2 = [X[i] - cam2.Ow[i] for i in range(3)]
        dist1 = np.sqrt((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2])
        dist2 = np.sqrt((d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2])
        if dist1 == f32(0) or dist2 == f32(0):
            return 9, x3d, source
        if far > f32(0) and (dist1 >= far or dist2 >= far):
            return 10, x3d, source
        ratio_dist = dist2 / dist1
        ratio_octave = sf[o1] / sf[o2]
        if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
            return 11, x3d, source
        return 1, x3d, source


def triangulate_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max=0.9998, ratio_factor=None,
                        far=0.0, details=None):
    """status, x3d_all, source of given matches; details: a list receiving (b, idx1, detail dict)."""
    B, n1 = len(neighbours), kf1.n
    status = np.zeros((B, n1), np.uint8)
    source = np.zeros((B, n1), np.uint8)
    x3d = np.zeros((B, n1, 3), f32)
    cam1 = C.Camera(kf1)
    for b, kf2 in enumerate(neighbours):
        row = match12[b]
        if not (row >= 0).any():
            continue
        cam2 = C.Camera(kf2)
        for idx1 in np.nonzero(row >= 0)[0]:
            det = {} if details is not None else None
            status[b, idx1], x3d[b, idx1], source[b, idx1] = triangulate_pair(
                cam1, cam2, kf1.kps[idx1], kf2.kps[row[idx1]], feature(kf1, idx1), feature(kf2, row[idx1]),
                scale_factors, level_sigma2, cos_max, ratio_factor, far, det)
            if details is not None:
                details.append((b, int(idx1), det))
    return status, x3d, source


def create_new_map_points(kf1, neighbours, scale_factors, level_sigma2, check_orientation, cos_max=0.9998,
                          ratio_factor=None, far=0.0, geoms=None, details=None, counters=None):
    """The batched stereo rule: the mb gate, the stereo search, the pairs, then create_points_numpy's
    claim. counters: a list that receives the search's per-pair counters (None for a gated neighbour)."""
    B, n1 = len(neighbours), kf1.n
    cam1 = C.Camera(kf1)
    gate = [gated(cam1, C.Camera(k), k.b) for k in neighbours]
    match12 = np.full((B, n1), -1, np.int32)
    nmatches = np.zeros(B, np.int32)
    for b, kf2 in enumerate(neighbours):
        if gate[b]:
            if counters is not None:
                counters.append(None)
            continue
        F, ep = geoms[b] if geoms is not None else (None, None)
        nmatches[b], match12[b], c = search_pair(kf1, kf2, scale_factors, level_sigma2, check_orientation, F, ep)
        if counters is not None:
            counters.append(c)
    status, x3d_all, source = triangulate_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max,
                                                  ratio_factor, far, details)
    r = C._finish(C.Result(), status, x3d_all, match12, nmatches, gate)
    r.source = source
    return r


def from_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max=0.9998, ratio_factor=None, far=0.0):
    """orbhip_triangulate_matches_stereo: no search, no gating."""
    match12 = np.asarray(match12, np.int32)
    status, x3d_all, source = triangulate_matches(kf1, neighbours, match12, scale_factors, level_sigma2, cos_max,
                                                  ratio_factor, far)
    r = C._finish(C.Result(), status, x3d_all, match12, (match12 >= 0).sum(1), np.zeros(len(neighbours), np.uint8))
    r.source = source
    return r


def sequential(kf1, neighbours, scale_factors, level_sigma2, check_orientation, cos_max=0.9998, ratio_factor=None,
               far=0.0):
    """Upstream's loop under the stereo rule: neighbour after neighbour, search with KF1's MapPoints as
    they are by then, make the points, give every accepted feature a MapPoint, go on."""
    import copy
    k1 = copy.copy(kf1)
    k1.has_mp = np.array(kf1.has_mp, np.uint8).copy()
    cam1 = C.Camera(kf1)
    nbr, idx1s, idx2s, pts = [], [], [], []
    for b, kf2 in enumerate(neighbours):
        cam2 = C.Camera(kf2)
        if gated(cam1, cam2, kf2.b):
            continue
        _, m, _ = search_pair(k1, kf2, scale_factors, level_sigma2, check_orientation)
        for idx1 in np.nonzero(m >= 0)[0]:
            st, X, _ = triangulate_pair(cam1, cam2, k1.kps[idx1], kf2.kps[m[idx1]], feature(k1, idx1),
                                        feature(kf2, m[idx1]), scale_factors, level_sigma2, cos_max, ratio_factor, far)
            if st == 1:
                k1.has_mp[idx1] = 1
                nbr.append(b); idx1s.append(int(idx1)); idx2s.append(int(m[idx1])); pts.append(X)
    return (np.array(nbr, np.int32), np.array(idx1s, np.int32), np.array(idx2s, np.int32),
            np.array(pts, f32).reshape(-1, 3))


def with_stereo(kf, u_right, depth, bf, b):
    """A copy of TriKeyFrame `kf` (sharing its arrays) that carries the stereo members."""
    from orb_slam3_ros2_amd.matcher import TriKeyFrame
    return TriKeyFrame(kf.kps, kf.desc, kf.node, kf.weight, kf.has_mp, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx,
                       kf.cy, u_right=u_right, depth=depth, bf=bf, b=b)


def without_stereo(kf):
    """The same keyframe without its stereo members."""
    from orb_slam3_ros2_amd.matcher import TriKeyFrame
    return TriKeyFrame(kf.kps, kf.desc, kf.node, kf.weight, kf.has_mp, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy)


def all_mono(kf, bf=30.0, b=1e-6):
    """`kf` as a stereo keyframe without a stereo feature and with a baseline below every gate."""
    n = kf.n
    return with_stereo(kf, np.full(n, -1.0, f32), np.full(n, -1.0, f32), bf, b)
