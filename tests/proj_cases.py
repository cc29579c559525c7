"""Crafted scenes for the projection searches' routes and edges (tests/test_proj_routes*.py), and a
float32 numpy restatement of their window tests that counts candidates.

Every builder returns the dict of synthetic_projection_scene (so ProjFrame and both oracle calls
take it unchanged) plus the call's parameters ("th_last", "th_local", "nnratio") and, where the
result is known by construction, "expect".

Construction: the pose is the identity rotation with a translation; a target pixel is back-projected
in float64 at 4 m. The window radii in use are 15 px (LastFrame, th 15, octave 0), 100 px (the ties
case) and 2.5 * 1.2^3 = 4.32 px (local points, level 3): a keypoint meant to be inside a window lies
within 2 px of its target (within 50 px in the ties case), one meant to be outside at least two
radii away, so membership never depends on a last-bit rounding. Descriptors derive from one random
base by flipping the lowest bits, so distances are known exactly.
"""
import numpy as np

from orb_slam3_ros2_amd._lib import KP_DTYPE
from orb_slam3_ros2_amd.synthetic import D435I

f32 = np.float32
POSE_Q = np.array([0.0, 0.0, 0.0, 1.0], np.float32)
POSE_T = np.array([0.1, -0.2, 0.3], np.float64)
DEPTH = 4.0
LEVEL = 3                       # the level every crafted local point predicts: max_dist / dist = 1.2^2.5
TH_LAST, TH_LOCAL = 15.0, 1.0
# targets of independent query groups: 75 x 90 px apart, so windows of 15 px never meet
LATTICE = [(40.0 + 75.0 * a, 50.0 + 90.0 * b) for b in range(5) for a in range(8)]


def flip_low_bits(base, k):
    """`base` (32 bytes) with its k lowest bits flipped: Hamming distance exactly k."""
    mask = np.packbits(np.arange(256) < k, bitorder="little")
    return np.bitwise_xor(base, mask)


def _kps(xy, octave, angle=0.0):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
    k["octave"] = octave
    k["angle"] = angle
    k["size"] = 31.0
    k["response"] = 50.0
    return k


def _points(uv):
    """World points that project onto the pixels uv (n, 2) at DEPTH, and their isInFrustum
    members: the normal along the viewing ray, max_dist = dist * 1.2^2.5 (level 3, far from a
    step), min_dist = max_dist / 1.2^7."""
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    c = D435I
    Xc = np.stack([(uv[:, 0] - c["cx"]) / c["fx"] * DEPTH, (uv[:, 1] - c["cy"]) / c["fy"] * DEPTH,
                   np.full(len(uv), DEPTH)], 1)
    pts = Xc - POSE_T                      # identity rotation: Xc = P + t, Ow = -t
    dist = np.linalg.norm(Xc, axis=1)
    max_dist = dist * 1.2 ** 2.5
    return (pts.astype(np.float32), (Xc / dist[:, None]).astype(np.float32), (max_dist / 1.2 ** 7).astype(np.float32),
            max_dist.astype(np.float32))


def _scene(kps, desc, uv, mp_desc, last_octave=0, last_angle=10.0, claimed=None, **extra):
    pts, nrm, mind, maxd = _points(uv)
    nq = len(pts)
    c = D435I
    s = dict(kps=kps, desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), pose_q=POSE_Q.copy(),
             pose_t=POSE_T.astype(np.float32), fx=c["fx"], fy=c["fy"], cx=c["cx"], cy=c["cy"], points=pts,
             mp_desc=np.ascontiguousarray(mp_desc, np.uint8).reshape(-1, 32),
             last_octave=np.full(nq, last_octave, np.int32) if np.isscalar(last_octave) else
             np.asarray(last_octave, np.int32),
             last_angle=np.full(nq, last_angle, np.float32) if np.isscalar(last_angle) else
             np.asarray(last_angle, np.float32),
             normals=nrm, min_dist=mind, max_dist=maxd,
             claimed=np.zeros(len(kps), np.uint8) if claimed is None else np.asarray(claimed, np.uint8),
             skip=np.zeros(nq, np.uint8), src=None, th_last=TH_LAST, th_local=TH_LOCAL, nnratio=0.8)
    s.update(extra)
    return s


def _cluster(target, count, pitch=0.3):
    """`count` distinct positions within 2 px of `target` (a 12 x 12 lattice of pitch 0.3 px)."""
    assert count <= 144
    j = np.arange(count)
    return np.stack([target[0] + ((j % 12) - 5.5) * pitch, target[1] + ((j // 12) - 5.5) * pitch], 1)


def chain(K, mode="last", rot_outliers=()):
    """K queries and nothing else, all projecting to one pixel (one grid cell) with one descriptor
    B; keypoint j is B with flips[j] bits flipped. mode "last": flips[j] = j, octave 0, so query i
    must take keypoint i while i <= 100 = TH_HIGH and gets -1 beyond. mode "local": the same with
    the octaves alternating between level - 1 and level, so best and second best never share a level
    (no ratio test). mode "ratio" (K = 12): every keypoint on the level, distances 0 1 2 3 4 10 11 20
    30 50 80 100 and nnratio 0.8: queries 0..4 match, query 5 sees 10 against 11 and is rejected,
    and because a rejected query claims nothing every later query sees the same pair and is
    rejected too (a claim by query 5 would let query 6 match keypoint 6 at 11 against 20).
    rot_outliers: queries whose angle lies in another rotation bin (LastFrame, orientation check)."""
    rng = np.random.default_rng(100 + K)
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    target = (322.0, 242.0)              # cell (32, 24), its borders 3 px and more from every keypoint
    if mode == "ratio":
        flips = [0, 1, 2, 3, 4, 10, 11, 20, 30, 50, 80, 100]
        assert K == len(flips)
        octave = np.full(K, LEVEL)
        expect = np.array([0, 1, 2, 3, 4] + [-1] * 7, np.int32)
    else:
        flips = list(range(K))
        octave = np.where(np.arange(K) % 2 == 0, LEVEL - 1, LEVEL) if mode == "local" else np.zeros(K, int)
        expect = np.where(np.arange(K) <= 100, np.arange(K), -1).astype(np.int32)
    kps = _kps(_cluster(target, K), octave)
    desc = np.stack([flip_low_bits(B, f) for f in flips])
    ang = np.full(K, 10.0, np.float32)
    ang[list(rot_outliers)] = 100.0
    return _scene(kps, desc, [target] * K, np.tile(B, (K, 1)), last_angle=ang, expect=expect, K=K)


def ties(K=40):
    """K queries on one pixel, K keypoints with the queries' descriptor (distance 0 everywhere) in
    K different grid cells inside the common window (LastFrame, th 100: 100 px), their indices
    running against the cell order: query i must take the i-th keypoint in walk order (cell
    px * 48 + py, then index), which is keypoint K - 1 - i."""
    assert K == 40
    rng = np.random.default_rng(7)
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    cells = [(px, py) for px in range(28, 36) for py in range(20, 25)]     # walk order
    xy = np.array([(10.0 * px + 1.0, 10.0 * py + 1.0) for px, py in cells])[::-1]
    return _scene(_kps(xy, 0), np.tile(B, (K, 1)), [(320.0, 240.0)] * K, np.tile(B, (K, 1)), th_last=100.0,
                  expect=np.arange(K - 1, -1, -1).astype(np.int32), K=K)


def dense_rect(R):
    """One group of 44 queries on one pixel whose cell rectangle (cells 30..34 x 22..26) holds
    exactly R keypoints: 40 within 2 px of the target on octave 0 (a chain: distances 0..39), the
    others spread over the rectangle on octave 5, outside the queries' level window. 300 keypoints
    elsewhere; the index order is shuffled."""
    rng = np.random.default_rng(200 + R)
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    target = (322.0, 242.0)
    near = _cluster(target, 40)
    m = R - 40
    other = np.stack([rng.uniform(297.0, 343.0, m), rng.uniform(217.0, 263.0, m)], 1)
    far = np.stack([rng.uniform(20.0, 200.0, 300), rng.uniform(20.0, 460.0, 300)], 1)
    kps = np.concatenate([_kps(near, 0), _kps(other, 5), _kps(far, 0)])
    desc = np.concatenate([np.stack([flip_low_bits(B, j) for j in range(40)]),
                           rng.integers(0, 256, (m + 300, 32), dtype=np.uint8)])
    perm = rng.permutation(len(kps))
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    expect = np.concatenate([inv[:40], [-1] * 4]).astype(np.int32)
    return _scene(kps[perm], desc[perm], [target] * 44, np.tile(B, (44, 1)), expect=expect, R=R)


def list_count(C, claim_best=False):
    """Query 20 of 41 has exactly C keypoints passing every window test (within 2 px of its
    target, octave 0): random descriptors but two, at distances 3 and 7. The other 40 queries sit
    on the lattice with one keypoint each at distance 5. claim_best: the keypoint at distance 3 is
    claimed before the call, so it is filtered before the list (C - 1 entries) and the query takes
    the one at distance 7."""
    rng = np.random.default_rng(300 + C + 1000 * claim_best)
    A = (302.0, 277.0)                   # 37 px and more from every lattice target
    qd = rng.integers(0, 256, (41, 32), dtype=np.uint8)
    big = rng.integers(0, 256, (C, 32), dtype=np.uint8)
    best, second = C - 1, C // 2         # the best one is the last the wave lists
    big[best], big[second] = flip_low_bits(qd[20], 3), flip_low_bits(qd[20], 7)
    qi = [i for i in range(41) if i != 20]
    one = np.array(LATTICE) + 0.5
    kps = np.concatenate([_kps(one, 0), _kps(_cluster(A, C), 0)])
    desc = np.concatenate([np.stack([flip_low_bits(qd[i], 5) for i in qi]), big])
    uv = np.zeros((41, 2))
    uv[qi], uv[20] = np.array(LATTICE), A
    claimed = np.zeros(len(kps), np.uint8)
    expect = np.zeros(41, np.int32)
    expect[qi] = np.arange(40)
    expect[20] = 40 + (second if claim_best else best)
    if claim_best:
        claimed[40 + best] = 1
    return _scene(kps, desc, uv, qd, claimed=claimed, expect=expect, big_query=20, C=C)


RESOLVE_LDS = 150 * 1024


def ent_cap_of(n, nq):
    """The resolve's LDS entry capacity as csrc/proj_kernels.hip states it (the tests compare it
    with the route hook's)."""
    head = ((3 * n + 2 * nq + 1) * 4 + 15) & ~15
    return 0 if head >= RESOLVE_LDS else (RESOLVE_LDS - head) // 8


ENTRIES_N, ENTRIES_NQ = 8000, 6200


def entries(extra):
    """ent_cap_of(8000, 6200) + extra list entries in all. Groups on the lattice: full groups of 10
    queries x 10 keypoints (100 entries each; the queries chain), then one group of q queries x 10
    keypoints and one query with the remaining keypoints. The other keypoints lie 34 px and more
    from every target (x offset 37 +- 3 px in the targets' rows), the other queries project onto
    empty image between the rows (35 px and more from every keypoint)."""
    rng = np.random.default_rng(400)
    total = ent_cap_of(ENTRIES_N, ENTRIES_NQ) + extra
    groups, rem, t = [], total, 0
    while rem >= 100:
        groups.append((10, 10)); rem -= 100
    if rem >= 10:
        groups.append((rem // 10, 10)); rem -= 10 * (rem // 10)
    if rem:
        groups.append((1, rem))
    assert len(groups) <= len(LATTICE)
    kxy, kd, uv, qd = [], [], [], []
    for (q, c), target in zip(groups, LATTICE):
        d = rng.integers(0, 256, (c, 32), dtype=np.uint8)
        kxy.append(_cluster(target, c)); kd.append(d)
        uv += [target] * q
        qd.append(np.stack([flip_low_bits(d[i % c], 3) for i in range(q)]))
    n_used, q_used = sum(len(x) for x in kxy), len(uv)
    m = ENTRIES_N - n_used
    t = rng.integers(0, len(LATTICE), m)
    lat = np.array(LATTICE)
    kxy.append(np.stack([lat[t, 0] + 37.0 + rng.uniform(-3.0, 3.0, m), lat[t, 1] + rng.uniform(-10.0, 10.0, m)], 1))
    kd.append(rng.integers(0, 256, (m, 32), dtype=np.uint8))
    e = ENTRIES_NQ - q_used
    uv = np.concatenate([np.array(uv), np.stack([rng.uniform(20.0, 620.0, e),
                                                 95.0 + 90.0 * rng.integers(0, 5, e) + rng.uniform(-3.0, 3.0, e)], 1)])
    qd.append(rng.integers(0, 256, (e, 32), dtype=np.uint8))
    qperm = rng.permutation(ENTRIES_NQ)            # the groups' queries spread over the whole range
    return _scene(_kps(np.concatenate(kxy), 0), np.concatenate(kd), uv[qperm], np.concatenate(qd)[qperm],
                  total=total, ent_cap=total - extra)


def dist256():
    """Query 2 of 6: its only candidate carries the complemented descriptor (distance 256): the
    list holds an entry and there is no match. The others match their one keypoint at distance 5."""
    rng = np.random.default_rng(500)
    qd = rng.integers(0, 256, (6, 32), dtype=np.uint8)
    kd = np.stack([flip_low_bits(qd[i], 5) for i in range(6)])
    kd[2] = np.bitwise_not(qd[2])
    uv = np.array(LATTICE[:6])
    expect = np.arange(6, dtype=np.int32)
    expect[2] = -1
    return _scene(_kps(uv + 0.5, LEVEL), kd, uv, qd, last_octave=LEVEL, expect=expect)


STEP_LEVELS = 10   # a step of 1.2^7 needs a level 8 to land on: the frame of scale_steps has 10 levels


def scale_steps():
    """SearchLocalPoints at the steps of PredictScale: for k = 0..7 and j = -8..8 a point with
    max_dist = float32(dist64 * 1.2^k * (1 + j 2^-24)), dist64 the float32 distance the search
    computes, so max_dist / dist lies within a few ulps of the step 1.2^k on both sides of it. The
    frame has STEP_LEVELS = 10 levels so that the levels above the step at k = 7 are not clamped onto
    it. One keypoint under each projection (octave k)."""
    rng = np.random.default_rng(600)
    ks, js = np.meshgrid(np.arange(8), np.arange(-8, 9), indexing="ij")
    ks, js = ks.ravel(), js.ravel()
    nq = len(ks)
    uv = np.stack([30.0 + 34.0 * (np.arange(nq) % 17), 40.0 + 55.0 * (np.arange(nq) // 17)], 1)
    qd = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    s = _scene(_kps(uv + 0.5, ks), np.stack([flip_low_bits(d, 5) for d in qd]), uv, qd, k=ks, j=js)
    P = s["points"]
    Ow = -s["pose_t"]
    PO = [P[:, i] - Ow[i] for i in range(3)]
    dist = np.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2])
    assert dist.dtype == np.float32
    s["max_dist"] = (dist.astype(np.float64) * 1.2 ** ks * (1.0 + js * 2.0 ** -24)).astype(np.float32)
    s["min_dist"] = (s["max_dist"] / np.float32(8.0)).astype(np.float32)
    return s


# ---------------------------------------------------------------------------
# the window tests in float32 numpy (PosInGrid, the cell rectangle, the level window, |dx|, |dy| < r,
# claimed keypoints), operation for operation as oracle/proj_oracle.cpp
# ---------------------------------------------------------------------------

def _cround(x):
    x = np.asarray(x, np.float64)
    return np.sign(x) * np.floor(np.abs(x) + 0.5)


def _qrot(q, v):
    """Eigen _transformVector in float32; q = (x, y, z, w), v (n, 3)."""
    q = [f32(c) for c in q]
    v = [v[:, 0], v[:, 1], v[:, 2]]
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [a + a for a in uv]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return [v[i] + q[3] * uv[i] + c[i] for i in range(3)]


def windows_last(frame, points, last_octave, th):
    """(u, v, r, minL, maxL, valid) of SearchByProjection(CurrentFrame, LastFrame, th, bMono)."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    t = [f32(c) for c in frame.pose_t]
    X = _qrot(frame.pose_q, P)
    X = [X[i] + t[i] for i in range(3)]
    minx, maxx, miny, maxy = (f32(b) for b in frame.bounds)
    with np.errstate(all="ignore"):
        u = f32(frame.fx) * X[0] / X[2] + f32(frame.cx)
        v = f32(frame.fy) * X[1] / X[2] + f32(frame.cy)
        valid = ~((1.0 / X[2].astype(np.float64)).astype(np.float32) < 0)
    valid &= ~((u < minx) | (u > maxx) | (v < miny) | (v > maxy))
    lo = np.asarray(last_octave, np.int64)
    r = f32(th) * frame.scale_factors[lo]
    assert u.dtype == np.float32 and r.dtype == np.float32
    return u, v, r, lo - 1, lo + 1, valid


def windows_local(frame, points, normals, th, in_view, level):
    """The same for SearchByProjection(F, vpMapPoints, th) given isInFrustum's outputs (taken from
    the oracle: the level is not restated here)."""
    P = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    q = [f32(c) for c in frame.pose_q]
    t = [f32(c) for c in frame.pose_t]
    two = f32(2)
    tx, ty, tz = two * q[0], two * q[1], two * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    one = f32(1)
    R = [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx,
         one - (txx + tyy)]
    Pc = [R[3 * i] * P[:, 0] + R[3 * i + 1] * P[:, 1] + R[3 * i + 2] * P[:, 2] + t[i] for i in range(3)]
    Ow = _qrot([-q[0], -q[1], -q[2], q[3]], np.array([[t[0] * f32(-1), t[1] * f32(-1), t[2] * f32(-1)]], np.float32))
    PO = [P[:, i] - Ow[i][0] for i in range(3)]
    with np.errstate(all="ignore"):
        u = f32(frame.fx) * Pc[0] / Pc[2] + f32(frame.cx)
        v = f32(frame.fy) * Pc[1] / Pc[2] + f32(frame.cy)
        dist = np.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2])
        vcos = (PO[0] * N[:, 0] + PO[1] * N[:, 1] + PO[2] * N[:, 2]) / dist
    valid = np.asarray(in_view) == 1
    lvl = np.where(valid, level, 0).astype(np.int64)
    r = np.where(vcos.astype(np.float64) > 0.998, f32(2.5), f32(4.0)).astype(np.float32)
    if th != 1.0:
        r = r * f32(th)
    r = r * frame.scale_factors[lvl]
    assert u.dtype == np.float32 and r.dtype == np.float32
    return u, v, r, lvl - 1, lvl, valid


def window_counts(frame, win):
    """Per query: (keypoints with a cell inside the query's cell rectangle, keypoints passing every
    window test that are not claimed): k_proj_lists' rectangle count and list count."""
    u, v, r, minL, maxL, valid = win
    minx, maxx, miny, maxy = (f32(b) for b in frame.bounds)
    invw, invh = f32(64) / (maxx - minx), f32(48) / (maxy - miny)
    kx, ky, oct_ = frame.kps["x"], frame.kps["y"], frame.kps["octave"]
    px, py = _cround((kx - minx) * invw), _cround((ky - miny) * invh)
    on_grid = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    free = np.ones(len(kx), bool) if frame.claimed is None else frame.claimed[:len(kx)] == 0
    nq = len(u)
    rect, cand = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for i in np.nonzero(valid)[0]:
        x0 = max(0.0, float(np.floor((u[i] - minx - r[i]) * invw)))
        x1 = min(63.0, float(np.ceil((u[i] - minx + r[i]) * invw)))
        y0 = max(0.0, float(np.floor((v[i] - miny - r[i]) * invh)))
        y1 = min(47.0, float(np.ceil((v[i] - miny + r[i]) * invh)))
        if x0 >= 64 or x1 < 0 or y0 >= 48 or y1 < 0:
            continue
        inr = on_grid & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1)
        rect[i] = inr.sum()
        ok = inr
        if minL[i] > 0 or maxL[i] >= 0:
            ok = ok & ~(oct_ < minL[i]) & ~((maxL[i] >= 0) & (oct_ > maxL[i]))
        ok = ok & (np.abs(kx - u[i]) < r[i]) & (np.abs(ky - v[i]) < r[i]) & free
        cand[i] = ok.sum()
    return rect, cand


def counts_last(s, frame, th=None):
    return window_counts(frame, windows_last(frame, s["points"], s["last_octave"], s.get("th_last", TH_LAST) if th is None else th))
