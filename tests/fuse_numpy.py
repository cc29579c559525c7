"""Test infrastructure: the restatement of U:src/ORBmatcher.cc::Fuse(KeyFrame* pKF, const
vector<MapPoint*>& vpMapPoints, const float th, bRight = false) (monocular, one pinhole camera,
mvKeysUn) that DESIGN.md writes down, in explicit np.float32 scalar operations: every product, sum,
quotient and comparison is one IEEE operation in the order the library performs it (no `@`, no dot:
BLAS may fuse), one function per step of the rule, and the candidate walk in the reference's order
(ix outer, iy inner, ascending index inside a cell, strict <). Not used by the product.

Keyframes are objects with the attributes of orb_slam3_ros2_amd.matcher.ProjFrame."""
import numpy as np

f32 = np.float32
TH_LOW = 50
COLS, ROWS = 64, 48
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)

# how many pairs each gate rejected (skip .. th_low), how many were accepted, how many candidates the
# two candidate gates dropped, and the ties: a later candidate of the winner's distance in another
# cell (decided by cell order) / in the winner's cell (decided by index)
# (no_window, an early return of GetFeaturesInArea, cannot fire inside Fuse: step 3 has already put
# (u, v) inside the bounds the grid spans, so with r > 0 the rectangle always meets the grid; the
# restatement keeps the branch because the reference has it)
COUNTERS = ("skip", "pair_skip", "behind", "outside", "dist_low", "dist_high", "angle", "no_window", "no_candidate",
            "th_low", "accepted", "cand_level_low", "cand_level_high", "cand_chi2", "tie_cell", "tie_index")
GATE_COUNTERS = tuple(k for k in COUNTERS if k != "no_window")


def roundf(v) -> int:
    """C roundf: halves away from zero (np.round rounds them to even)."""
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def qrot(q, v):
    """Eigen QuaternionBase::_transformVector in fp32."""
    q = [f32(x) for x in q]
    v = [f32(x) for x in v]
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [x + x for x in uv]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return [(v[i] + q[3] * uv[i]) + c[i] for i in range(3)]


class Grid:
    """A keyframe as Fuse reads it: Tcw, mOw, the intrinsics, the image bounds and the 64 x 48 grid
    (KeyFrame ctor: AssignFeaturesToGrid with PosInGrid's round)."""

    def __init__(self, kf):
        self.q = [f32(v) for v in kf.pose_q]
        self.t = [f32(v) for v in kf.pose_t]
        self.Ow = qrot([-self.q[0], -self.q[1], -self.q[2], self.q[3]], [v * f32(-1.0) for v in self.t])
        self.fx, self.fy, self.cx, self.cy = f32(kf.fx), f32(kf.fy), f32(kf.cx), f32(kf.cy)
        self.minx, self.maxx, self.miny, self.maxy = (f32(b) for b in kf.bounds)
        with np.errstate(all="ignore"):
            self.invw = f32(COLS) / (self.maxx - self.minx)
            self.invh = f32(ROWS) / (self.maxy - self.miny)
        self.x = np.asarray(kf.kps["x"], f32)
        self.y = np.asarray(kf.kps["y"], f32)
        self.octave = np.asarray(kf.kps["octave"], np.int64)
        self.desc = np.asarray(kf.desc, np.uint8).reshape(-1, 32)
        self.sf = np.asarray(kf.scale_factors, f32)
        self.n_levels = len(self.sf)
        self.log_sf = f32(kf.log_scale_factor)
        self.cells = {}
        for i in range(self.x.shape[0]):
            px = roundf((self.x[i] - self.minx) * self.invw)
            py = roundf((self.y[i] - self.miny) * self.invh)
            if 0 <= px < COLS and 0 <= py < ROWS:
                self.cells.setdefault((px, py), []).append(i)


def step1_camera(g, P):
    """Pc = Tcw * P (quaternion form)."""
    r = qrot(g.q, P)
    return [r[0] + g.t[0], r[1] + g.t[1], r[2] + g.t[2]]


def step2_project(g, Pc):
    return (g.fx * Pc[0]) / Pc[2] + g.cx, (g.fy * Pc[1]) / Pc[2] + g.cy


def step3_in_image(g, u, v):
    """KeyFrame::IsInImage: the maximum is strict."""
    return bool(u >= g.minx and u < g.maxx and v >= g.miny and v < g.maxy)


def step4_distance(g, P):
    PO = [f32(P[0]) - g.Ow[0], f32(P[1]) - g.Ow[1], f32(P[2]) - g.Ow[2]]
    return PO, np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2])


def step5_view_ok(PO, Pn, dist3D):
    Pn = [f32(x) for x in Pn]
    return not ((PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2] < f32(0.5) * dist3D)


def step6_level(g, max_dist, dist3D):
    """MapPoint::PredictScale."""
    x = np.ceil(np.log(f32(max_dist) / dist3D) / g.log_sf)
    if not x > 0:
        return 0
    return g.n_levels - 1 if x >= g.n_levels else int(x)


def step7_radius(g, th, lvl):
    return f32(th) * g.sf[lvl]


def step8_rectangle(g, u, v, r):
    """The cell rectangle of KeyFrame::GetFeaturesInArea, None at one of its early returns."""
    x0 = max(0, int(np.floor((u - g.minx - r) * g.invw)))
    if x0 >= COLS:
        return None
    x1 = min(COLS - 1, int(np.ceil((u - g.minx + r) * g.invw)))
    if x1 < 0:
        return None
    y0 = max(0, int(np.floor((v - g.miny - r) * g.invh)))
    if y0 >= ROWS:
        return None
    y1 = min(ROWS - 1, int(np.ceil((v - g.miny + r) * g.invh)))
    if y1 < 0:
        return None
    return x0, x1, y0, y1


def step8_area(g, u, v, r):
    """GetFeaturesInArea(u, v, r): [(cell, idx)] in walk order; None at an early return."""
    rect = step8_rectangle(g, u, v, r)
    if rect is None:
        return None
    x0, x1, y0, y1 = rect
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for j in g.cells.get((ix, iy), ()):
                dx, dy = g.x[j] - u, g.y[j] - v
                if abs(dx) < r and abs(dy) < r:
                    out.append((ix * ROWS + iy, j))
    return out


def step9_walk(g, cand, u, v, lvl, desc, inv_s2, cnt):
    """The candidate loop. Returns (bestDist, bestIdx)."""
    best_dist, best_idx, best_cell = 256, -1, -1
    d = np.asarray(desc, np.uint8).reshape(32)
    for cell, idx in cand:
        o = int(g.octave[idx])
        if o < lvl - 1:
            cnt["cand_level_low"] += 1
            continue
        if o > lvl:
            cnt["cand_level_high"] += 1
            continue
        ex, ey = u - g.x[idx], v - g.y[idx]
        e2 = ex * ex + ey * ey
        if np.float64(e2 * inv_s2[o]) > 5.99:
            cnt["cand_chi2"] += 1
            continue
        dist = int(_POP[np.bitwise_xor(g.desc[idx], d)].sum())
        if dist < best_dist:
            best_dist, best_idx, best_cell = dist, idx, cell
        elif dist == best_dist:
            cnt["tie_cell" if cell != best_cell else "tie_index"] += 1
    return best_dist, best_idx


def fuse_pair(g, P, Pn, min_dist, max_dist, desc, inv_s2, th, cnt):
    """One (keyframe, MapPoint) pair that is not skipped: (best_idx, best_dist, level)."""
    with np.errstate(all="ignore"):
        P = [f32(x) for x in P]
        Pc = step1_camera(g, P)
        if Pc[2] < f32(0.0):
            cnt["behind"] += 1
            return -1, 256, -1
        u, v = step2_project(g, Pc)
        if not step3_in_image(g, u, v):
            cnt["outside"] += 1
            return -1, 256, -1
        PO, dist3D = step4_distance(g, P)
        if dist3D < f32(0.8) * f32(min_dist):
            cnt["dist_low"] += 1
            return -1, 256, -1
        if dist3D > f32(1.2) * f32(max_dist):
            cnt["dist_high"] += 1
            return -1, 256, -1
        if not step5_view_ok(PO, Pn, dist3D):
            cnt["angle"] += 1
            return -1, 256, -1
        lvl = step6_level(g, max_dist, dist3D)
        r = step7_radius(g, th, lvl)
        cand = step8_area(g, u, v, r)
        if cand is None:
            cnt["no_window"] += 1
            return -1, 256, lvl
        best_dist, best_idx = step9_walk(g, cand, u, v, lvl, desc, inv_s2, cnt)
        if best_idx < 0:
            cnt["no_candidate"] += 1
            return -1, 256, lvl
        if best_dist <= TH_LOW:      # step 10
            cnt["accepted"] += 1
            return best_idx, best_dist, lvl
        cnt["th_low"] += 1
        return -1, best_dist, lvl


def level_ratio64(g, P, max_dist):
    """log(max_dist / dist3D) / log_scale_factor in float64, from the fp32 dist3D of step 4."""
    with np.errstate(all="ignore"):
        _, dist3D = step4_distance(g, [f32(x) for x in P])
        return float(np.log(np.float64(f32(max_dist)) / np.float64(dist3D)) / np.float64(g.log_sf))


def fuse(kfs, points, normals, min_dist, max_dist, mp_desc, inv_level_sigma2, th=3.0, skip=None, pair_skip=None,
         ratios=None):
    """Every keyframe against every point. Returns (nfused (B,), best_idx, best_dist, level (B, n),
    counters). ratios: a list that receives (b, m, level_ratio64) of every pair reaching step 6."""
    kfs = list(kfs)
    B = len(kfs)
    P = np.asarray(points, f32).reshape(-1, 3)
    n = P.shape[0]
    N = np.asarray(normals, f32).reshape(-1, 3)
    mn, mx = np.asarray(min_dist, f32), np.asarray(max_dist, f32)
    D = np.asarray(mp_desc, np.uint8).reshape(-1, 32)
    inv_s2 = np.asarray(inv_level_sigma2, f32)
    ps = None if pair_skip is None else np.asarray(pair_skip).reshape(B, n)
    idx = np.full((B, n), -1, np.int32)
    dist = np.full((B, n), 256, np.int32)
    lvl = np.full((B, n), -1, np.int32)
    cnt = {k: 0 for k in COUNTERS}
    for b, kf in enumerate(kfs):
        g = Grid(kf)
        for m in range(n):
            if skip is not None and skip[m]:
                cnt["skip"] += 1
                continue
            if ps is not None and ps[b, m]:
                cnt["pair_skip"] += 1
                continue
            idx[b, m], dist[b, m], lvl[b, m] = fuse_pair(g, P[m], N[m], mn[m], mx[m], D[m], inv_s2, th, cnt)
            if ratios is not None and lvl[b, m] >= 0:
                ratios.append((b, m, level_ratio64(g, P[m], mx[m])))
    return (idx >= 0).sum(1).astype(np.int32), idx, dist, lvl, cnt


def fuse_scene(s, **over):
    """fuse() on a scene dict of synthetic_fuse_scene (keys of `over` replace the scene's)."""
    a = dict(s, **over)
    return fuse(a["kfs"], a["points"], a["normals"], a["min_dist"], a["max_dist"], a["mp_desc"],
                a["inv_level_sigma2"], a["th"], a["skip"], a["pair_skip"], a.get("ratios"))


# ---- small hand-made cases: a keyframe at the identity pose, a point through a chosen pixel ----
def make_keyframe(kps, descs, bounds=None, cam=None):
    """A ProjFrame at the identity pose (mOw = 0) with keypoints (x, y, octave)."""
    from orb_slam3_ros2_amd._lib import KP_DTYPE
    from orb_slam3_ros2_amd.matcher import ProjFrame
    from orb_slam3_ros2_amd.synthetic import D435I
    cam = D435I if cam is None else cam
    k = np.zeros(len(kps), KP_DTYPE)
    for i, (x, y, o) in enumerate(kps):
        k["x"][i], k["y"][i], k["octave"][i] = x, y, o
    d = np.array(descs, np.uint8).reshape(len(kps), 32)
    return ProjFrame(k, d, [0, 0, 0, 1], [0, 0, 0], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["w"], cam["h"],
                     bounds=bounds)


def make_point(u, v, z, level, cam=None):
    """A MapPoint that projects near (u, v) at depth z with predicted level `level` as the identity
    pose sees it: P, its exact fp32 projection (u, v), dist (dist3D), a distance range and a normal
    along the viewing ray."""
    from orb_slam3_ros2_amd.synthetic import D435I
    cam = D435I if cam is None else cam
    P = np.array([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], f32)
    g = Grid(make_keyframe([], np.zeros((0, 32)), cam=cam))
    pu, pv = step2_project(g, step1_camera(g, P))
    _, d = step4_distance(g, P)
    mx = f32(float(d) * 1.2 ** (level - 0.5))
    return dict(P=P, u=pu, v=pv, dist=d, max_dist=mx, min_dist=f32(float(mx) / 1.2 ** 7),
                normal=(P / np.linalg.norm(P)).astype(f32))


# ---- the parity scene set (tests/test_fuse.py asserts its conditions on the CPU,
# tests/test_fuse_gpu.py runs the library on it) ----
PARITY_SCENES = [dict(n_kp=300, n_mp=300, B=3, seed=s) for s in (0, 1, 2)]
_scene_cache = {}


def parity_scene(k: int):
    """Scene k of the set with the restatement's result under "expected" = (nfused, best_idx,
    best_dist, level, counters) and "ratios" (built once per process; treat it as read-only)."""
    if k not in _scene_cache:
        from orb_slam3_ros2_amd.synthetic import synthetic_fuse_scene
        s = synthetic_fuse_scene(**PARITY_SCENES[k])
        s["ratios"] = []
        s["expected"] = fuse_scene(s)
        _scene_cache[k] = s
    return _scene_cache[k]
