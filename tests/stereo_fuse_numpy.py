"""Test infrastructure: the stereo branch of U:src/ORBmatcher.cc::Fuse(pKF, vpMapPoints, th, bRight =
false) as DESIGN.md "Stereo LocalMapping" writes it down. Only step 9 differs from the monocular
rule, so every other step is tests/fuse_numpy.py's, imported; the changed step is restated here in
explicit np.float32 scalars (fp64 comparisons on the widened value). Not used by the product.

Keyframes are orb_slam3_ros2_amd.matcher.ProjFrame objects that carry u_right (mvuRight, one per
keypoint; >= 0: a stereo keypoint) and bf (mbf)."""
import numpy as np

import fuse_numpy as F

f32 = np.float32

# fuse_numpy's counters; cand_chi2 counts the candidates either chi-square test dropped, and of the
# stereo candidates (ur >= 0): only_78 passed at 7.8 with a (u, v) error the monocular 5.99 rejects,
# only_er were dropped at 7.8 with a (u, v) error the monocular 5.99 accepts; cand_stereo / cand_mono:
# the candidates that reached the chi-square gate, by kind
COUNTERS = F.COUNTERS + ("cand_stereo", "cand_mono", "only_78", "only_er")


def right_projection(g, bf, Pc, u):
    """urp = u - bf * (1 / Pc.z)."""
    invz = f32(1.0) / Pc[2]
    return u - f32(bf) * invz


def step9_walk_stereo(g, ur, urp, cand, u, v, lvl, desc, inv_s2, cnt):
    """The candidate loop with the stereo chi-square. Returns (bestDist, bestIdx)."""
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
        mono_ok = not np.float64(e2 * inv_s2[o]) > 5.99
        if ur[idx] >= f32(0.0):
            cnt["cand_stereo"] += 1
            er = urp - ur[idx]
            e3 = e2 + er * er
            if np.float64(e3 * inv_s2[o]) > 7.8:
                cnt["cand_chi2"] += 1
                cnt["only_er"] += mono_ok
                continue
            cnt["only_78"] += not mono_ok
        else:
            cnt["cand_mono"] += 1
            if not mono_ok:
                cnt["cand_chi2"] += 1
                continue
        dist = int(F._POP[np.bitwise_xor(g.desc[idx], d)].sum())
        if dist < best_dist:
            best_dist, best_idx, best_cell = dist, idx, cell
        elif dist == best_dist:
            cnt["tie_cell" if cell != best_cell else "tie_index"] += 1
    return best_dist, best_idx


def fuse_pair_stereo(g, ur, bf, P, Pn, min_dist, max_dist, desc, inv_s2, th, cnt):
    """fuse_numpy.fuse_pair with step 9 replaced (the gates before it are the same calls)."""
    with np.errstate(all="ignore"):
        P = [f32(x) for x in P]
        Pc = F.step1_camera(g, P)
        if Pc[2] < f32(0.0):
            cnt["behind"] += 1
            return -1, 256, -1
        u, v = F.step2_project(g, Pc)
        if not F.step3_in_image(g, u, v):
            cnt["outside"] += 1
            return -1, 256, -1
        PO, dist3D = F.step4_distance(g, P)
        if dist3D < f32(0.8) * f32(min_dist):
            cnt["dist_low"] += 1
            return -1, 256, -1
        if dist3D > f32(1.2) * f32(max_dist):
            cnt["dist_high"] += 1
            return -1, 256, -1
        if not F.step5_view_ok(PO, Pn, dist3D):
            cnt["angle"] += 1
            return -1, 256, -1
        lvl = F.step6_level(g, max_dist, dist3D)
        r = F.step7_radius(g, th, lvl)
        cand = F.step8_area(g, u, v, r)
        if cand is None:
            cnt["no_window"] += 1
            return -1, 256, lvl
        best_dist, best_idx = step9_walk_stereo(g, ur, right_projection(g, bf, Pc, u), cand, u, v, lvl, desc, inv_s2, cnt)
        if best_idx < 0:
            cnt["no_candidate"] += 1
            return -1, 256, lvl
        if best_dist <= F.TH_LOW:
            cnt["accepted"] += 1
            return best_idx, best_dist, lvl
        cnt["th_low"] += 1
        return -1, best_dist, lvl


def fuse_stereo(kfs, points, normals, min_dist, max_dist, mp_desc, inv_level_sigma2, th=3.0, skip=None,
                pair_skip=None, ratios=None):
    """Every stereo keyframe against every point; arguments and results of fuse_numpy.fuse."""
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
        g = F.Grid(kf)
        ur = np.asarray(kf.u_right, f32).reshape(-1)
        assert ur.shape[0] == g.x.shape[0]
        for m in range(n):
            if skip is not None and skip[m]:
                cnt["skip"] += 1
                continue
            if ps is not None and ps[b, m]:
                cnt["pair_skip"] += 1
                continue
            idx[b, m], dist[b, m], lvl[b, m] = fuse_pair_stereo(g, ur, kf.bf, P[m], N[m], mn[m], mx[m], D[m], inv_s2, th,
                                                               cnt)
            if ratios is not None and lvl[b, m] >= 0:
                ratios.append((b, m, F.level_ratio64(g, P[m], mx[m])))
    return (idx >= 0).sum(1).astype(np.int32), idx, dist, lvl, cnt


def fuse_stereo_scene(s, **over):
    """fuse_stereo() on a scene dict of synthetic_stereo_fuse_scene (keys of `over` replace the scene's)."""
    a = dict(s, **over)
    return fuse_stereo(a["kfs"], a["points"], a["normals"], a["min_dist"], a["max_dist"], a["mp_desc"],
                       a["inv_level_sigma2"], a["th"], a["skip"], a["pair_skip"], a.get("ratios"))


def stereo_keyframe(kf, u_right, bf, b):
    """A copy of ProjFrame `kf` (sharing its arrays) that carries the stereo members."""
    from orb_slam3_ros2_amd.matcher import ProjFrame
    out = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, claimed=kf.claimed,
                    bounds=kf.bounds, u_right=u_right, bf=bf, b=b)
    out.scale_factors, out.log_scale_factor = kf.scale_factors, kf.log_scale_factor
    return out


def mono_keyframe(kf):
    """The same keyframe without its stereo members."""
    from orb_slam3_ros2_amd.matcher import ProjFrame
    out = ProjFrame(kf.kps, kf.desc, kf.pose_q, kf.pose_t, kf.fx, kf.fy, kf.cx, kf.cy, claimed=kf.claimed,
                    bounds=kf.bounds)
    out.scale_factors, out.log_scale_factor = kf.scale_factors, kf.log_scale_factor
    return out


# ---- direct cases: one keyframe at the identity pose, one point, one keypoint; the answer follows
# from the definition (tests/test_stereo_fuse.py runs the restatement on them, tests/test_stereo_fuse_gpu.py
# the library) ----
DIRECT_B = 0.08


def direct_cases():
    """[dict(name, kf (stereo), pt (fuse_numpy.make_point), want = (best_idx, best_dist) under the
    stereo rule, mono = the same under the monocular rule on the keyframe without u_right, chi2 =
    the float64 value the stereo test compares, or None)]. The descriptor of the point is all zeros,
    as the keypoint's."""
    from orb_slam3_ros2_amd.synthetic import D435I, orb_scale_tables
    sf, s2 = orb_scale_tables()
    inv_s2 = (f32(1.0) / s2).astype(f32)
    bf = float(f32(f32(D435I["fx"]) * f32(DIRECT_B)))
    probe = F.Grid(F.make_keyframe([], np.zeros((0, 32))))
    cases = []

    def add(name, octave, rho, d_ur, want, mono, ur_value=None):
        """The keypoint rho level sigma from the projection along +x; its right coordinate d_ur level
        sigma below the point's right projection (ur_value: that value instead)."""
        pt = F.make_point(300.0, 200.0, 4.0, octave)
        Pc = F.step1_camera(probe, [f32(x) for x in pt["P"]])
        urp = right_projection(probe, bf, Pc, pt["u"])
        x = f32(pt["u"] + f32(rho * float(sf[octave])))
        ur = f32(urp - f32(d_ur * float(sf[octave]))) if ur_value is None else f32(ur_value)
        ex, er = pt["u"] - x, urp - ur
        chi2 = None
        if ur >= 0:
            chi2 = float(np.float64(((ex * ex + f32(0) * f32(0)) + er * er) * inv_s2[octave]))
        kf = stereo_keyframe(F.make_keyframe([(x, pt["v"], octave)], np.zeros((1, 32), np.uint8)), [ur], bf, DIRECT_B)
        cases.append(dict(name=name, kf=kf, pt=pt, want=want, mono=mono, chi2=chi2, octave=octave))

    hit, miss = (0, 0), (-1, 256)
    for o in (0, 7):
        # 2.6^2 = 6.76: above 5.99, below 7.8
        add(f"uv_2.6_sigma_perfect_ur_octave{o}", o, 2.6, 0.0, hit, miss)
        # 7.8 = 2.7928^2, by the right coordinate alone
        add(f"ur_2.79_sigma_octave{o}", o, 0.0, 2.79, hit, hit)
        add(f"ur_2.80_sigma_octave{o}", o, 0.0, 2.80, miss, hit)
        add(f"ur_minus_2.79_sigma_octave{o}", o, 0.0, -2.79, hit, hit)
        add(f"ur_minus_2.80_sigma_octave{o}", o, 0.0, -2.80, miss, hit)
    # what makes a keypoint stereo: 0.0f counts (and is far from the right projection), -1 and NaN do not
    add("ur_zero_is_stereo", 3, 0.0, 0.0, miss, hit, ur_value=0.0)
    add("ur_minus_one_is_monocular", 3, 0.0, 0.0, hit, hit, ur_value=-1.0)
    add("ur_nan_is_monocular", 3, 0.0, 0.0, hit, hit, ur_value=np.nan)
    # a monocular keypoint 2.6 sigma away keeps the 5.99 test
    add("uv_2.6_sigma_monocular", 3, 2.6, 0.0, miss, miss, ur_value=-1.0)
    return cases


def direct_args(c):
    """The Fuse arguments of a direct case after the keyframes: points .. mp_desc."""
    pt = c["pt"]
    return (pt["P"][None], pt["normal"][None], np.array([pt["min_dist"]], f32), np.array([pt["max_dist"]], f32),
            np.zeros((1, 32), np.uint8))


# ---- the parity scene set (tests/test_stereo_fuse.py asserts its conditions on the CPU,
# tests/test_stereo_fuse_gpu.py runs the library on it) ----
PARITY_SCENES = [dict(n_kp=300, n_mp=300, B=3, seed=s) for s in (0, 1, 2)]
_scene_cache = {}


def parity_scene(k: int):
    """Scene k of the set with the restatement's result under "expected" = (nfused, best_idx,
    best_dist, level, counters) and "ratios" (built once per process; treat it as read-only)."""
    if k not in _scene_cache:
        from orb_slam3_ros2_amd.synthetic import synthetic_stereo_fuse_scene
        s = synthetic_stereo_fuse_scene(**PARITY_SCENES[k])
        s["ratios"] = []
        s["expected"] = fuse_stereo_scene(s)
        _scene_cache[k] = s
    return _scene_cache[k]
