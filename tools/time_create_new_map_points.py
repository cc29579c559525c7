#!/usr/bin/env python3
"""Times orbhip_create_new_map_points (SearchForTriangulation and the triangulation of its matches
in one call) against orbhip_search_for_triangulation alone and against a NumPy-vectorised host
triangulation of the same matches, the stand-in for what a caller did on the host before. The C
calls are bare (structs marshalled once, as a C++ caller holds them) and end in a stream
synchronisation, so the host clock around a call covers its upload, kernels and read-back; every
figure is the median of --calls calls after --warmup, in two windows. The kernels' own time comes
from the library's stage timer (7: the search's launch pair, 10: k_tri_points and k_tri_claim), in
calls of their own. Prints one JSON line.

    python tools/time_create_new_map_points.py [--B 20] [--n 1000] [--nodes 100] [--calls 50] [--warmup 10]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    t = np.array(t)
    return dict(median=float(np.median(t)), min=float(t.min()), p90=float(np.percentile(t, 90)))


def host_triangulation(k1, nb, m12, sf, s2, cos_max, ratio_factor):
    """The host loop a caller ran on the read-back matches, vectorised per neighbour: rays, parallax,
    the 4x4 systems by numpy's batched float32 SVD, depth, reprojection and scale checks, then the
    first accepting neighbour per feature. Returns the number of new points."""
    from orb_slam3_ros2_amd.synthetic import quat_to_rot64
    f = np.float32

    def cam(k):
        R = quat_to_rot64(k.pose_q).astype(f)
        t = k.pose_t.astype(f)
        return R, t, -(R.T @ t), np.concatenate([R, t[:, None]], 1)
    R1, t1, O1, T1 = cam(k1)
    taken = np.zeros(k1.n, bool)
    total = 0
    for b, k2 in enumerate(nb):
        i1 = np.nonzero(m12[b] >= 0)[0]
        if not i1.size:
            continue
        i2 = m12[b, i1]
        R2, t2, O2, T2 = cam(k2)
        p1 = np.stack([k1.kps["x"][i1], k1.kps["y"][i1]], 1)
        p2 = np.stack([k2.kps["x"][i2], k2.kps["y"][i2]], 1)
        xn1 = (p1 - f([k1.cx, k1.cy])) / f([k1.fx, k1.fy])
        xn2 = (p2 - f([k2.cx, k2.cy])) / f([k2.fx, k2.fy])
        r1 = np.concatenate([xn1, np.ones((len(i1), 1), f)], 1) @ R1
        r2 = np.concatenate([xn2, np.ones((len(i1), 1), f)], 1) @ R2
        cosp = (r1 * r2).sum(1) / (np.linalg.norm(r1, axis=1) * np.linalg.norm(r2, axis=1))
        A = np.stack([xn1[:, :1] * T1[2] - T1[0], xn1[:, 1:] * T1[2] - T1[1],
                      xn2[:, :1] * T2[2] - T2[0], xn2[:, 1:] * T2[2] - T2[1]], 1)
        v = np.linalg.svd(A)[2][:, 3]
        with np.errstate(all="ignore"):
            X = v[:, :3] / v[:, 3:]
            ok = (cosp > 0) & (cosp < cos_max) & (v[:, 3] != 0)
            for R, t, k, p, o in ((R1, t1, k1, p1, k1.kps["octave"][i1]), (R2, t2, k2, p2, k2.kps["octave"][i2])):
                Xc = X @ R.T + t
                e = f([k.fx, k.fy]) * Xc[:, :2] / Xc[:, 2:] + f([k.cx, k.cy]) - p
                ok &= (Xc[:, 2] > 0) & ((e * e).sum(1) <= 5.991 * s2[o])
            d1, d2 = np.linalg.norm(X - O1, axis=1), np.linalg.norm(X - O2, axis=1)
            rd, ro = d2 / d1, sf[k1.kps["octave"][i1]] / sf[k2.kps["octave"][i2]]
            ok &= (d1 > 0) & (d2 > 0) & ~(rd * ratio_factor < ro) & ~(rd > ro * ratio_factor)
        new = i1[ok & ~taken[i1]]
        taken[new] = True
        total += new.size
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=20)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_create_new_map_points: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd._lib import Context, NewPointsC, TriKeyFrameC, TriParamsC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_triangulation_scene
    s = synthetic_triangulation_scene(a.n, a.B, a.seed, n_nodes=a.nodes, n2=a.n)
    k1, nb, sf, s2 = s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"]
    ctx = Context()
    L = lib()
    c1 = k1.to_c()
    arr = (TriKeyFrameC * a.B)(*[k.to_c() for k in nb])
    n1 = k1.n
    m12 = np.empty((a.B, n1), np.int32)
    nmb = np.empty(a.B, np.int32)
    ratio = float(np.float32(1.5) * sf[1])
    prm = TriParamsC(0.9998, ratio, 0.0)
    gated, nnew = np.empty(a.B, np.uint8), np.empty(a.B, np.int32)
    first, nbr, i1, i2 = (np.empty(n1, np.int32) for _ in range(4))
    x3d = np.empty((n1, 3), np.float32)
    lean = NewPointsC(None, ptr(nmb), ptr(gated), None, None, ptr(first), ptr(nnew), ptr(nbr), ptr(i1), ptr(i2),
                      ptr(x3d))

    def search():
        return check(L.orbhip_search_for_triangulation(ctx.handle, ctypes.byref(c1), arr, a.B, ptr(sf), ptr(s2),
                                                       len(sf), 0, ptr(m12), ptr(nmb)), "orbhip_search_for_triangulation")

    def fused():
        return check(L.orbhip_create_new_map_points(ctx.handle, ctypes.byref(c1), arr, a.B, None, ptr(sf), ptr(s2),
                                                    len(sf), 0, ctypes.byref(prm), ctypes.byref(lean)),
                     "orbhip_create_new_map_points")

    def host():
        return host_triangulation(k1, nb, m12, sf, s2, 0.9998, np.float32(ratio))

    matches, points = search(), fused()
    host_points = host()
    out = dict(tool="time_create_new_map_points", device=torch.cuda.get_device_name(0), B=a.B, n=a.n, nodes=a.nodes,
               calls=a.calls, matches=matches, new_points=points, host_new_points=host_points,
               read_back_bytes=dict(search=a.B * n1 * 4 + a.B * 4, fused=(n1 + 2 * a.B + 1) * 4 + n1 * 24))
    for window in ("", "_again"):
        out["search_call_ms" + window] = median_ms(search, a.calls, a.warmup)
        out["fused_call_ms" + window] = median_ms(fused, a.calls, a.warmup)
        out["host_triangulation_ms" + window] = median_ms(host, a.calls, 2)
    for stage, name in ((7, "search_kernels_ms"), (10, "triangulation_kernels_ms")):
        check(L.orbhip_profile_stage(ctx.handle, stage), "orbhip_profile_stage")
        for _ in range(a.calls):
            fused()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        out[name] = ms.value / max(cnt.value, 1)
        out[name.replace("_ms", "_samples")] = int(cnt.value)
    check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
