#!/usr/bin/env python3
"""Times the stereo forms of LocalMapping's two map operations beside the monocular forms on the same
scene with the stereo members dropped. CreateNewMapPoints (orbhip_create_new_map_points_stereo /
orbhip_create_new_map_points without median_depth) at B = 20 neighbours x n = 1000 features and B = 30
x n = 2048 (synthetic_stereo_new_points_scene, scale 0.5: no neighbour is gated by mb, so both forms
search the same pairs). ORBmatcher.Fuse (orbhip_fuse_stereo / orbhip_fuse) for SearchInNeighbors' two
call shapes: B = 30 keyframes x 1000 MapPoints and B = 1 keyframe x 20000 MapPoints, 1000 keypoints
per keyframe (synthetic_stereo_fuse_scene). All are the bare C calls with the structs marshalled once;
every call ends in a stream synchronisation, so the host clock around a call covers its staging,
upload, kernels and read-back. Per case: 10 warm-up calls of each form, then `rounds` rounds of
(median of `calls` stereo calls, median of `calls` monocular calls), alternating in one run. The
kernel-only times (orbhip_profile_stage 7: the search, 10: the triangulation and the claim, 8:
k_fuse_grid + k_fuse_search; one event pair per call) are taken in calls of their own afterwards.
Prints one JSON line.

    python tools/time_stereo_local_mapping.py [--calls 50] [--warmup 10] [--rounds 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def window_ms(fn, calls):
    t = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--n-kp", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_stereo_local_mapping: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd._lib import (Context, FrameC, LocalPointsC, NewPointsC, StereoViewC, TriKeyFrameC,
                                         TriParamsC, TriStereoKeyFrameC, check, lib, ptr)
    from orb_slam3_ros2_amd.synthetic import synthetic_stereo_fuse_scene, synthetic_stereo_new_points_scene
    L = lib()
    ctx = Context()

    def kernels_ms(fn, stage=8):
        check(L.orbhip_profile_stage(ctx.handle, stage), "orbhip_profile_stage")
        for _ in range(a.calls):
            fn()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
        return round(ms.value / max(cnt.value, 1), 5)

    def alternate(stereo, mono):
        for fn in (stereo, mono):
            for _ in range(a.warmup):
                fn()
        ts, tm = [], []
        for _ in range(a.rounds):
            ts.append(round(window_ms(stereo, a.calls), 5))
            tm.append(round(window_ms(mono, a.calls), 5))
        return ts, tm

    new_points = []
    for B, n in ((20, 1000), (30, 2048)):
        s = synthetic_stereo_new_points_scene(n, B, a.seed, scale=0.5, gated_at=None, n_nodes=100, n2=n)
        k1, nb, sf, s2 = s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"]
        cs1, cm1 = k1.to_c_stereo(), s["mono_kf1"].to_c()
        arr_s = (TriStereoKeyFrameC * B)(*[k.to_c_stereo() for k in nb])
        arr_m = (TriKeyFrameC * B)(*[k.to_c() for k in s["mono_neighbours"]])
        n1 = k1.n
        prm = TriParamsC(0.9998, float(np.float32(1.5) * sf[1]), float(s["far_threshold"]))
        nmb, gated, nnew = np.empty(B, np.int32), np.empty(B, np.uint8), np.empty(B, np.int32)
        first, nbr, i1, i2 = (np.empty(n1, np.int32) for _ in range(4))
        x3d, source = np.empty((n1, 3), np.float32), np.zeros((B, n1), np.uint8)
        lean = NewPointsC(None, ptr(nmb), ptr(gated), None, None, ptr(first), ptr(nnew), ptr(nbr), ptr(i1), ptr(i2),
                          ptr(x3d))

        def stereo(src=None):
            return check(L.orbhip_create_new_map_points_stereo(ctx.handle, ctypes.byref(cs1), arr_s, B, ptr(sf), ptr(s2),
                                                               len(sf), 0, ctypes.byref(prm), ctypes.byref(lean), src),
                         "orbhip_create_new_map_points_stereo")

        def mono():
            return check(L.orbhip_create_new_map_points(ctx.handle, ctypes.byref(cm1), arr_m, B, None, ptr(sf), ptr(s2),
                                                        len(sf), 0, ctypes.byref(prm), ctypes.byref(lean)),
                         "orbhip_create_new_map_points")

        points = dict(stereo=stereo(ptr(source)), stereo_gated=int(gated.sum()), mono=mono())
        ts, tm = alternate(stereo, mono)
        new_points.append(dict(B=B, n=n, new_points=points,
                               source=[int(v) for v in np.bincount(source.ravel(), minlength=4)],
                               stereo_features=int(sum(int((k.u_right >= 0).sum()) for k in [k1] + nb)),
                               stereo_c_call_ms=ts, mono_c_call_ms=tm,
                               stereo_search_kernels_ms=kernels_ms(stereo, 7), mono_search_kernels_ms=kernels_ms(mono, 7),
                               stereo_triangulation_kernels_ms=kernels_ms(stereo, 10),
                               mono_triangulation_kernels_ms=kernels_ms(mono, 10)))

    cases = []
    for B, n_mp in ((30, 1000), (1, 20000)):
        s = synthetic_stereo_fuse_scene(a.n_kp, n_mp, B, a.seed)
        pts, nrm, mn, mx, desc, skip, ps, inv_s2 = (np.ascontiguousarray(s[k]) for k in (
            "points", "normals", "min_dist", "max_dist", "mp_desc", "skip", "pair_skip", "inv_level_sigma2"))
        views = (StereoViewC * B)(*[k.to_c_stereo() for k in s["kfs"]])
        frames = (FrameC * B)(*[k.to_c() for k in s["mono_kfs"]])
        lc = LocalPointsC(n_mp, ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(desc), ptr(skip))
        out = [np.empty((B, n_mp), np.int32) for _ in range(3)] + [np.empty(B, np.int32)]

        def stereo():
            return check(L.orbhip_fuse_stereo(ctx.handle, views, B, ctypes.byref(lc), ptr(ps), ptr(inv_s2), s["th"],
                                              ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])), "orbhip_fuse_stereo")

        def mono():
            return check(L.orbhip_fuse(ctx.handle, frames, B, ctypes.byref(lc), ptr(ps), ptr(inv_s2), s["th"],
                                       ptr(out[0]), ptr(out[1]), ptr(out[2]), ptr(out[3])), "orbhip_fuse")

        fused = dict(stereo=stereo(), mono=mono())
        ts, tm = alternate(stereo, mono)
        cases.append(dict(B=B, n_mp=n_mp, n_kp=a.n_kp, fused=fused,
                          stereo_keypoints=int(sum(int((k.u_right >= 0).sum()) for k in s["kfs"])),
                          stereo_c_call_ms=ts, mono_c_call_ms=tm,
                          stereo_kernels_only_ms=kernels_ms(stereo), mono_kernels_only_ms=kernels_ms(mono)))
    print(json.dumps(dict(tool="time_stereo_local_mapping", device=torch.cuda.get_device_name(0), calls=a.calls,
                          warmup=a.warmup, rounds=a.rounds, create_new_map_points=new_points, fuse=cases)))


if __name__ == "__main__":
    main()
