#!/usr/bin/env python3
"""Times ORBmatcher.Fuse (B keyframes against one list of MapPoints in one call) and, as the
nearest path the library had without it, B sequential SearchLocalPoints calls of the same sizes on
the same context. SearchLocalPoints computes a DIFFERENT rule (isInFrustum's matrix projection,
RadiusByViewingCos, a ratio test, greedy claims, no chi-square gate): the comparison is of call
shapes, not of results. Every call ends in a stream synchronisation, so the host clock around a call
covers its staging, upload, kernels and read-back. The batched call is timed through the Python
mirror (batched_call_ms, as the SearchLocalPoints calls are), again after the sequential calls (a
second window of the same run) and as the bare C call with the structs marshalled once (c_call_ms).
The kernel-only time (k_fuse_grid + k_fuse_search) comes from the library's stage timer
(orbhip_profile_stage 8: one event pair per call), taken in calls of their own. Prints one JSON line.

    python tools/time_fuse.py [--B 30] [--n-mp 1000] [--n-kp 1000] [--calls 50] [--warmup 10]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=30)
    ap.add_argument("--n-mp", type=int, default=1000)
    ap.add_argument("--n-kp", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_fuse: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import ORBmatcher
    from orb_slam3_ros2_amd._lib import Context, FrameC, LocalPointsC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_fuse_scene
    s = synthetic_fuse_scene(a.n_kp, a.n_mp, a.B, a.seed)
    kfs, inv_s2 = s["kfs"], s["inv_level_sigma2"]
    pts, nrm, mn, mx, desc, skip, ps = (s[k] for k in ("points", "normals", "min_dist", "max_dist", "mp_desc", "skip",
                                                       "pair_skip"))
    ctx = Context()
    mt = ORBmatcher(0.6, True, ctx=ctx)

    def batched():
        return mt.Fuse(kfs, pts, nrm, mn, mx, desc, inv_s2, s["th"], skip, ps)

    def sequential():
        tot = 0
        for kf in kfs:
            tot += mt.SearchLocalPoints(kf, pts, nrm, mn, mx, desc, skip, th=s["th"])[0]
        return tot

    # the bare C call: the structs marshalled once, as a C++ caller holds them
    L = lib()
    arr = (FrameC * a.B)(*[k.to_c() for k in kfs])
    lc = LocalPointsC(a.n_mp, ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(desc), ptr(skip))
    idx = np.empty((a.B, a.n_mp), np.int32)
    dist = np.empty((a.B, a.n_mp), np.int32)
    lvl = np.empty((a.B, a.n_mp), np.int32)
    nf = np.empty(a.B, np.int32)

    def bare():
        return check(L.orbhip_fuse(ctx.handle, arr, a.B, ctypes.byref(lc), ptr(ps), ptr(inv_s2), s["th"], ptr(idx),
                                   ptr(dist), ptr(lvl), ptr(nf)), "orbhip_fuse")

    def bare_idx_only():
        return check(L.orbhip_fuse(ctx.handle, arr, a.B, ctypes.byref(lc), ptr(ps), ptr(inv_s2), s["th"], ptr(idx),
                                   None, None, ptr(nf)), "orbhip_fuse")

    nfused, idx_py, _, _ = batched()
    assert bare() == int(nfused.sum()) and np.array_equal(idx, idx_py)
    bare_t = median_ms(bare, a.calls, a.warmup)
    bare_idx_t = median_ms(bare_idx_only, a.calls, a.warmup)
    bat = median_ms(batched, a.calls, a.warmup)
    seq = median_ms(sequential, a.calls, a.warmup)
    bat2 = median_ms(batched, a.calls, 2)      # again after the other: the spread between two windows
    bare2 = median_ms(bare, a.calls, 2)
    check(L.orbhip_profile_stage(ctx.handle, 8), "orbhip_profile_stage")
    for _ in range(a.calls):
        bare()
    ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
    check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
    check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
    print(json.dumps(dict(
        tool="time_fuse", device=torch.cuda.get_device_name(0), B=a.B, n_mp=a.n_mp, n_kp=a.n_kp, calls=a.calls,
        fused_per_keyframe=[int(v) for v in nfused],
        c_call_ms=bare_t, c_call_again_ms=bare2, c_call_best_idx_only_ms=bare_idx_t,
        batched_call_ms=bat, batched_call_again_ms=bat2,
        sequential_search_local_points_ms=dict(seq, calls_per_sample=a.B),
        kernels_only_ms=ms.value / max(cnt.value, 1), kernel_samples=int(cnt.value))))


if __name__ == "__main__":
    main()
