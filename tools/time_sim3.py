#!/usr/bin/env python3
"""Times the two Sim3 functions LoopClosing calls.

ORBmatcher.FuseSim3 (B keyframes against one list of MapPoints) beside ORBmatcher.Fuse on the same
scene: the same kernels with and without the chi-square gate. ORBmatcher.SearchByProjectionSim3 (one
keyframe, the sequential greedy pass) at upstream's three (th, ratioHamming) pairs beside
SearchLocalPoints at the same sizes, the nearest path the library had; SearchLocalPoints computes a
DIFFERENT rule (a ratio test, RadiusByViewingCos), so that comparison is of call shapes only. Every
call ends in a stream synchronisation, so the host clock around a call covers its staging, upload,
kernels and read-back. Each figure is the median of --calls calls after --warmup calls, taken in two
windows of one run (the second after everything else ran: their spread is the noise). The bare C
calls marshal their structs once. Kernel-only times come from the library's stage timer
(orbhip_profile_stage 8: Fuse / Fuse-Sim3, 9: the projection search's three launches), taken in
calls of their own. Prints one JSON line.

    python tools/time_sim3.py [--B 30] [--n-mp 1000] [--n-kp 1000] [--proj-kp 1250] [--proj-mp 3000]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SETTINGS = ((3, 1.5), (5, 1.0), (8, 1.5))


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
    ap.add_argument("--proj-kp", type=int, default=1250)
    ap.add_argument("--proj-mp", type=int, default=3000)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_sim3: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import ORBmatcher
    from orb_slam3_ros2_amd._lib import Context, FrameC, LocalPointsC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_fuse_scene, synthetic_sim3_scene
    L = lib()
    ctx = Context()
    mt = ORBmatcher(0.6, True, ctx=ctx)

    def kernels_ms(stage, fn):
        check(L.orbhip_profile_stage(ctx.handle, stage), "orbhip_profile_stage")
        for _ in range(a.calls):
            fn()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
        return ms.value / max(cnt.value, 1)

    # ---- Fuse with a Sim3 beside Fuse ----
    s = synthetic_fuse_scene(a.n_kp, a.n_mp, a.B, a.seed, th=4.0)
    kfs, inv_s2 = s["kfs"], s["inv_level_sigma2"]
    pts, nrm, mn, mx, desc, skip, ps = (s[k] for k in ("points", "normals", "min_dist", "max_dist", "mp_desc", "skip",
                                                       "pair_skip"))
    arr = (FrameC * a.B)(*[k.to_c() for k in kfs])
    lc = LocalPointsC(a.n_mp, ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(desc), ptr(skip))
    idx = np.empty((a.B, a.n_mp), np.int32)
    dist = np.empty((a.B, a.n_mp), np.int32)
    lvl = np.empty((a.B, a.n_mp), np.int32)
    nf = np.empty(a.B, np.int32)

    def fuse_bare():
        return check(L.orbhip_fuse(ctx.handle, arr, a.B, ctypes.byref(lc), ptr(ps), ptr(inv_s2), 4.0, ptr(idx),
                                   ptr(dist), ptr(lvl), ptr(nf)), "orbhip_fuse")

    def sim3_bare():
        return check(L.orbhip_fuse_sim3(ctx.handle, arr, a.B, ctypes.byref(lc), ptr(ps), 4.0, ptr(idx), ptr(dist),
                                        ptr(lvl), ptr(nf)), "orbhip_fuse_sim3")

    def sim3_mirror():
        return mt.FuseSim3(kfs, pts, nrm, mn, mx, desc, 4.0, skip, ps)

    n_fuse = fuse_bare()
    n_sim3 = sim3_bare()
    assert n_sim3 == int(sim3_mirror()[0].sum()) >= n_fuse
    fuse = dict(B=a.B, n_mp=a.n_mp, n_kp=a.n_kp, fused=dict(fuse=n_fuse, fuse_sim3=n_sim3),
                fuse_c_call_ms=median_ms(fuse_bare, a.calls, a.warmup),
                fuse_sim3_c_call_ms=median_ms(sim3_bare, a.calls, a.warmup),
                fuse_sim3_mirror_call_ms=median_ms(sim3_mirror, a.calls, a.warmup))

    # ---- SearchByProjection with a Sim3 beside SearchLocalPoints ----
    proj = []
    for th, ratio in SETTINGS:
        p = synthetic_sim3_scene(a.proj_kp, a.proj_mp, a.seed, th=float(th), ratio=ratio, n_claimed=a.proj_kp // 15)
        kf = p["kf"]
        fc = kf.to_c()
        plc = LocalPointsC(a.proj_mp, *[ptr(p[k]) for k in ("points", "normals", "min_dist", "max_dist", "mp_desc", "skip")])
        match = np.empty(a.proj_mp, np.int32)
        mdist = np.empty(a.proj_mp, np.int32)
        mlvl = np.empty(a.proj_mp, np.int32)

        def bare():
            return check(L.orbhip_search_by_projection_sim3(ctx.handle, ctypes.byref(fc), ctypes.byref(plc), float(th),
                                                            ratio, ptr(match), ptr(mdist), ptr(mlvl)),
                         "orbhip_search_by_projection_sim3")

        def mirror():
            return mt.SearchByProjectionSim3(kf, p["points"], p["normals"], p["min_dist"], p["max_dist"], p["mp_desc"],
                                             th, ratio, p["skip"])

        def local():
            return mt.SearchLocalPoints(kf, p["points"], p["normals"], p["min_dist"], p["max_dist"], p["mp_desc"],
                                        p["skip"], th=float(th))[0]

        nm = bare()
        assert nm == mirror()[0]
        row = dict(th=th, ratio=ratio, n_kp=a.proj_kp, n_mp=a.proj_mp, matches=nm,
                   c_call_ms=median_ms(bare, a.calls, a.warmup), mirror_call_ms=median_ms(mirror, a.calls, a.warmup),
                   search_local_points_ms=median_ms(local, a.calls, a.warmup),
                   c_call_again_ms=median_ms(bare, a.calls, 2), kernels_only_ms=kernels_ms(9, bare))
        proj.append(row)

    # the second window of the Fuse figures, after everything else ran
    fuse.update(fuse_c_call_again_ms=median_ms(fuse_bare, a.calls, 2),
                fuse_sim3_c_call_again_ms=median_ms(sim3_bare, a.calls, 2),
                fuse_kernels_only_ms=kernels_ms(8, fuse_bare), fuse_sim3_kernels_only_ms=kernels_ms(8, sim3_bare))
    print(json.dumps(dict(tool="time_sim3", device=torch.cuda.get_device_name(0), calls=a.calls, fuse=fuse,
                          search_by_projection=proj)))


if __name__ == "__main__":
    main()
