#!/usr/bin/env python3
"""Times Optimizer::OptimizeSim3 on the device: the whole two-round procedure of every candidate in
one launch.

Three shapes: B = 1 candidate x n = 100 correspondences, B = 3 x n = 300 (a
DetectCommonRegionsFromBoW round) and B = 1 x n = 1000; free scale, 20 % outliers. Per shape: the
bare C call (orbhip_optimize_sim3_batch, structs marshalled once), the Python mirror
(Optimizer.OptimizeSim3_batch), the kernel alone through the library's stage timer
(orbhip_profile_stage 13, in calls of their own), and beside them, in the same run, the float64
numpy restatement of the tests on the host (fewer calls: it is the slow side). As a sanity figure the
same run times PoseOptimization for one frame of 300 points. Every device call ends in a stream
synchronisation, so the host clock around it covers staging, upload, kernel and read-back. Each
figure is the median of --calls calls after --warmup calls; the C call is taken in two windows of
one run (the second after everything else ran: their spread is the noise). Prints one JSON line.

    python tools/time_sim3_opt.py [--calls 50] [--warmup 10]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1, 100), (3, 300), (1, 1000))   # B, n


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
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_sim3_opt: needs a GPU (no fallback)")
    import sim3_opt_numpy as ref
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd._lib import Context, Sim3OptProblemC, Sim3OptResultC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_pose_problem, synthetic_sim3_opt_problem
    L = lib()
    ctx = Context()
    opt = Optimizer(ctx=ctx)

    def kernel_ms(fn):
        check(L.orbhip_profile_stage(ctx.handle, 13), "orbhip_profile_stage")
        for _ in range(a.calls):
            fn()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
        return ms.value / max(cnt.value, 1)

    pose, _ = synthetic_pose_problem(n=300, outlier_frac=0.15, seed=a.seed)
    pose_ms = median_ms(lambda: opt.PoseOptimization(pose), a.calls, a.warmup)
    rows = []
    for B, n in SHAPES:
        probs = [synthetic_sim3_opt_problem(n=n, outlier_frac=0.2, seed=a.seed + b)[0].normalized() for b in range(B)]
        cprobs = (Sim3OptProblemC * B)(*[p.to_c() for p in probs])
        cres = (Sim3OptResultC * B)()
        keeps = [np.zeros(n, np.uint8) for _ in range(B)]
        for b in range(B):
            cres[b].keep = ptr(keeps[b])

        def bare():
            return check(L.orbhip_optimize_sim3_batch(ctx.handle, cprobs, B, cres), "orbhip_optimize_sim3_batch")

        def mirror():
            return opt.OptimizeSim3_batch(probs)

        def host():
            return [ref.optimize_sim3(p) for p in probs]

        bare()
        want = host()
        agree = all(r.n_in == w["n_in"] and r.n_bad == w["n_bad"] and np.array_equal(k, w["keep"])
                    for r, w, k in zip(cres, want, keeps))
        row = dict(B=B, n=n, n_in=[int(r.n_in) for r in cres], n_bad=[int(r.n_bad) for r in cres],
                   lm_trials=[int(r.lm_trials) for r in cres], equals_restatement=bool(agree),
                   c_call_ms=median_ms(bare, a.calls, a.warmup), mirror_call_ms=median_ms(mirror, a.calls, a.warmup),
                   numpy_f64_ms=median_ms(host, max(3, a.calls // 10), 1), kernel_only_ms=kernel_ms(bare),
                   c_call_again_ms=median_ms(bare, a.calls, 2))
        rows.append(row)
    print(json.dumps(dict(tool="time_sim3_opt", device=torch.cuda.get_device_name(0), calls=a.calls,
                          pose_optimization_300_ms=pose_ms, shapes=rows)))


if __name__ == "__main__":
    main()
