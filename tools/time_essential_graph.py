#!/usr/bin/env python3
"""Times Optimizer::OptimizeEssentialGraph on the device: the pose graph of a loop closure, the
Levenberg slots enqueued without a host round trip, and the map-point correction in the same call.

The flagship shape is a loop of 400 keyframes (399 free vertices, n = 2793) with 3 covisibility edges
per keyframe, 5 loop keyframes, 20 000 map points and upstream's 20 iterations; beside it a 100- and
a 200-keyframe loop. Per shape: the bare C call (orbhip_optimize_essential_graph, structs marshalled
once), the Python mirror, and the device span of one call through the library's stage timer
(orbhip_profile_stage 15: the first kernel's start to the last kernel's end, in calls of their own),
each on the default solver route and with ORBHIP_EG_BLOCKED=1. Every call ends in a stream
synchronisation, so the host clock around it covers the structure build, staging, upload, slots and
read-back. Each figure is the median of --calls calls after --warmup calls. There is no g2o on these
machines, so no CPU baseline is timed; --numpy times the float64 restatement of the tests on the
smallest shape as a sanity figure only. Prints one JSON line.

    python tools/time_essential_graph.py [--calls 10] [--warmup 2] [--numpy]
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

SHAPES = ((100, 5000), (200, 10000), (400, 20000))   # keyframes, map points


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
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--numpy", action="store_true")
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_essential_graph: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd._lib import Context, EssentialGraphResultC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_essential_graph
    L = lib()
    ctx = Context()
    opt = Optimizer(ctx=ctx)

    def span_ms(fn):
        check(L.orbhip_profile_stage(ctx.handle, 15), "orbhip_profile_stage")
        for _ in range(a.calls):
            fn()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
        return ms.value / max(cnt.value, 1)

    rows = []
    for n_kf, n_pts in SHAPES:
        p = synthetic_essential_graph(n_kf=n_kf, k_covis=3, loop_span=5, seed=a.seed, n_points=n_pts)[0].normalized()
        S, pts = np.zeros_like(p.S), np.zeros_like(p.points)
        pc, r = p.to_c(), EssentialGraphResultC()
        r.S, r.points = ptr(S), ptr(pts)

        def bare():
            return check(L.orbhip_optimize_essential_graph(ctx.handle, ctypes.byref(pc), ctypes.byref(r)),
                         "orbhip_optimize_essential_graph")

        row = dict(keyframes=n_kf, n=7 * (n_kf - 1), edges=int(p.edge_ij.shape[0]), points=n_pts, iterations=p.iterations)
        for route, env in (("default", None), ("blocked", "1")):
            if env:
                os.environ["ORBHIP_EG_BLOCKED"] = env
            else:
                os.environ.pop("ORBHIP_EG_BLOCKED", None)
            bare()
            row[route] = dict(solver=int(r.solver), iterations_run=int(r.iterations_run), lm_trials=int(r.lm_trials),
                              lm_rejected=int(r.lm_rejected), chi2_initial=r.chi2_initial, chi2_final=r.chi2_final,
                              c_call_ms=median_ms(bare, a.calls, a.warmup),
                              mirror_call_ms=median_ms(lambda: opt.OptimizeEssentialGraph(p), a.calls, a.warmup),
                              device_span_ms=span_ms(bare))
        os.environ.pop("ORBHIP_EG_BLOCKED", None)
        if a.numpy and n_kf == SHAPES[0][0]:
            import essential_graph_numpy as ref
            row["numpy_f64_ms"] = median_ms(lambda: ref.optimize_essential_graph(
                p.S, p.fixed, p.edge_ij, p.edge_S, p.fix_scale, p.iterations, p.lambda_init, p.points, p.point_ref), 1, 0)
        rows.append(row)
    print(json.dumps(dict(tool="time_essential_graph", device=torch.cuda.get_device_name(0), calls=a.calls,
                          shapes=rows)))


if __name__ == "__main__":
    main()
