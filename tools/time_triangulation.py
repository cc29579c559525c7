#!/usr/bin/env python3
"""Times ORBmatcher.SearchForTriangulation (one keyframe against B neighbours in one call) and,
as the nearest path without it, B sequential SearchByBoW calls of the same sizes on the same
context. Both calls end in a stream synchronisation, so the host clock around a call covers its
upload, kernels and read-back. The batched call is timed twice: through the Python mirror
(batched_call_ms, as the SearchByBoW calls are) and as the bare C call with the structs marshalled
once (c_call_ms). The kernel-only time of the batched call comes from the library's
stage timer (orbhip_profile_stage 7: the ordering pre-pass and the search as one event pair), taken
in calls of their own. Prints one JSON line.

    python tools/time_triangulation.py [--B 20] [--n 1000] [--nodes 100] [--calls 50] [--warmup 10]
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
    return float(np.median(t)), float(t.min()), float(np.percentile(t, 90))


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
        sys.exit("time_triangulation: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import ORBmatcher
    from orb_slam3_ros2_amd._lib import Context, check, lib
    from orb_slam3_ros2_amd.synthetic import synthetic_triangulation_scene
    s = synthetic_triangulation_scene(a.n, a.B, a.seed, n_nodes=a.nodes, n2=a.n)
    k1, nb, sf, s2 = s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"]
    ctx = Context()
    mt = ORBmatcher(0.6, False, ctx=ctx)

    def batched():
        return mt.SearchForTriangulation(k1, nb, sf, s2)

    a1 = np.ascontiguousarray(k1.kps["angle"])
    a2 = [np.ascontiguousarray(k.kps["angle"]) for k in nb]
    valid = [np.ascontiguousarray(1 - k.has_mp) for k in nb]

    def sequential():
        tot = 0
        for b, k in enumerate(nb):
            n, _ = mt.SearchByBoW(k.desc, a2[b], k.node, k.weight, valid[b], k1.desc, a1, k1.node, k1.weight)
            tot += n
        return tot

    # the bare C call: the structs marshalled once, as a C++ caller holds them
    from orb_slam3_ros2_amd._lib import TriKeyFrameC, ptr
    L = lib()
    c1 = k1.to_c()
    arr = (TriKeyFrameC * a.B)(*[k.to_c() for k in nb])
    m12 = np.empty((a.B, k1.n), np.int32)
    nmb = np.empty(a.B, np.int32)

    def bare():
        return check(L.orbhip_search_for_triangulation(ctx.handle, ctypes.byref(c1), arr, a.B, ptr(sf), ptr(s2),
                                                       len(sf), 0, ptr(m12), ptr(nmb)), "orbhip_search_for_triangulation")

    nm, m_py = batched()
    assert bare() == int(nm.sum()) and np.array_equal(m12, m_py)
    bare_t = median_ms(bare, a.calls, a.warmup)
    bat = median_ms(batched, a.calls, a.warmup)
    seq = median_ms(sequential, a.calls, a.warmup)
    bat2 = median_ms(batched, a.calls, 2)      # again after the other: the spread between two windows
    check(L.orbhip_profile_stage(ctx.handle, 7), "orbhip_profile_stage")
    for _ in range(a.calls):
        batched()
    ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
    check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
    check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
    print(json.dumps(dict(
        tool="time_triangulation", device=torch.cuda.get_device_name(0), B=a.B, n=a.n, nodes=a.nodes, calls=a.calls,
        matches_per_pair=[int(v) for v in nm],
        c_call_ms=dict(median=bare_t[0], min=bare_t[1], p90=bare_t[2]),
        batched_call_ms=dict(median=bat[0], min=bat[1], p90=bat[2]),
        batched_call_again_ms=dict(median=bat2[0], min=bat2[1], p90=bat2[2]),
        sequential_search_bow_ms=dict(median=seq[0], min=seq[1], p90=seq[2], calls_per_sample=a.B),
        kernels_only_ms=ms.value / max(cnt.value, 1), kernel_samples=int(cnt.value))))


if __name__ == "__main__":
    main()
