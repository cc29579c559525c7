#!/usr/bin/env python3
"""Times TwoViewReconstruction: both RANSACs, the model choice and the motion recovery of every
frame pair in one device call.

Five shapes: B = 1 and B = 16 frame pairs x N = 300 and N = 1500 matches, and one pair of N = 8192
(the envelope's edge), 200 hypotheses per model.
Per shape: the bare C call (orbhip_two_view_reconstruct_batch, structs marshalled once), the Python
class (TwoViewReconstruction.reconstruct_batch) and the four kernels alone through the library's
stage timer (orbhip_profile_stage 16, in calls of their own). Every device call ends in a stream
synchronisation, so the host clock around it covers the host-side Normalize, staging, upload,
kernels and read-back. Each figure is the median of --calls calls after --warmup calls; the C call
is taken in two windows of one run (the second after everything else ran: their spread is the
noise). There is no CPU baseline: the project has no host implementation of this call outside the
test suite's numpy restatement. Prints one JSON line.

    python tools/time_two_view.py [--calls 50] [--warmup 10]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((1, 300), (16, 300), (1, 1500), (16, 1500), (1, 8192))   # B, N; the last is the envelope's edge
HYP = 200


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
        sys.exit("time_two_view: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import TwoViewReconstruction
    from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, TwoViewProblemC, TwoViewResultC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_two_view_scene
    L = lib()
    ctx = Context()

    def kernels_ms(fn):
        check(L.orbhip_profile_stage(ctx.handle, 16), "orbhip_profile_stage")
        for _ in range(a.calls):
            fn()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
        return ms.value / max(cnt.value, 1)

    rows = []
    for B, n in SHAPES:
        scenes = [synthetic_two_view_scene("general", n=n, seed=a.seed + b, n_hyp=HYP, unmatched_frac=0.5) for b in range(B)]
        probs, ress = (TwoViewProblemC * B)(), (TwoViewResultC * B)()
        keep = []
        for b, s in enumerate(scenes):
            k1, k2 = np.zeros(len(s["kps1"]), KP_DTYPE), np.zeros(len(s["kps2"]), KP_DTYPE)
            k1["x"], k1["y"], k2["x"], k2["y"] = s["kps1"][:, 0], s["kps1"][:, 1], s["kps2"][:, 0], s["kps2"][:, 1]
            p3d, tri = np.empty((len(k1), 3), np.float32), np.empty(len(k1), np.uint8)
            probs[b] = TwoViewProblemC(len(k1), len(k2), ptr(k1), ptr(k2), ptr(s["matches12"]),
                                       (ctypes.c_float * 4)(*s["K"]), 1.0, HYP, ptr(s["sets"]))
            ress[b].p3d, ress[b].triangulated = ptr(p3d), ptr(tri)
            keep.append((k1, k2, p3d, tri))

        def bare():
            return check(L.orbhip_two_view_reconstruct_batch(ctx.handle, probs, B, ress),
                         "orbhip_two_view_reconstruct_batch")

        tvs = [TwoViewReconstruction(s["K"], 1.0, HYP, ctx=ctx) for s in scenes]
        pairs = [(k[0], k[1], s["matches12"], s["sets"]) for k, s in zip(keep, scenes)]

        def mirror():
            return TwoViewReconstruction.reconstruct_batch(tvs, pairs)

        nok = bare()
        row = dict(B=B, N=n, H=HYP, succeeded=nok, models=[int(r.model) for r in ress],
                   c_call_ms=median_ms(bare, a.calls, a.warmup), python_call_ms=median_ms(mirror, a.calls, a.warmup),
                   kernels_only_ms=kernels_ms(bare), c_call_again_ms=median_ms(bare, a.calls, 2),
                   cpu_baseline="no CPU baseline")
        rows.append(row)
    print(json.dumps(dict(tool="time_two_view", device=torch.cuda.get_device_name(0), calls=a.calls, shapes=rows)))


if __name__ == "__main__":
    main()
