#!/usr/bin/env python3
"""Times Sim3Solver: every RANSAC hypothesis of every loop candidate in one device call.

Two shapes: B = 3 candidates x n = 100 correspondences x H = 300 hypotheses (a
DetectCommonRegionsFromBoW round) and B = 1 x n = 1000 x H = 300. Per shape: the bare C call
(orbhip_sim3_solve_batch, structs marshalled once), the Python mirror (Sim3Solver.solve_batch plus
iterate to the end), the two kernels alone through the library's stage timer (orbhip_profile_stage
11, in calls of their own), and beside them, in the same run, a numpy-vectorised float32 form of the
same rule on the host (all hypotheses at once: batched eigh, broadcast CheckInliers). Every device
call ends in a stream synchronisation, so the host clock around it covers staging, upload, kernels
and read-back. Each figure is the median of --calls calls after --warmup calls; the C call is taken
in two windows of one run (the second after everything else ran: their spread is the noise).
Prints one JSON line.

    python tools/time_sim3_solver.py [--calls 50] [--warmup 10]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((3, 100, 300, 0.6), (1, 1000, 300, 0.6))   # B, n, H, outlier fraction


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


def numpy_f32(s):
    """The rule in float32, vectorised over the hypotheses (LAPACK's eigh for the eigenvector: the
    counts agree with the device's up to correspondences at a bound) -> n_inliers[H]."""
    F = np.float32
    X1, X2, tri = s["X1"], s["X2"], s["triples"]
    P1, P2 = X1[tri], X2[tri]                              # H x 3 points x 3
    O1, O2 = P1.mean(1, dtype=F), P2.mean(1, dtype=F)
    P1, P2 = P1 - O1[:, None], P2 - O2[:, None]
    M = np.einsum("hki,hkj->hij", P2, P1)
    N = np.empty((len(tri), 4, 4), F)
    N[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    N[:, 0, 1] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    N[:, 1, 2] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    N[:, 2, 3] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    _, v = np.linalg.eigh(N, UPLO="U")
    w, x, y, z = (v[:, k, 3] for k in range(4))            # ascending eigenvalues: the last column
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3).astype(F)
    with np.errstate(all="ignore"):
        P3 = np.einsum("hij,hkj->hki", R, P2)
        sc = np.ones(len(tri), F) if s["fix_scale"] else ((P1 * P3).sum((1, 2)) / (P3 * P3).sum((1, 2))).astype(F)
        sR = sc[:, None, None] * R
        t = O1 - np.einsum("hij,hj->hi", sR, O2)
        Ri = np.swapaxes(R, 1, 2) / sc[:, None, None]
        ti = -np.einsum("hij,hj->hi", Ri, t)

        def proj(cam, X):
            return cam[0] * X[..., 0] / X[..., 2] + cam[2], cam[1] * X[..., 1] / X[..., 2] + cam[3]
        p1u, p1v = proj(s["cam1"], X1)
        p2u, p2v = proj(s["cam2"], X2)
        q1u, q1v = proj(s["cam1"], np.einsum("hij,nj->hni", sR, X2) + t[:, None])
        q2u, q2v = proj(s["cam2"], np.einsum("hij,nj->hni", Ri, X1) + ti[:, None])
        e1 = (p1u - q1u) ** 2 + (p1v - q1v) ** 2
        e2 = (p2u - q2u) ** 2 + (p2v - q2v) ** 2
        return ((e1 < s["max_err1"]) & (e2 < s["max_err2"])).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_sim3_solver: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import Sim3Solver
    from orb_slam3_ros2_amd._lib import Context, Sim3ProblemC, Sim3ResultC, check, lib, ptr
    from orb_slam3_ros2_amd.synthetic import synthetic_sim3_solver_scene
    L = lib()
    ctx = Context()

    def kernels_ms(fn):
        check(L.orbhip_profile_stage(ctx.handle, 11), "orbhip_profile_stage")
        for _ in range(a.calls):
            fn()
        ms, cnt = ctypes.c_double(0), ctypes.c_int32(0)
        check(L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)), "orbhip_profile_collect")
        check(L.orbhip_profile_stage(ctx.handle, 0), "orbhip_profile_stage")
        return ms.value / max(cnt.value, 1)

    rows = []
    for B, n, H, frac in SHAPES:
        scenes = [synthetic_sim3_solver_scene(n, frac, a.seed + b, False, n_hyp=H, min_inliers=20) for b in range(B)]
        probs, ress = (Sim3ProblemC * B)(), (Sim3ResultC * B)()
        outs = []
        for b, s in enumerate(scenes):
            n_inl, hyp, inl = np.empty(H, np.int32), np.empty((H, 13), np.float32), np.empty(n, np.uint8)
            probs[b] = Sim3ProblemC((ctypes.c_float * 4)(*s["cam1"]), (ctypes.c_float * 4)(*s["cam2"]), n, ptr(s["X1"]),
                                    ptr(s["X2"]), ptr(s["max_err1"]), ptr(s["max_err2"]), 0, s["min_inliers"], H,
                                    ptr(s["triples"]))
            ress[b].n_inliers, ress[b].hyp, ress[b].inliers = ptr(n_inl), ptr(hyp), ptr(inl)
            outs.append((n_inl, hyp, inl))

        def bare():
            return check(L.orbhip_sim3_solve_batch(ctx.handle, probs, B, ress), "orbhip_sim3_solve_batch")

        def mirror():
            ms = [Sim3Solver(s["X1"], s["X2"], s["octaves1"], s["octaves2"], s["level_sigma2"], s["level_sigma2"],
                             s["cam1"], s["cam2"], False, s["indices1"], s["n1"], ctx=ctx) for s in scenes]
            for m in ms:
                m.SetRansacParameters(0.99, 20, H)
            Sim3Solver.solve_batch(ms, [s["triples"] for s in scenes])
            return [m.iterate(H)[4] for m in ms]

        def host():
            return [numpy_f32(s) for s in scenes]

        nconv = bare()
        counts = host()
        differ = sum(int((c != o[0]).sum()) for c, o in zip(counts, outs))
        row = dict(B=B, n=n, H=H, converged=nconv, first=[int(r.converged) for r in ress],
                   numpy_counts_that_differ=differ,
                   c_call_ms=median_ms(bare, a.calls, a.warmup), mirror_call_ms=median_ms(mirror, a.calls, a.warmup),
                   numpy_f32_ms=median_ms(host, a.calls, a.warmup), kernels_only_ms=kernels_ms(bare),
                   c_call_again_ms=median_ms(bare, a.calls, 2))
        rows.append(row)
    print(json.dumps(dict(tool="time_sim3_solver", device=torch.cuda.get_device_name(0), calls=a.calls, shapes=rows)))


if __name__ == "__main__":
    main()
