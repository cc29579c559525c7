#!/usr/bin/env python3
"""Times the C4-size LocalBundleAdjustment (50 KF / 2000 points / 8000 observations) as a stereo
problem (about stereo_frac of its observations EdgeStereoSE3ProjectXYZ edges, through
orbhip_ba_solve_stereo) and, in the same run, the same problem without its right coordinates
(orbhip_ba_solve). Host buffers in and out, the host clock around `reps` solves, stereo and
monocular alternating over `rounds` rounds. The two problems run different numbers of LM trials, so
the figure to compare is ms per trial. Prints one JSON line.

    python tools/time_stereo_lba.py [--reps 20] [--rounds 7] [--stereo-frac 0.7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(t):
    t = np.array(t)
    return dict(median=round(float(np.median(t)), 4), min=round(float(t.min()), 4), max=round(float(t.max()), 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n-kf", type=int, default=50)
    ap.add_argument("--n-pts", type=int, default=2000)
    ap.add_argument("--stereo-frac", type=float, default=0.7)
    ap.add_argument("--seed", type=int, default=7)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_stereo_lba: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.synthetic import synthetic_stereo_ba_problem
    ps, _ = synthetic_stereo_ba_problem(n_kf=a.n_kf, n_pts=a.n_pts, seed=a.seed, stereo_frac=a.stereo_frac)
    pm = ps.mono()
    opt = Optimizer()
    stereo, mono = (lambda: opt.LocalBundleAdjustment(ps)), (lambda: opt.LocalBundleAdjustment(pm))
    for fn in (stereo, mono):
        for _ in range(3):
            fn()

    def window(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    ts, tm = [], []
    for _ in range(a.rounds):
        ts.append(window(stereo))
        tm.append(window(mono))
    rs, rm = stereo(), mono()
    out = dict(tool="time_stereo_lba", device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds,
               n_kf=a.n_kf, n_pts=a.n_pts, edges=int(ps.edge_pose.shape[0]),
               stereo_edges=int((ps.edge_ur >= 0).sum()), stereo_ms=stats(ts), mono_ms=stats(tm),
               stereo_trials=rs.lm_trials, mono_trials=rm.lm_trials,
               stereo_iterations=rs.iterations_done, mono_iterations=rm.iterations_done,
               stereo_ms_per_trial=round(float(np.median(ts)) / max(rs.lm_trials, 1), 4),
               mono_ms_per_trial=round(float(np.median(tm)) / max(rm.lm_trials, 1), 4),
               stereo_chi2=[round(rs.initial_chi2, 1), round(rs.final_chi2, 1)],
               mono_chi2=[round(rm.initial_chi2, 1), round(rm.final_chi2, 1)])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
