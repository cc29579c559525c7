#!/usr/bin/env python3
"""Times the three per-frame tracking calls on a rectified-stereo Frame and, in the same run, the
monocular call on the same scene with u_right dropped: SearchByProjection(CurrentFrame, LastFrame)
and SearchLocalPoints at 1250 keypoints x 1000 map points, one frame's PoseOptimization at 600
correspondences (15 % mismatches, about half of them stereo edges). Host buffers in and out, the
host clock around `reps` calls, stereo and monocular alternating over `rounds` rounds. The scenes are
the stereo generators' (synthetic_stereo_projection_scene, level_frac 0: the map points of the
benchmark's scene). Two more pairs time SearchLocalPoints through the C entries with preallocated
outputs (no Python marshalling): the stereo entry with and without its mTrackProjXR output
(proj_xr NULL) against the monocular entry. Prints one JSON line.

    python tools/time_stereo_track.py [--reps 50] [--rounds 7] [--motion forward]
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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n-kp", type=int, default=1250)
    ap.add_argument("--n-mp", type=int, default=1000)
    ap.add_argument("--edges", type=int, default=600)
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--motion", default="forward", choices=["forward", "backward", "neutral"])
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_stereo_track: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import ORBmatcher, Optimizer
    from orb_slam3_ros2_amd.matcher import ProjFrame
    from orb_slam3_ros2_amd.optimizer import PoseProblem
    from orb_slam3_ros2_amd.synthetic import synthetic_stereo_pose_problem, synthetic_stereo_projection_scene
    s = synthetic_stereo_projection_scene(n_kp=a.n_kp, n_mp=a.n_mp, seed=a.seed, motion=a.motion, level_frac=0.0)

    def frame(stereo):
        f = ProjFrame(s["kps"], s["desc"], s["pose_q"], s["pose_t"], s["fx"], s["fy"], s["cx"], s["cy"],
                      claimed=s["claimed"])
        if stereo:
            f.u_right, f.bf, f.b = s["u_right"], s["bf"], s["b"]
        return f

    fs, fm = frame(True), frame(False)
    last_pose = (s["last_pose_q"], s["last_pose_t"])
    ps = synthetic_stereo_pose_problem(n=a.edges, outlier_frac=0.15, seed=1000)[0]
    pm = PoseProblem(**{**ps.__dict__, "u_right": None, "bf": 0.0})
    opt = Optimizer()
    m1, m2 = ORBmatcher(0.9, True, ctx=opt.ctx), ORBmatcher(0.8, False, ctx=opt.ctx)
    calls = {
        "search_by_projection_last": (
            lambda: m1.SearchByProjectionLastFrame(fs, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"],
                                                   last_pose=last_pose),
            lambda: m1.SearchByProjectionLastFrame(fm, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"])),
        "search_local_points": (
            lambda: m2.SearchLocalPoints(fs, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"],
                                         s["skip"], th=1.0),
            lambda: m2.SearchLocalPoints(fm, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"],
                                         s["skip"], th=1.0)),
        "pose_optimization": (lambda: opt.PoseOptimization(ps), lambda: opt.PoseOptimization(pm)),
    }

    # SearchLocalPoints through the C entries with preallocated outputs (no Python result arrays):
    # stereo with and without its mTrackProjXR output (proj_xr NULL) against the monocular entry
    import ctypes
    from orb_slam3_ros2_amd._lib import LocalPointsC, lib, ptr
    arrs = [np.ascontiguousarray(s[k]) for k in ("points", "normals", "min_dist", "max_dist", "mp_desc", "skip")]
    lc = LocalPointsC(a.n_mp, *[ptr(x) for x in arrs])
    o_iv, o_lvl, o_m = np.empty(a.n_mp, np.uint8), np.empty(a.n_mp, np.int32), np.empty(a.n_mp, np.int32)
    o_xr = np.empty(a.n_mp, np.float32)
    sc, mc = fs.to_c_stereo(), fm.to_c()

    def local_c_stereo(xr):
        return lambda: lib().orbhip_search_local_points_stereo(opt.ctx.handle, ctypes.byref(sc), ctypes.byref(lc), 0.5,
                                                               1.0, 0.8, 0, 0.0, ptr(o_iv), ptr(o_lvl), xr, ptr(o_m))

    def local_c_mono():
        return lib().orbhip_search_local_points(opt.ctx.handle, ctypes.byref(mc), ctypes.byref(lc), 0.5, 1.0, 0.8, 0,
                                                0.0, ptr(o_iv), ptr(o_lvl), ptr(o_m))

    calls["search_local_points_c_entry"] = (local_c_stereo(ptr(o_xr)), local_c_mono)
    calls["search_local_points_c_entry_no_proj_xr"] = (local_c_stereo(None), local_c_mono)

    def window(fn):
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    out = dict(tool="time_stereo_track", device=torch.cuda.get_device_name(0), reps=a.reps, rounds=a.rounds,
               n_kp=a.n_kp, n_mp=a.n_mp, edges=a.edges, stereo_edges=int((ps.u_right >= 0).sum()), motion=a.motion,
               keypoints_with_right=int((s["u_right"] > 0).sum()))
    for name, (stereo, mono) in calls.items():
        for fn in (stereo, mono):
            for _ in range(10):
                fn()
        ts, tm = [], []
        for _ in range(a.rounds):
            ts.append(window(stereo))
            tm.append(window(mono))
        out[name + "_stereo_ms"] = stats(ts)
        out[name + "_mono_ms"] = stats(tm)
    rs, rm = calls["search_by_projection_last"][0](), calls["search_by_projection_last"][1]()
    out["last_matches_stereo_mono"] = [int(rs[0]), int(rm[0])]
    ls, lm = calls["search_local_points"][0](), calls["search_local_points"][1]()
    out["local_matches_stereo_mono"] = [int(ls[0]), int(lm[0])]
    qs, qm = calls["pose_optimization"][0](), calls["pose_optimization"][1]()
    out["pose_inliers_trials_stereo_mono"] = [[qs.n_inliers, qs.lm_trials], [qm.n_inliers, qm.lm_trials]]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
