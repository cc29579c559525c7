#!/usr/bin/env python3
"""Times the stereo frame calls for one pair: orbhip_extract_stereo_device (P = 1), the extraction
it contains (orbhip_extract_batch_device with B = 2 and vLappingArea {0, 0}) on the same tensors, and
the host form (orbhip_extract_stereo through the Python mirror, upload and read-back included). The
device calls are timed as `reps` back-to-back calls on one stream ending in one synchronisation
(host clock, per call), the two alternating over `rounds` rounds; their difference is the stereo
stage (k_stereo_match + k_stereo_median behind the extraction). Prints one JSON line.

    python tools/time_stereo.py [--w 640] [--h 480] [--reps 200] [--rounds 7] [--seed 6]
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
    return dict(median=float(np.median(t)), min=float(t.min()), max=float(t.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--w", type=int, default=640)
    ap.add_argument("--h", type=int, default=480)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--seed", type=int, default=6)
    ap.add_argument("--bf", type=float, default=60.0)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("time_stereo: needs a GPU (no fallback)")
    from orb_slam3_ros2_amd import ORBextractor, stereo_frame
    from orb_slam3_ros2_amd.stereo import extract_stereo_device
    from orb_slam3_ros2_amd.synthetic import synthetic_stereo_pair
    left, right = synthetic_stereo_pair(a.seed, a.w, a.h)
    ext = ORBextractor(1000, 1.2, 8, 20, 7)
    dev = torch.device("cuda:0")
    cap = ext.max_keypoints(a.w, a.h)
    fr = torch.from_numpy(np.stack([left, right])).to(dev)
    kps = torch.zeros((2, cap, 6), dtype=torch.float32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(2, dtype=torch.int32, device=dev)
    mono = torch.zeros(2, dtype=torch.int32, device=dev)
    u = torch.zeros((1, cap), dtype=torch.float32, device=dev)
    z = torch.zeros((1, cap), dtype=torch.float32, device=dev)
    ns = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()

    def stereo_call():
        extract_stereo_device(ext, fr, a.bf, 1.0, kps, desc, n, mono, u, z, ns, stream=stream)

    def extract_call():
        ext.extract_batch_device(fr, kps, desc, n, mono, (0, 0), stream=stream)

    def window(fn):
        stream.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        stream.synchronize()
        return (time.perf_counter() - t0) * 1e3 / a.reps

    for fn in (stereo_call, extract_call):
        for _ in range(20):
            fn()
    stream.synchronize()
    f = stereo_frame(ext, left, right, a.bf, 1.0)
    assert int(ns[0]) == f.n_stereo and int(n[0]) == len(f.mvKeys)
    ts, te, th = [], [], []
    for _ in range(a.rounds):
        ts.append(window(stereo_call))
        te.append(window(extract_call))
    for _ in range(5):
        stereo_frame(ext, left, right, a.bf, 1.0)
    for _ in range(50):
        t0 = time.perf_counter()
        stereo_frame(ext, left, right, a.bf, 1.0)
        th.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps(dict(
        tool="time_stereo", device=torch.cuda.get_device_name(0), w=a.w, h=a.h, reps=a.reps, rounds=a.rounds,
        n_left=len(f.mvKeys), n_right=len(f.mvKeysRight), n_stereo=f.n_stereo,
        stereo_device_call_ms=stats(ts), extract_batch2_call_ms=stats(te),
        stereo_stage_ms=stats(np.array(ts) - np.array(te)), host_form_python_ms=stats(th))))


if __name__ == "__main__":
    main()
