#!/usr/bin/env python3
"""bench.py — headline benchmark of the MI355X ORB front-end + BA back-end.

BASELINE.json metric: "frames/sec ORB extract+match @640x480; KF/sec LocalBA (50 KF, 2k pts)".

Workload of `value` (configs[1]): one step = ONE 640x480 synthetic frame (device-resident)
through the full ORBextractor::operator() path (8 levels, 1000 features, FAST 20/7, octree,
IC_Angle, rBRIEF) plus the brute-force Hamming match against the previous frame (TH_LOW 50,
ratio 0.9, rotation check) — batch 1, the tracking-thread regime. value = frames/s summed over
ranks (weak scaling: every rank streams its own frames, no collective on the data path).

A plain run sets up the camera streams, warms up, times the K steps, writes the last step's
outputs when --dump-outputs DIR is given, and prints the headline line. Everything else is
behind --full, as extra entries of the same JSON object (rank 0): the strict batch-1 and
one-camera figures, C3 (1280x720 batch 64 extract + 63-pair match),
C4 LocalBundleAdjustment (50 KF / 2000 pts / 8000 obs, 10 LM iterations, host API incl.
H2D/D2H) in LBA/s == KF/s, C5, the 8f rows, the roofline of the dominant kernel measured live
with HIP events on its launch stream, and the CPU baseline (oracle/ restatement timed on this
host's cores).

Usage: python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]
(torchrun for N > 1)
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec
STAGES = {1: "pyramid (k_pyr_cone | 7x k_resize)", 2: "k_fast_cells", 3: "k_octree", 4: "rBRIEF (k_desc_kp | k_desc)",
          5: "match (k_match_fused | k_match_top2)", 6: "k_match_finish"}


def kernel_symbol(stage, batch):
    """The kernel a stage launches at this batch size (liborbhip picks the small-batch variants
    while B x tiles / keypoints leave the chip idle: orbhip_api.cpp run_extract, launch_desc)."""
    small = batch <= 4
    return {1: "k_pyr_cone" if small else "k_resize", 2: "k_fast_cells", 3: "k_octree",
            4: "k_desc_kp" if small else "k_desc", 5: "k_match_fused" if small else "k_match_top2",
            6: "k_match_finish"}[stage]


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200, help="timed steps (one frame per camera each)")
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (every camera's keypoints, descriptors and "
                         "matches) as DIR/<name>.npy (float32; rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline also measure the stage replay and roofline, the batch-1 and "
                         "one-camera figures, C3 / C4 / C5 / 8f and the CPU baselines (the options below)")
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline leg")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the C3 / LBA extra lines")
    ap.add_argument("--c3-steps", type=int, default=10)
    ap.add_argument("--c3-inflight", type=int, default=8,
                    help="C3 batches in flight (each its own context and stream)")
    ap.add_argument("--lba-steps", type=int, default=20)
    ap.add_argument("--lba-batch", type=int, default=256)
    ap.add_argument("--gba-iters", type=int, default=10)
    ap.add_argument("--cameras", type=int, default=16,
                    help="independent C2 camera streams per GPU (the CPU baseline runs 16 frame streams)")
    ap.add_argument("--inflight", type=int, default=1,
                    help="frames in flight per camera (pipelined batch-1 frames; 1 = frame by frame)")
    ap.add_argument("--extra-timeout", type=float, default=240.0,
                    help="seconds for the extras (C3/C4/C5/8f) before the watchdog prints the headline")
    ap.add_argument("--detail", default=os.path.join("gpurun_out", "bench_detail.json"),
                    help="file for the full record (counters, stage tables); '' for none")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


# ORBHIP_BENCH_REHEARSAL=1: the N-rank flow on fewer GPUs than ranks (ranks share GPUs by LOCAL_RANK
# modulo the device count; the bench's own collectives over gloo on the host; the C5 solve as
# replicas, since RCCL refuses two ranks on one GPU). A rehearsal of the multi-rank code paths on a
# one-GPU box, never a measurement.
REHEARSAL = os.environ.get("ORBHIP_BENCH_REHEARSAL", "0") == "1"


def _dist_setup(args):
    import torch
    ws = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if ws > 1:
        import torch.distributed as dist
        if REHEARSAL:
            local %= torch.cuda.device_count()
            torch.cuda.set_device(local)
            dist.init_process_group("gloo")
        else:
            torch.cuda.set_device(local)
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    else:
        torch.cuda.set_device(0)
    return ws, rank, local


def _barrier(ws):
    import torch
    if ws > 1:
        import torch.distributed as dist
        dist.barrier()
    torch.cuda.synchronize()


def _all_reduce_value(v: float, op) -> float:
    import torch
    import torch.distributed as dist
    t = torch.tensor([v], dtype=torch.float64, device="cpu" if REHEARSAL else "cuda")
    dist.all_reduce(t, op=op)
    return float(t.item())


def _max_over_ranks(ws, v: float) -> float:
    if ws == 1:
        return v
    import torch.distributed as dist
    return _all_reduce_value(v, dist.ReduceOp.MAX)


def _sum_over_ranks(ws, v: float) -> float:
    if ws == 1:
        return v
    import torch.distributed as dist
    return _all_reduce_value(v, dist.ReduceOp.SUM)


def make_stream_frames(n, w, h, seed0):
    """A panning camera over one static scene, SURVEY.md 8d image statistics at every frame
    (synthetic.synthetic_stream)."""
    from orb_slam3_ros2_amd.synthetic import synthetic_stream
    return synthetic_stream(n, w, h, seed0)


class Profiler:
    def __init__(self, ctx):
        from orb_slam3_ros2_amd._lib import lib
        self.L, self.ctx = lib(), ctx

    def select(self, stage):
        self.L.orbhip_profile_stage(self.ctx.handle, int(stage))

    def collect(self):
        ms, n = ctypes.c_double(0), ctypes.c_int32(0)
        self.L.orbhip_profile_collect(self.ctx.handle, ctypes.byref(ms), ctypes.byref(n))
        return ms.value, n.value


# ---------------------------------------------------------------------------------------
# C2: batch-1 stream of 640x480 frames, extract + match to the previous frame
# ---------------------------------------------------------------------------------------
class StreamC2:
    """One camera stream of 640x480 frames, each extracted (batch 1) and matched to the previous
    frame. `inflight` > 1 pipelines the stream: frame k runs on context/stream k % inflight (each
    context owns its device scratch), so frame k+1's extraction overlaps frame k's; a frame's
    match waits on an event for the previous frame's extraction, and a slot's buffers are
    rewritten only after the match that last read them. Every frame is still one batch-1
    extraction plus one pair match."""
    W, H, NF = 640, 480, 32

    def __init__(self, rank, inflight=1, null_stream=False):
        import torch
        from orb_slam3_ros2_amd import ORBextractor
        from orb_slam3_ros2_amd._lib import lib
        self.torch = torch
        self.L = lib()
        self.S = S = max(1, int(inflight))
        self.exts = [ORBextractor(1000, 1.2, 8, 20, 7) for _ in range(S)]
        self.ext = self.exts[0]
        self.cap = self.ext.max_keypoints(self.W, self.H)
        dev = torch.device("cuda")
        self.frames_np = make_stream_frames(self.NF, self.W, self.H, 1000 * rank + 1)
        self.frames = torch.from_numpy(self.frames_np).to(dev)
        # output slots: two suffice for one stream; with S streams, 2S slots put a slot's last
        # cross-stream reader 2S - 1 frames back, so its event is normally complete by reuse
        # time and the host skips the stream wait (a hipStreamWaitEvent costs ~4 us of host time)
        ns = 2 if S == 1 else 2 * S
        self.ns = ns
        self.kps = torch.zeros((ns, self.cap, 6), dtype=torch.float32, device=dev)
        self.desc = torch.zeros((ns, self.cap, 32), dtype=torch.uint8, device=dev)
        self.n = torch.zeros(ns, dtype=torch.int32, device=dev)
        self.mono = torch.zeros(ns, dtype=torch.int32, device=dev)
        self.mm = torch.zeros((ns, 3, self.cap), dtype=torch.int32, device=dev)
        self.nm = torch.zeros(ns, dtype=torch.int32, device=dev)
        # own streams (the launch sequences of repeated frames replay as graphs, graph_cache.h);
        # null_stream: torch's current (HIP null) stream, every launch direct
        if null_stream:
            assert S == 1
            self.streams = [torch.cuda.current_stream()]
        else:
            self.streams = [torch.cuda.Stream() for _ in range(S)]
        self.sts = [ctypes.c_void_p(st.cuda_stream) for st in self.streams]
        self.ev_x = [torch.cuda.Event() for _ in range(ns)]   # extraction of the slot's frame done
        self.ev_m = [torch.cuda.Event() for _ in range(ns)]   # match that read the slot as `prev` done
        self.s = 0
        # device pointers of every slot and frame, resolved once (a tensor view per call costs
        # microseconds of host time, which a pipelined stream would pay per frame)
        self.p_frames = [self.frames[i].data_ptr() for i in range(self.NF)]
        self.p_kps = [self.kps[i].data_ptr() for i in range(ns)]
        self.p_desc = [self.desc[i].data_ptr() for i in range(ns)]
        self.p_n = [self.n[i:].data_ptr() for i in range(ns)]
        self.p_mono = [self.mono[i:].data_ptr() for i in range(ns)]
        self.p_mm = [[self.mm[i, r].data_ptr() for r in range(3)] for i in range(ns)]
        self.p_nm = [self.nm[i:].data_ptr() for i in range(ns)]
        self.handles = [e.ctx.handle for e in self.exts]
        self.ratio = ctypes.c_float(0.9)
        self.extract = self.L.orbhip_extract_batch_device
        self.match = self.L.orbhip_match_frames_device
        torch.cuda.synchronize()   # frames uploaded before the side streams read them

    def step(self):
        k = self.s
        j = k % self.S
        cur, prev = k % self.ns, (k - 1) % self.ns
        c, sp = self.handles[j], self.sts[j]
        if self.S > 1 and k >= self.ns and not self.ev_m[cur].query():
            # slot `cur` was last read (as `prev`) by the match of frame k - ns + 1, on another
            # stream, and that match has not finished yet (its reader as `cur`, frame k - ns,
            # ran on this stream: ordered already)
            self.streams[j].wait_event(self.ev_m[cur])
        rc = self.extract(c, self.p_frames[k % self.NF], 1, self.W, self.H, self.W, self.W * self.H, 0, 1000,
                          self.p_kps[cur], self.p_desc[cur], self.cap, self.p_n[cur], self.p_mono[cur], sp)
        assert rc == 0, rc
        if self.S > 1:
            self.ev_x[cur].record(self.streams[j])
            if k >= 1:
                self.streams[j].wait_event(self.ev_x[prev])
        mm = self.p_mm[cur]
        rc = self.match(c, self.p_kps[prev], self.p_desc[prev], self.p_n[prev], self.p_kps[cur], self.p_desc[cur],
                        self.p_n[cur], self.cap, 50, self.ratio, 1, mm[0], mm[1], mm[2], self.p_nm[cur], sp)
        assert rc == 0, rc
        if self.S > 1:
            self.ev_m[prev].record(self.streams[j])
        self.s += 1

    def last_matches(self):
        return int(self.nm[(self.s - 1) % self.ns].item())

    def stage_bytes(self):
        return stage_bytes(self.ext, self.W, self.H, float(self.n.float().mean().item()) or 1000.0, 1)


class FrontendC2:
    """C2 through the library's front-end (FrameStream, include/orbhip.h orbhip_frontend_*):
    `cameras` independent camera streams, the CPU baseline's layout (one frame stream per
    thread), each a FrameStream with `inflight` frames in flight (1: frame by frame, no event
    hand-offs). One step pushes ONE frame into EVERY camera (round-robin from this host thread),
    so a step is `cameras` frames and a short timed region still runs the pipeline in steady
    state. Every frame: batch-1 ORBextractor::operator() + brute-force match to the same
    camera's previous frame, one C call. The cameras replay the bench's 32-frame stream at
    different phases."""
    W, H, NF = 640, 480, 32

    def __init__(self, rank, inflight=1, cameras=1):
        import torch
        from orb_slam3_ros2_amd.frontend import FrameStream
        self.S, self.C = max(1, int(inflight)), max(1, int(cameras))
        self.fss = [FrameStream(self.W, self.H, self.S, 1000, 1.2, 8, 20, 7, 50, 0.9, True) for _ in range(self.C)]
        self._ext = None
        self.frames_np = make_stream_frames(self.NF, self.W, self.H, 1000 * rank + 1)
        self.frames = torch.from_numpy(self.frames_np).to("cuda")
        p = [self.frames[i].data_ptr() for i in range(self.NF)]
        self.p_frames = [[p[(k + 5 * c) % self.NF] for k in range(self.NF)] for c in range(self.C)]
        self.pushes = [fs.push_ptr for fs in self.fss]
        self.ctx0 = self.fss[0].context(0)
        self.k, self.last = 0, (0, -1)
        torch.cuda.synchronize()

    @property
    def frames_per_step(self):
        return self.C

    @property
    def ext(self):
        """Level tables for the roofline bytes, and the context of the --full extras."""
        if self._ext is None:
            from orb_slam3_ros2_amd import ORBextractor
            self._ext = ORBextractor(1000, 1.2, 8, 20, 7)
        return self._ext

    def push_one(self, c):
        slot = self.pushes[c](self.p_frames[c][self.k % self.NF], self.W)
        if slot < 0:
            raise RuntimeError(f"orbhip_frontend_push: {slot}")
        self.last = (c, slot)

    def step(self):
        """One frame into every camera."""
        for c in range(self.C):
            self.push_one(c)
        self.k += 1

    def last_matches(self):
        c, slot = self.last
        self.fss[c].wait(slot)
        return int(self.fss[c].view(slot)["nmatch"].item())

    def last_outputs(self):
        """What the last step computed, as a caller of the front-end receives it: for every camera
        the slot of its last frame (keypoints (cap, 6): x, y, size, angle, response, octave;
        descriptors (cap, 32), their count n, the mono count) and that frame's match against the
        camera's previous frame (per query, i.e. per keypoint of the previous frame: matched
        index, best and second distance; nmatch).
        Arrays over the cameras; rows past n and queries past the previous frame's n, which the
        library leaves as they were, are written as 0 and -1."""
        import torch
        torch.cuda.synchronize()
        names = ("kps", "desc", "n", "mono", "match", "best", "second", "nmatch")
        out = {k: [] for k in names}
        for fs in self.fss:
            slot = (self.k - 1) % fs.slots
            v = {k: t.cpu().numpy() for k, t in fs.view(slot).items() if k in names}
            n = int(v["n"][0])
            nq = int(fs.view((slot - 1) % fs.slots)["n"].item()) if self.k >= 2 else 0
            v["kps"][:, 5] = v["kps"][:, 5].view(np.int32)   # the record's octave field is an int32
            v["kps"][n:], v["desc"][n:] = 0, 0
            for k in ("match", "best", "second"):
                v[k][nq:] = -1
            for k in names:
                out[k].append(v[k])
        return {k: np.stack(a) for k, a in out.items()}

    def mean_keypoints(self):
        import torch
        torch.cuda.synchronize()
        fs = self.fss[0]
        ns = [int(fs.view(i)["n"].item()) for i in range(min(fs.slots, self.k))]
        return float(np.mean(ns)) if ns else 0.0

    def stage_bytes(self):
        torch_sync()
        self.n_cand = measured_candidates(self.ctx0, self.W, self.H, 1)
        return stage_bytes(self.ext, self.W, self.H, self.mean_keypoints() or 1000.0, 1, self.n_cand)

    def close(self):
        """End the camera streams (the level-table extractor stays)."""
        for fs in self.fss:
            fs.close()
        self.fss, self.pushes = [], []


def measured_candidates(ctx, w, h, frames=1):
    """Mean FAST candidates per frame of the context's last extraction (the octree's input,
    orbhip_test_candidates), None if unavailable."""
    from orb_slam3_ros2_amd._lib import lib
    L = lib()
    try:
        f = L.orbhip_test_candidates
    except AttributeError:
        return None
    f.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    tot, n = 0, ctypes.c_int64(0)
    for i in range(frames):
        if f(ctx.handle, w, h, i, ctypes.byref(n)) != 0:
            return None
        tot += n.value
    return tot / max(1, frames)


def stage_bytes(ext, w, h, n_kp, frames, n_cand=None):
    """Algorithmic HBM bytes per launch of each stage. Pyramid: at batch <= 4 the
    one-launch cone (k_pyr_cone) reads level 0 once and writes levels 1..7 (A0 + sum_{l>=1} A_l;
    its halo recompute stays on chip), the 7-launch k_resize cascade of bigger batches reads level
    l-1 and writes level l (sum A[:-1] + sum A[1:], all 7 launches). FAST reads every level once,
    octree reads its candidates (8 B each, the measured count n_cand of FAST's output) and writes
    kept keypoints (8 B), desc reads a 43x43
    patch + writes kp/desc (56 B), match reads query+train descriptors and writes 3 ints per
    query, rot filter 12 B/kp."""
    info = ext.level_info(w, h)
    A = (info["w"].astype(np.int64) * info["h"]).tolist()
    pyr = sum(A) if frames <= 4 else sum(A[:-1]) + sum(A[1:])
    per = {1: pyr, 2: sum(A), 3: 8.0 * (n_cand if n_cand else 4500) + 8 * n_kp, 4: n_kp * (43 * 43 + 56),
           5: 2 * n_kp * 32 + n_kp * 12, 6: n_kp * 12}
    return {k: v * frames for k, v in per.items()}


def survey_frame_bytes(ext, w, h, n_kp):
    """SURVEY.md §8(d) algorithmic bytes of one frame: the input level read once, every cascaded
    level written once and read once, N keypoint records + descriptors (24 + 32 B) written."""
    info = ext.level_info(w, h)
    A = (info["w"].astype(np.int64) * info["h"]).tolist()
    return float(A[0] + 2 * sum(A[1:]) + 56 * n_kp)


def load_traffic(kernel_name, regime="c2"):
    """HBM bytes per launch of `kernel_name` from the committed PMC summary of the regime
    (profiles/traffic_<regime>.json: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of
    this bench's C2 stream or C3 batch, FETCH_SIZE doubled per the gfx950 correction in
    MI355X_MICROARCH.md); None when no summary is committed."""
    path = os.path.join(ROOT, "profiles", f"traffic_{regime}.json")
    try:
        with open(path) as f:
            d = json.load(f)
        return d["kernels"][kernel_name]["hbm_bytes_per_launch"]
    except (OSError, KeyError, ValueError):
        return None


class BatchC3:
    """C3: 1280x720, a batch of B = 64 consecutive frames of one stream, extracted in one batched
    call and matched pair by pair (i, i+1). With N ranks the batch is cut into contiguous slices
    with a one-frame halo (sharding.frame_slice_with_halo): rank r extracts frames
    [lo, hi_ext) and matches its own pairs; no collective. Every rank holds the same 64 frames."""
    W, H, B = 1280, 720, 64

    def __init__(self, rank=0, ws=1):
        import torch
        from orb_slam3_ros2_amd import ORBextractor, ORBmatcher
        from orb_slam3_ros2_amd.sharding import frame_slice_with_halo
        self.ext = ORBextractor(1000, 1.2, 8, 20, 7)
        self.mt = ORBmatcher(0.9, True, ctx=self.ext.ctx)
        self.cap = self.ext.max_keypoints(self.W, self.H)
        self.lo, self.hi, self.plo, self.phi = frame_slice_with_halo(self.B, rank, ws)
        self.nb = self.hi - self.lo           # frames this rank extracts (halo included)
        self.npairs = self.phi - self.plo      # pairs this rank owns (= nb - 1)
        dev = torch.device("cuda")
        allf = make_stream_frames(self.B, self.W, self.H, 5000)
        self.frames = torch.from_numpy(np.ascontiguousarray(allf[self.lo:self.hi])).to(dev)
        B, cap = max(self.nb, 1), self.cap
        self.kps = torch.zeros((B, cap, 6), dtype=torch.float32, device=dev)
        self.desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
        self.n = torch.zeros(B, dtype=torch.int32, device=dev)
        self.mono = torch.zeros(B, dtype=torch.int32, device=dev)
        self.mm = torch.zeros((3, max(B - 1, 1), cap), dtype=torch.int32, device=dev)
        self.nm = torch.zeros(max(B - 1, 1), dtype=torch.int32, device=dev)
        self.stream = torch.cuda.current_stream()

    def step(self):
        if self.nb <= 0:
            return
        self.ext.extract_batch_device(self.frames, self.kps, self.desc, self.n, self.mono, stream=self.stream)
        if self.nb > 1:
            self.mt.match_pairs_device(self.kps, self.desc, self.n, self.mm[0], self.mm[1], self.mm[2], self.nm,
                                       stream=self.stream)


class PipelinedC3:
    """C3 as a stream of 64-frame batches with `inflight` batches in flight: batch k runs on slot
    k % inflight, each slot a BatchC3 with its own context (scratch), output buffers and HIP
    stream, so one batch's latency-bound stages (octree, matcher, the small pyramid levels)
    overlap the next batch's FAST. A slot's stream is in order, so its buffers are reused only
    after its previous batch."""

    def __init__(self, rank=0, ws=1, inflight=2):
        import torch
        self.slots = [BatchC3(rank, ws) for _ in range(max(1, inflight))]
        for sl in self.slots:
            sl.stream = torch.cuda.Stream()
        self.B, self.k = self.slots[0].B, 0

    def step(self):
        self.slots[self.k % len(self.slots)].step()
        self.k += 1


def torch_sync():
    import torch
    torch.cuda.synchronize()


def timed(ws, fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    _barrier(ws)
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    _barrier(ws)
    return _max_over_ranks(ws, time.perf_counter() - t0)


# ---------------------------------------------------------------------------------------
# CPU baseline: the oracle restatement on this host's cores (bounded sample)
# ---------------------------------------------------------------------------------------
def host_cpus():
    """The host's CPUs: nproc (affinity), the cgroup CPU quota (cpu.max), the CPU model. The
    baseline runs one thread per CPU this process may actually use = min(affinity, quota): on
    the GPU box the container sees 256 hardware threads but its cgroup quota is 16 CPUs, so more
    threads would only be throttled to the same 16 CPUs of time."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, per = f.read().split()[:2]
            if q != "max":
                quota = max(1, int(int(q) // int(per)))
    except (OSError, ValueError):
        pass
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return {"usable": max(1, min(aff, quota or aff)), "nproc": aff, "cgroup_quota_cpus": quota, "model": model}


def cpu_baseline(frames_np, budget_s=12.0):
    """Each CPU thread streams frames exactly like a GPU step: extract frame i, match it to
    frame i-1 (whose extraction was the previous step). frames/s = produced frames / wall."""
    from oracle import pyoracle as O
    O.lib()
    cores = host_cpus()["usable"]
    nf = len(frames_np)

    def stream(start, count):
        _, kp, dp = O.extract(frames_np[start % nf])
        for i in range(1, count + 1):
            _, kc, dc = O.extract(frames_np[(start + i) % nf])
            O.match_bf(dp, kp[:, 3], dc, kc[:, 3], 50, 0.9, True)
            kp, dp = kc, dc
        return count

    t0 = time.perf_counter()
    n1 = 0
    while time.perf_counter() - t0 < budget_s / 4:
        n1 += stream(n1, 4)
    t1 = time.perf_counter() - t0
    single = n1 / t1
    per_thread = max(4, int(1.5 * single))   # ~1.5 s per thread: ~24 CPU-seconds at 16 threads
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        done = sum(ex.map(lambda k: stream(k * 7, per_thread), range(cores)))
    tm = time.perf_counter() - t0
    return dict(value=done / tm, single=single, cores=cores, frames=done + n1, wall=tm + t1)


def cpu_lba(prob, budget_s=8.0):
    from oracle import pyoracle as O
    cores = host_cpus()["usable"]
    t0 = time.perf_counter()
    n1 = 0
    while time.perf_counter() - t0 < budget_s / 4:
        O.ba_solve(prob)
        n1 += 1
    t1 = time.perf_counter() - t0
    total = max(cores, int(budget_s * 0.75 / (t1 / n1)))
    t0 = time.perf_counter()
    with ThreadPoolExecutor(cores) as ex:
        list(ex.map(lambda i: O.ba_solve(prob), range(total)))
    tm = time.perf_counter() - t0
    return dict(value=total / tm, single=n1 / t1, cores=cores, solves=total + n1)


def c5_gba(ws, rank, iters):
    """C5 GlobalBundleAdjustment (400 KF loop, 20k points, 80k obs, 20-KF co-visibility window).
    One GPU: the nested-dissection solve of the reduced camera system (csrc/ba_nd.hip).
    N > 1: c5_gba_ms is the sharded solve (ORBHIP_C5_SHARDED=0 turns it off): the keyframe loop cut
    into N segments, rank r holding segment r's landmarks (sharding.shard_problem_nd); each rank
    factors its interior, the separator system and the pose update are all-reduced over RCCL inside
    the device-driven LM; a segment plan that does not fit (too many ranks for the
    loop) falls back to contiguous landmark shards with the summed reduced camera system (every rank
    solving it by the dissection planned on the ranks' union adjacency, r06). Replicas
    (every rank its own whole GBA) are timed beside it as c5_gba_replica_ms. Time = the median of
    three solves, each the max over the ranks, after one untimed solve."""
    import torch
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.sharding import nd_segments, pose_blocks, shard_problem, shard_problem_nd
    from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem
    prob, _ = synthetic_ba_problem(n_kf=400, n_pts=20000, layout="loop", window=20, seed=11)
    prob.iterations, prob.huber_delta = iters, float(np.sqrt(5.99))   # BundleAdjustment(bRobust)
    opt = Optimizer()

    def run(solve, reps=3):
        # one untimed solve, then the median of `reps` timed ones (each the max over the ranks)
        solve()
        ts = []
        for _ in range(reps):
            _barrier(ws)
            t0 = time.perf_counter()
            r = solve()
            torch.cuda.synchronize()
            _barrier(ws)
            ts.append(_max_over_ranks(ws, time.perf_counter() - t0))
        return r, float(np.median(ts))

    out = {"c5_problem": "400 KF loop / 20000 pts / 80000 obs, n = 2394"}
    sharded = ws > 1 and os.environ.get("ORBHIP_C5_SHARDED", "1") == "1" and not REHEARSAL
    if sharded:
        import torch.distributed as dist
        uid = [Optimizer.comm_unique_id() if rank == 0 else None]
        dist.broadcast_object_list(uid, src=0)
        sopt = Optimizer()
        sopt.comm_init(ws, rank, uid[0])
        if nd_segments(*pose_blocks(prob), ws) is not None:
            shard, pts_sel, _ = shard_problem_nd(prob, rank, ws)
            mode = f"rccl segments x{ws} (interiors per rank, separator system all-reduced)"
        else:
            shard, lo, hi, _ = shard_problem(prob, rank, ws)
            pts_sel = np.arange(lo, hi)
            mode = f"rccl landmark shards x{ws} (reduced camera system all-reduced, replicated dissected solve)"
        r, t = run(lambda: sopt.solve_sharded(shard))
        rr, tr = run(lambda: opt.solve(prob))
        out["c5_gba_replica_ms"] = round(1e3 * tr, 2)
        out["c5_gba_replica_mode"] = f"replicas x{ws} (one GPU per solve, nested dissection)"
        out["c5_gba_scaling_note"] = ("the sharded N-rank time is the driver's first measurement of it: no multi-GPU "
                                      "run was available to this build (DESIGN.md, C5 sharding)")
        # the first multi-rank run checks itself: this rank's sharded result against the one-GPU
        # solve of the whole problem (the same LM on the same data: chi2, poses and the rank's
        # points within the north_star's 1e-4, the LM schedule identical), every rank's verdict
        # AND-ed over the ranks
        out.update(c5_sharded_parity(ws, r, rr, pts_sel))
    else:
        mode = f"replicas x{ws} (one GPU per solve, nested dissection)" if ws > 1 else \
            "one GPU (nested dissection, device-driven LM)"
        r, t = run(lambda: opt.solve(prob))
    out.update({"c5_gba_ms": round(1e3 * t, 2), "c5_gba_iterations": r.iterations_done, "c5_gba_trials": r.lm_trials,
                "c5_gba_chi2": [round(r.initial_chi2, 1), round(r.final_chi2, 1)], "c5_gba_mode": mode})
    return out


def c5_sharded_parity(ws, r, rr, pts_sel, tol=1e-4):
    """Sharded C5 result `r` (this rank's landmarks pts_sel) against the replica `rr` of the whole
    problem. Relative errors: chi2 and the poses (quaternion + translation, against the largest
    magnitude of each), the rank's points; `c5_sharded_parity` is True on every rank only if each
    is within tol and the iteration / trial counts agree."""
    def rel(a, b):
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)) if b.size else 0.0
    errs = {"chi2": rel([r.final_chi2], [rr.final_chi2]), "pose_q": rel(r.pose_q, rr.pose_q),
            "pose_t": rel(r.pose_t, rr.pose_t), "points": rel(r.points, rr.points[pts_sel])}
    sched = r.iterations_done == rr.iterations_done and r.lm_trials == rr.lm_trials
    ok = float(sched and max(errs.values()) <= tol)
    worst = _max_over_ranks(ws, max(errs.values()))
    ok_all = _max_over_ranks(ws, 1.0 - ok) == 0.0
    return {"c5_sharded_parity": bool(ok_all), "c5_sharded_max_rel_err": float(f"{worst:.3g}"),
            "c5_sharded_schedule_equal": bool(_max_over_ranks(ws, 0.0 if sched else 1.0) == 0.0)}


def cpu_gba(iters_sample=3, iters=10):
    """C5 on one core: the oracle GBA (same problem as c5_gba) for the first `iters_sample` LM
    iterations (one trial each on this problem), scaled to the GPU run's `iters` (a full 10-iteration
    oracle solve takes ~22 s on one core)."""
    from oracle import pyoracle as O
    from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem
    prob, _ = synthetic_ba_problem(n_kf=400, n_pts=20000, layout="loop", window=20, seed=11)
    prob.iterations, prob.huber_delta = iters_sample, float(np.sqrt(5.99))
    t0 = time.perf_counter()
    r = O.ba_solve(prob)
    t = time.perf_counter() - t0
    per = t / max(1, int(r["iterations_done"]))
    return {"c5_gba_single_core_ms": round(1e3 * per * iters, 1),
            "c5_gba_single_core_ms_per_iteration": round(1e3 * per, 1),
            "c5_sample": f"oracle GBA (ba_oracle.cpp), C5 problem, first {int(r['iterations_done'])} LM iterations "
                         f"({int(r['lm_trials'])} trials) on one core in {t:.1f}s, scaled to {iters} iterations"}


def _f8_inputs():
    from orb_slam3_ros2_amd.matcher import ProjFrame
    from orb_slam3_ros2_amd.synthetic import synthetic_init_pair, synthetic_pose_problem, synthetic_projection_scene
    probs = [synthetic_pose_problem(n=600, outlier_frac=0.15, seed=1000 + i)[0] for i in range(1024)]
    s = synthetic_projection_scene(n_kp=1250, n_mp=1000, seed=77)
    f = ProjFrame(s["kps"], s["desc"], s["pose_q"], s["pose_t"], s["fx"], s["fy"], s["cx"], s["cy"],
                  claimed=s["claimed"])
    return probs, s, f, synthetic_init_pair(n1=1800, seed=31)


def _kfdb_inputs():
    from orb_slam3_ros2_amd.synthetic import synthetic_kfdb_scene, synthetic_query_bow
    sc = synthetic_kfdb_scene(n_kf=1000, seed=21)
    qbow = synthetic_query_bow(sc, [120, 480, 900], seed=5, keep=0.5)
    con = np.zeros(1000, np.uint8)
    con[sc["covis"][120][sc["covis"][120] >= 0]] = 1
    return sc, qbow, con


def _ms(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return 1e3 * (time.perf_counter() - t0) / reps


def f8_tracking(ctx):
    """SURVEY.md 8f rows on the device (host buffers in and out, PCIe-inclusive): PoseOptimization
    (600 edges, 15% mismatches) single-frame latency and 1024-frame batch rate; the two
    projection-guided searches (1250 keypoints x 1000 map points) per call."""
    from orb_slam3_ros2_amd import ORBmatcher, Optimizer
    probs, s, f, ini = _f8_inputs()
    opt = Optimizer(ctx=ctx)
    out = {"f8_pose_opt_single_ms": round(_ms(lambda: opt.PoseOptimization(probs[0]), 50), 4)}
    opt.PoseOptimization_batch(probs)
    t0 = time.perf_counter()
    opt.PoseOptimization_batch(probs)
    out["f8_pose_opt_batch1024_frames_per_s"] = round(len(probs) / (time.perf_counter() - t0), 1)
    m1, m2 = ORBmatcher(0.9, True), ORBmatcher(0.8, False)
    out["f8_search_by_projection_last_ms"] = round(_ms(lambda: m1.SearchByProjectionLastFrame(
        f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"]), 50), 4)
    out["f8_search_local_points_ms"] = round(_ms(lambda: m2.SearchLocalPoints(
        f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"], th=1.0), 50), 4)
    mi = ORBmatcher(0.9, True, ctx=ctx)
    out["a12_search_for_initialization_ms"] = round(_ms(lambda: mi.SearchForInitialization(*ini, 100), 20), 4)
    from orb_slam3_ros2_amd import KeyFrameDatabase
    sc, qbow, con = _kfdb_inputs()
    db = KeyFrameDatabase(len(sc["bows"]), ctx=ctx)
    for i, b in enumerate(sc["bows"]):
        db.add(i, b)
    qid = iter(range(1, 1 << 30))
    out["f8_kfdb_relocalization_ms"] = round(_ms(lambda: db.DetectRelocalizationCandidates(
        next(qid), qbow, sc["covis"]), 20), 4)
    out["f8_kfdb_nbest_ms"] = round(_ms(lambda: db.DetectNBestCandidates(
        next(qid), qbow, sc["covis"], con, 3, sc["kf_map"], 0), 20), 4)
    db.close()
    out["f8_inputs"] = ("PoseOptimization 600 edges/frame; projection 1250 keypoints x 1000 map points; "
                        "SearchForInitialization 1114 octave-0 queries x 1128 F2 keypoints, window 100; "
                        "KeyFrameDatabase 1000 keyframes (~600 words each), query of 3 places")
    return out


def cpu_f8_tracking():
    """The oracle on one core for the same 8f inputs (ms per frame / per call)."""
    from oracle import pyoracle as O
    probs, s, f, ini = _f8_inputs()
    sc, qbow, con = _kfdb_inputs()
    db = O.KeyFrameDatabase(len(sc["bows"]), 20000)
    for i, b in enumerate(sc["bows"]):
        db.add(i, b)
    qid = iter(range(1, 1 << 30))
    kf = {"f8_kfdb_relocalization_single_core_ms": round(_ms(lambda: db.DetectRelocalizationCandidates(
              next(qid), qbow, sc["covis"]), 20), 4),
          "f8_kfdb_nbest_single_core_ms": round(_ms(lambda: db.DetectNBestCandidates(
              next(qid), qbow, sc["covis"], con, 3, sc["kf_map"], 0), 20), 4)}
    return {**kf, "a12_search_for_initialization_single_core_ms": round(_ms(
                lambda: O.search_for_initialization(*ini, 100, 0.9, True), 20), 4),
            "f8_pose_opt_single_core_ms": round(_ms(lambda: O.pose_optimization(probs[0]), 20), 4),
            "f8_search_by_projection_last_single_core_ms": round(_ms(lambda: O.search_by_projection_last(
                f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"]), 20), 4),
            "f8_search_local_points_single_core_ms": round(_ms(lambda: O.search_local_points(
                f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"], th=1.0,
                nnratio=0.8), 20), 4)}


def load_counters(kernel_name, regime):
    """Instruction-mix counters of `kernel_name` from the committed PMC summary
    (profiles/counters.json, written by tools/prof_summary.py counters from separate rocprofv3
    --pmc passes of this bench): VALU / LDS / MFMA activity per launch and the fraction of the
    chip's issue capacity they used over the kernel's duration; None when not committed."""
    try:
        with open(os.path.join(ROOT, "profiles", "counters.json")) as f:
            return json.load(f)["regimes"][regime].get(kernel_name)
    except (OSError, KeyError, ValueError):
        return None


def _spawn_ranks(args) -> int:
    """--gpus N > 1 without a launcher: start N rank processes through torch.distributed.run
    (one per GPU, 127.0.0.1 rendezvous) as CHILD processes and return their exit code. Runs
    before anything touches the GPU (no exec from a GPU-initialised process)."""
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.call(cmd, env=env)


class Watchdog:
    """Extras (C3/C4/C5/8f) run after the headline is measured. If one of them hangs (an RCCL
    collective across ranks, say), the watchdog prints the line measured so far with the stage
    that timed out and ends the process, so the driver never loses the headline."""

    def __init__(self, out, rank, limit_s, detail=None):
        import threading
        self.out, self.rank, self.stage, self.done, self.detail = out, rank, "", False, detail
        self.t = threading.Timer(limit_s, self._fire)
        self.t.daemon = True
        self.t.start()

    def _fire(self):
        if self.done:
            return
        if self.rank == 0:
            self.out.setdefault("extra", {})["timeout_in"] = self.stage
            print(json.dumps(compact_line(self.out, write_detail(self.out, self.detail))), flush=True)
        os._exit(0)

    def disarm(self):
        self.done = True
        self.t.cancel()


def c2_headline(args, ws, rank):
    """C2 camera streams: K timed steps of one frame per camera, then (--dump-outputs) the last
    step's outputs. Returns the headline figures and the camera streams, still open."""
    import torch
    K, W = args.steps, args.warmup
    c2 = FrontendC2(rank, args.inflight, args.cameras)
    # ---- timed region (no stage timer open: the frames replay as launch graphs) ----
    for _ in range(W):
        c2.step()
    _barrier(ws)
    t0 = time.perf_counter()
    for _ in range(K):
        c2.step()
    t_enq = time.perf_counter() - t0   # host time to submit the frames (no blocking call inside)
    torch.cuda.synchronize()
    _barrier(ws)
    elapsed = _max_over_ranks(ws, time.perf_counter() - t0)
    frames_total = _sum_over_ranks(ws, float(K * c2.frames_per_step))
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, c2.last_outputs())
    r = {"value": frames_total / elapsed, "elapsed": elapsed, "frames_per_step": c2.frames_per_step,
         "cameras": c2.C, "inflight": c2.S, "host_submit_ms_per_frame": 1e3 * t_enq / (K * c2.frames_per_step)}
    return r, c2


def dump_outputs(path, arrays):
    """arrays as path/<name>.npy, float32 (every value is an integer below 2^24 or a float32)."""
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a, dtype=np.float32))


def c2_detail(args, ws, rank, c2, r):
    """--full, after the timed region: a stage replay of the same
    16-camera stream, untimed, in which camera c's contexts time stage (c mod 5) + 1 with the
    stage timer (execution-only: the kernels carry the events, StageTimer in orbhip_kernels.h),
    so every stage's average kernel duration comes from launches under the timed region's own
    concurrency and the dominant kernel is the one rocprofv3's kernel trace of this C2 section
    ranks first; then the strict batch-1 figure (one camera, one frame at a time) and one camera
    with 8 frames in flight. Adds its figures to r and closes the camera streams."""
    import torch
    K, W = args.steps, args.warmup
    seq = FrontendC2(rank, 1, 1)
    # ---- stage replay: K more steps of the same stream, every stage timed on its own cameras ----
    profs = []
    for c, fs in enumerate(c2.fss):
        st = 1 + c % 5   # stages 1..5 (k_match_finish runs only with the unfused matcher)
        for j in range(c2.S):
            p = Profiler(fs.context(j))
            p.select(st)
            profs.append((st, p))
    for _ in range(K):
        c2.step()
    torch.cuda.synchronize()
    acc = {}
    for st, p in profs:
        ms, n = p.collect()
        p.select(0)
        a = acc.setdefault(st, [0.0, 0])
        a[0] += ms
        a[1] += n
    stage_ms = {st: a[0] / a[1] for st, a in sorted(acc.items()) if a[1]}
    dom = max(stage_ms, key=stage_ms.get)
    r.update({"keypoints": c2.mean_keypoints(), "nmatch": c2.last_matches(), "stage_ms": stage_ms, "dom": dom,
              "dom_avg_ms": stage_ms[dom], "dom_n": acc[dom][1]})
    r["dom_bytes"] = c2.stage_bytes()[dom]
    r["octree_candidates_per_frame"] = c2.n_cand
    r["frames_np"] = c2.frames_np
    r["ctx"] = c2.ext.ctx
    r["ext"] = c2.ext
    # the camera streams end here, so that the one-camera figures below run with one camera in the
    # process (the front-end sizes its cone tiles by the number of live streams)
    c2.close()
    # ---- strict batch 1: one camera, one frame at a time on one stream ----
    K1 = max(K, 200)
    for _ in range(W):
        seq.step()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for _ in range(K1):
        seq.step()
    torch.cuda.synchronize()
    r["batch1_ms"] = 1e3 * (time.perf_counter() - t1) / K1
    # per-stage kernel durations of the one-frame stream (informational)
    prof_s = Profiler(seq.ctx0)
    one_ms = {}
    for st in (1, 2, 3, 4, 5):
        prof_s.select(st)
        for _ in range(20):
            seq.step()
        ms, n = prof_s.collect()
        one_ms[st] = ms / max(n, 1)
    prof_s.select(0)
    r["stage_ms_one_frame"] = one_ms
    # ---- one camera, 8 frames in flight (event hand-offs between its contexts) ----
    one = FrontendC2(rank, 8, 1)
    for _ in range(max(W, 16)):
        one.step()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    for _ in range(K1):
        one.step()
    torch.cuda.synchronize()
    r["one_camera_inflight_fps"] = K1 / (time.perf_counter() - t2)
    del one
    return r


SIMDS, CUS = 1024, 256   # MI355X: 256 CUs x 4 SIMDs


def headline_bound(kernel):
    """What bounds the headline kernel, read off its committed counters (profiles/counters.json,
    c2 regime): "latency" when its waves mostly wait and neither VALU nor LDS issue is busy (the
    HBM fraction is still reported as the line's frac), else the busiest issue resource."""
    cn = load_counters(kernel, "c2")
    if not cn:
        return "latency"
    valu, lds = cn.get("valu_issue_frac") or 0.0, cn.get("lds_issue_frac") or 0.0
    if max(valu, lds) >= 0.5:
        return "valu issue" if valu >= lds else "lds issue"
    return "latency"


def issue_roofline(kernel, regime, alg_bytes, avg_ms):
    """Roofline of an extractor kernel against the resource that binds it. HBM: algorithmic bytes
    / the live average duration. Issue: the kernel's wave64 VALU and LDS instruction counts per
    launch (profiles/counters.json, rocprofv3 --pmc of the same workload) over the live duration,
    against the chip's issue rate at the clock those counters saw (busy cycles / duration): a
    wave64 VALU op holds a SIMD for 2 cycles (1024 SIMDs), one LDS instruction per CU per cycle.
    `bound` = the resource with the highest fraction; the other fractions ride along."""
    ach = alg_bytes / (avg_ms * 1e-3) / 1e9
    hbm = {"achieved": round(ach, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5)}
    out = {"kernel": kernel, "bound": "hbm", **hbm, "traffic": load_traffic(kernel, regime),
           "algorithmic_bytes_per_launch": int(alg_bytes), "avg_launch_ms": round(avg_ms, 4)}
    cn = load_counters(kernel, regime)
    out["counters"] = cn
    if cn and cn.get("busy_cycles") and cn.get("duration_us"):
        clk = cn["busy_cycles"] / (cn["duration_us"] * 1e-6)   # Hz
        sec = avg_ms * 1e-3
        valu = cn.get("SQ_INSTS_VALU", 0.0) / sec / 1e9
        lds = cn.get("SQ_INSTS_LDS", 0.0) / sec / 1e9
        vpk, lpk = SIMDS / 2 * clk / 1e9, CUS * clk / 1e9
        fr = {"hbm": ach / HBM_PEAK_GBS, "valu issue": valu / vpk, "lds issue": lds / lpk}
        out["issue"] = {"clock_ghz": round(clk / 1e9, 3),
                        "valu": {"achieved": round(valu, 2), "peak": round(vpk, 1), "unit": "G wave-instr/s",
                                 "frac": round(valu / vpk, 4)},
                        "lds": {"achieved": round(lds, 2), "peak": round(lpk, 1), "unit": "G wave-instr/s",
                                "frac": round(lds / lpk, 4)}}
        b = max(fr, key=fr.get)
        if b != "hbm":
            src = out["issue"]["valu" if b == "valu issue" else "lds"]
            out.update({"bound": b, "achieved": src["achieved"],
                        "peak": src["peak"], "unit": src["unit"], "frac": src["frac"], "hbm": hbm})
    return out


def c3_batch(args, ws, rank):
    """C3 1280x720 B=64 extract + 63 pair matches; N > 1: halo slices (strong scaling of the
    batch). frames/s = 64 x steps / max-over-ranks time."""
    c3 = BatchC3(rank, ws)
    t = timed(ws, c3.step, args.c3_steps, 2)
    pc = PipelinedC3(rank, ws, args.c3_inflight)
    tp = timed(ws, pc.step, args.c3_steps * len(pc.slots), 2 * len(pc.slots))
    out = {"c3_1280x720_b64_extract_match_frames_per_s": round(pc.B * args.c3_steps * len(pc.slots) / tp, 1),
           "c3_batches_in_flight": len(pc.slots),
           "c3_one_batch_at_a_time_frames_per_s": round(c3.B * args.c3_steps / t, 1),
           "c3_partition": f"{ws} contiguous slice(s) + 1-frame halo; rank {rank}: frames [{c3.lo},{c3.hi}), "
                           f"pairs [{c3.plo},{c3.phi})"}
    if rank == 0:
        p3 = Profiler(c3.ext.ctx)
        c3_ms = {}
        for st in (1, 2, 3, 4, 5, 6):
            p3.select(st)
            for _ in range(3):
                c3.step()
            ms, n = p3.collect()
            c3_ms[st] = ms / max(n, 1)
        p3.select(0)
        d3 = max(c3_ms, key=c3_ms.get)
        torch_sync()
        cand3 = measured_candidates(c3.ext.ctx, c3.W, c3.H, c3.nb)
        b3 = stage_bytes(c3.ext, c3.W, c3.H, float(c3.n.float().mean().item()) or 1000.0, c3.nb, cand3)
        out["c3_octree_candidates_per_frame"] = cand3
        ks = kernel_symbol(d3, c3.nb)
        out["c3_roofline"] = issue_roofline(ks, "c3", b3[d3], c3_ms[d3])
        out["c3_roofline"]["stage_avg_ms"] = {STAGES[k]: round(v, 4) for k, v in c3_ms.items()}
        # the extractor's streaming stage against the HBM roof: the 7-level k_resize cascade
        # (level l-1 read, level l written, per frame), timed as one stage (first kernel's start
        # to the last kernel's end: the launch gaps between the 7 kernels are included)
        ah = b3[1] / (c3_ms[1] * 1e-3) / 1e9
        out["c3_hbm_stage"] = {"kernel": kernel_symbol(1, c3.nb), "bound": "hbm", "achieved": round(ah, 1),
                               "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ah / HBM_PEAK_GBS, 4),
                               "algorithmic_bytes_per_stage": int(b3[1]), "stage_ms": round(c3_ms[1], 4)}
    return out


FP64_MFMA_PEAK_TFS = 78.6   # MI355X FP64 matrix peak (AMD spec; the guide lists no fp64 row)


def ba_cholesky_roofline(n, regime):
    """Live fp64 MFMA roofline of the dense Cholesky solve (n^3/3 + 2n^2 flops per LM
    trial): a C4 / C5-sized SPD reduced camera system factored and solved by the persistent DAG
    kernel the LM loop launches (k_chol_dag: one launch per solve, ba_chol_dag.hip), timed with HIP
    events around 20 back-to-back launches. Counters: the same workload's rocprofv3 --pmc passes
    (tools/pmc_workload.py c4 / c5)."""
    from orb_slam3_ros2_amd._lib import lib
    rng = np.random.default_rng(3)
    A = rng.standard_normal((n, n))
    S = A @ A.T / n + np.eye(n) * 2.0
    b = rng.standard_normal(n)
    x = np.zeros(n)
    ms = ctypes.c_float(0)
    rc = lib().orbhip_test_cholesky_dag(S.ctypes.data, b.ctypes.data, x.ctypes.data, n, 20, 0, ctypes.byref(ms),
                                        None)
    if rc != 0:
        return {"error": rc}
    err = float(np.abs(S @ x - b).max() / np.abs(b).max())
    flops = n ** 3 / 3 + 2 * n * n
    ach = flops / (ms.value * 1e-3) / 1e12
    return {"kernel": "k_chol_dag", "bound": "mfma", "achieved": round(ach, 4), "peak": FP64_MFMA_PEAK_TFS,
            "unit": "TFLOP/s", "frac": round(ach / FP64_MFMA_PEAK_TFS, 6), "n": n, "flops_per_launch": int(flops),
            "avg_launch_ms": round(ms.value, 4), "residual": err, "counters": load_counters("k_chol_dag", regime)}


def ba_nd_roofline(reps=20):
    """Live fp64 MFMA roofline of the solve the C5 GBA actually runs: the nested dissection of the
    reduced camera system (csrc/ba_nd.hip) on a C5-structured system (399 optimised poses, cyclic
    co-visibility band w = 19: synthetic.banded_pose_system), with the planner's K. The kernels are
    k_chol_dag_multi (the K interiors' partial factorizations in one launch), k_nd_assemble, the
    separator's k_chol_dag and k_nd_backsolve (+ k_nd_finish); the two halves are timed alone as
    well (HIP events, `reps` solves each). Algorithmic flops of one solve: every
    interior's banded factorization n_I b^2 with b = 6 w, plus its Schur contribution to its two
    separators n_I (2b)^2, plus the separator system's dense Cholesky n_Z^3 / 3 + 2 n_Z^2,
    n_Z = 6 w K; with the second level (K >= 6) the separator part is its own interiors (n_I = b or
    2b, the same banded terms) plus the dense remainder n_Zd = b K / 2. Counters: rocprofv3 --pmc
    passes of tools/pmc_workload.py c5nd."""
    from orb_slam3_ros2_amd._lib import lib
    from orb_slam3_ros2_amd.synthetic import banded_pose_system
    n_pose, w = 399, 19
    A, b, bi, bj = banded_pose_system(n_pose, w, True, seed=1)
    L = lib()
    f = L.orbhip_test_nd_stages
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p] * 4
    x = np.zeros(A.shape[0])
    ms, ku = ctypes.c_float(0), ctypes.c_int(0)
    stage = (ctypes.c_float * 2)()
    seg = (ctypes.c_int * 65)()
    rc = f(A.ctypes.data, b.ctypes.data, x.ctypes.data, n_pose, bi.ctypes.data, bj.ctypes.data, bi.size, 0, reps,
           ctypes.byref(ms), ctypes.byref(ku), stage, seg)
    if rc != 0:
        return {"error": rc}
    K = ku.value
    bw = 6 * w
    n_int = [6 * (seg[r + 1] - seg[r] - w) for r in range(K)]
    n_z = 6 * w * K
    fl_int = sum(ni * bw * bw + ni * (2 * bw) ** 2 for ni in n_int)
    # the second level (ba_nd.hip nd_inner_plan; cyclic, K >= 6, ORBHIP_ND_LEVELS != 1): the even
    # separators are the interiors of the separator system (the last inner segment of an odd K
    # holds two), the K // 2 odd ones its dense part
    two = os.environ.get("ORBHIP_ND_LEVELS", "2") != "1" and K >= 6
    n_int2 = [bw * (2 if (K % 2 and r == K // 2 - 1) else 1) for r in range(K // 2)] if two else []
    n_zd = bw * (K // 2) if two else n_z
    fl_int2 = sum(ni * bw * bw + ni * (2 * bw) ** 2 for ni in n_int2)
    fl_sep = fl_int2 + n_zd ** 3 / 3 + 2 * n_zd * n_zd
    flops = fl_int + fl_sep
    err = float(np.abs(A @ x - b).max() / np.abs(b).max())
    ach = flops / (ms.value * 1e-3) / 1e12
    out = {"kernels": "k_chol_dag_multi + k_nd_assemble + k_chol_dag (separator) + k_nd_backsolve + k_nd_finish",
           "bound": "mfma", "achieved": round(ach, 4), "peak": FP64_MFMA_PEAK_TFS, "unit": "TFLOP/s",
           "frac": round(ach / FP64_MFMA_PEAK_TFS, 6), "n": int(A.shape[0]), "segments": K, "band_poses": w,
           "n_interiors": n_int, "n_separator": n_z, "levels": 2 if two else 1, "n_interiors_level2": n_int2,
           "n_separator_dense": n_zd, "flops_per_solve": int(flops),
           "flops_interiors": int(fl_int), "flops_separator": int(fl_sep), "avg_solve_ms": round(ms.value, 4),
           "interiors_and_assembly_ms": round(stage[0], 4), "separator_and_backsolve_ms": round(stage[1], 4),
           "residual": err, "counters": {k: load_counters(k, "c5nd") for k in
                                         ("k_chol_dag_multi", "k_chol_dag", "k_nd_backsolve", "k_nd_assemble")}}
    return out


def c4_lba(args, ws, rank, ctx):
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem
    out = {}
    opt = Optimizer(ctx=ctx)
    if rank == 0:
        prob, _ = synthetic_ba_problem()
        r = None
        for _ in range(2):
            r = opt.LocalBundleAdjustment(prob)
        t0 = time.perf_counter()
        for _ in range(args.lba_steps):
            r = opt.LocalBundleAdjustment(prob)
        tp = time.perf_counter() - t0
        # the headline: the orbhip_ba_solve call itself on the problem's arrays, as the C++
        # LocalMapping adapter makes it (host preparation, upload, the device LM and the outputs
        # included; the Python layer's per-call marshalling, ~20-60 us, is not on the C++ path and
        # is reported beside it as c4_lba_python_api_ms)
        single = opt.prepare_single(prob)
        for _ in range(2):
            opt.run_single(single)
        t0 = time.perf_counter()
        for _ in range(args.lba_steps):
            r = opt.run_single(single)
        tl = time.perf_counter() - t0
        out.update({"c4_lba_kf_per_s": round(args.lba_steps / tl, 2), "c4_lba_ms": round(1e3 * tl / args.lba_steps, 3),
                    "c4_lba_python_api_ms": round(1e3 * tp / args.lba_steps, 3),
                    "c4_lba_trials": r.lm_trials, "c4_lba_chi2": [round(r.initial_chi2, 3), round(r.final_chi2, 3)]})
    # replicas: independent LBA problems (concurrent maps / agents) in one batched solve per rank
    probs = [synthetic_ba_problem(seed=100 + 1000 * rank + i)[0] for i in range(args.lba_batch)]
    # the batch in C-ABI form (what a C++ host adapter holds); the timed call is orbhip_ba_solve_batch
    # itself: host preparation, H2D of every problem, the solves, D2H and the per-edge outputs
    batch = opt.prepare_batch(probs)
    opt.run_batch(batch)   # warm-up at full size (pinned staging grows once)
    _barrier(ws)
    t0 = time.perf_counter()
    rs = opt.run_batch(batch)
    _barrier(ws)
    tb = _max_over_ranks(ws, time.perf_counter() - t0)
    out["c4_lba_batched_kf_per_s"] = round(_sum_over_ranks(ws, float(len(probs))) / tb, 1)
    out["c4_lba_batch_per_gpu"] = len(probs)
    out["c4_lba_batched_trials_mean"] = round(float(np.mean([x.lm_trials for x in rs])), 2)
    if rank == 0:
        out["c4_roofline"] = ba_cholesky_roofline(294, "c4")
        # a microbenchmark: the dense n = 2394 solve through the plain DAG kernel (C5-sized); the
        # C5 GBA itself runs the nested dissection measured by c5_nd_roofline
        out["c5_dense_solve_microbench"] = ba_cholesky_roofline(2394, "c5")
        out["c5_nd_roofline"] = ba_nd_roofline()
    return out


def main(argv=None):
    args = parse(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(_spawn_ranks(args))
    ws, rank, local = _dist_setup(args)
    if ws != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={ws}")
    r, c2 = c2_headline(args, ws, rank)
    K, W = args.steps, args.warmup
    out = {
        "metric": "frames/sec ORB extract+match @640×480; KF/sec LocalBA (50 KF, 2k pts)",
        "value": round(r["value"], 2),
        "unit": "frames/s",
        "n_gpus": ws,
        "steps": K,
        "warmup": W,
        "ms_per_step": round(1e3 * r["elapsed"] / K, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "u8",
        "data": "synthetic (SURVEY.md 8d rectangles + sigma-4 noise; a camera panning over one static scene, seeded)",
        "config": {"workload": "C2: 640x480, 8-level pyramid, 1000 feat/frame, FAST 20/7, batch=1 per camera stream; "
                               "ORBextractor::operator() + brute-force Hamming match to the camera's previous frame",
                   "step": f"one frame on each of {r['cameras']} independent camera streams",
                   "frames_per_step": r["frames_per_step"],
                   "parallelism": f"replicas x{ws} (no collective); {r['cameras']} camera streams per GPU, batch 1 each",
                   "cameras": r["cameras"], "frames_in_flight_per_camera": r["inflight"],
                   "host_submit_ms_per_frame": round(r["host_submit_ms_per_frame"], 4)},
    }
    detail = None
    if args.full:
        full_record(args, ws, rank, c2, r, out)
        if rank == 0:
            detail = write_detail(out, args.detail)
    else:
        c2.close()
    if rank == 0:
        print(json.dumps(compact_line(out, detail)), flush=True)
    if ws > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


def full_record(args, ws, rank, c2, r, out):
    """--full: everything the bench measures beside the headline, added to `out`: the stage replay
    and roofline of the C2 streams, the batch-1 and one-camera figures, the extras (C5, C3, C4, 8f)
    under a watchdog, and the CPU baselines (one rank, unless --no-cpu)."""
    c2_detail(args, ws, rank, c2, r)
    dom = r["dom"]
    # algorithmic bytes per frame = A0 + 2 sum_{l>=1} A_l + N * 56 (1,649,864 B at
    # 640x480 and N = 1000), one frame per launch of the dominant kernel; the kernel's own bytes
    # (stage_bytes) ride along as kernel_own_bytes
    frame_bytes = survey_frame_bytes(r["ext"], StreamC2.W, StreamC2.H, r["keypoints"] or 1000.0)
    achieved = frame_bytes / (r["dom_avg_ms"] * 1e-3) / 1e9
    own = r["dom_bytes"] / (r["dom_avg_ms"] * 1e-3) / 1e9
    ks = kernel_symbol(dom, 1)
    host = host_cpus()
    out.update({
        "batch1_frames_per_s": round(1e3 / r["batch1_ms"], 1),
        "batch1_latency_ms": round(r["batch1_ms"], 4),
        "roofline": {"kernel": ks, "bound": headline_bound(ks), "achieved": round(achieved, 3), "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6),
                     "traffic": load_traffic(ks, "c2"), "counters": load_counters(ks, "c2"),
                     "algorithmic_bytes_per_launch": int(frame_bytes),
                     "bytes_rule": "SURVEY 8(d): A0 + 2*sum(A_l, l>=1) + N*56 per frame, 1 frame per launch",
                     "kernel_own_bytes": {"bytes": int(r["dom_bytes"]), "achieved": round(own, 3),
                                          "frac": round(own / HBM_PEAK_GBS, 6)},
                     "avg_launch_ms": round(r["dom_avg_ms"], 5),
                     "launches_timed": r["dom_n"],
                     "timing": "kernel execution span from device timestamps (k_pyr_cone: first workgroup "
                               "start -> last workgroup end, s_memrealtime; the other stages: "
                               "hipExtLaunchKernelGGL events) over a replay of the timed 16-camera stream; "
                               "rocprofv3 --kernel-trace of this C2 section: profiles/r05_c2_kernel_stats.md",
                     "octree_candidates_per_frame": r.get("octree_candidates_per_frame"),
                     "stage_avg_ms": {STAGES[k]: round(v, 5) for k, v in r["stage_ms"].items()},
                     "stage_avg_ms_one_frame_stream": {STAGES[k]: round(v, 5)
                                                       for k, v in r["stage_ms_one_frame"].items()}},
    })
    out["config"].update({"batch1_latency_ms": round(r["batch1_ms"], 4),
                          "batch1_frames_per_s": round(1e3 / r["batch1_ms"], 1),
                          "one_camera_8_in_flight_frames_per_s": round(r["one_camera_inflight_fps"], 1),
                          "keypoints_per_frame": round(r["keypoints"], 1), "matches_last_pair": r["nmatch"]})
    if not args.no_extra:
        wd = Watchdog(out, rank, args.extra_timeout, args.detail)
        extra = {}
        for name, fn in (("c5", lambda: c5_gba(ws, rank, args.gba_iters)),
                         ("c3", lambda: c3_batch(args, ws, rank)),
                         ("c4", lambda: c4_lba(args, ws, rank, r["ctx"])),
                         ("f8", lambda: f8_tracking(r["ctx"]) if rank == 0 else {})):
            wd.stage = name
            try:
                extra.update(fn())
            except Exception as e:   # never lose the headline line to an extra
                extra[f"{name}_error"] = repr(e)[:200]
            out["extra"] = extra
        wd.disarm()
    if rank == 0 and ws == 1 and not args.no_cpu:
        cb = cpu_baseline(r["frames_np"])
        out["cpu_baseline"] = {"value": round(cb["value"], 2), "unit": "frames/s", "cores": cb["cores"],
                               "kind": "port",
                               "sample": f"oracle/ C++ restatement (g++ -O3), {cb['frames']} frames of the bench's "
                                         f"640x480 stream, each extract + match to the previous frame, "
                                         f"{cb['cores']} threads (one frame stream per thread), {cb['wall']:.1f}s wall",
                               "host": host,
                               "single_core_value": round(cb["single"], 2)}
        if "extra" in out:
            from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem
            prob, _ = synthetic_ba_problem()
            cl = cpu_lba(prob)
            out["cpu_baseline"]["c4_lba_kf_per_s"] = round(cl["value"], 2)
            out["cpu_baseline"]["c4_lba_single_core_kf_per_s"] = round(cl["single"], 2)
            out["cpu_baseline"]["c4_lba_sample"] = f"{cl['solves']} oracle LBA solves, {cl['cores']} threads"
            out["cpu_baseline"].update(cpu_f8_tracking())
            out["cpu_baseline"].update(cpu_gba(iters=args.gba_iters))
            # C3's workload on the CPU: 1280x720 frames of the same generator, each extracted and
            # matched to the previous one, one frame stream per thread (bounded sample)
            c3f = make_stream_frames(16, BatchC3.W, BatchC3.H, 5000)
            c3c = cpu_baseline(c3f, budget_s=8.0)
            out["cpu_baseline"]["c3_frames_per_s"] = round(c3c["value"], 2)
            out["cpu_baseline"]["c3_single_core_frames_per_s"] = round(c3c["single"], 2)
            out["cpu_baseline"]["c3_sample"] = (f"{c3c['frames']} 1280x720 frames (16-frame stream, seed 5000), each "
                                                f"extract + match to the previous frame, {c3c['cores']} threads, "
                                                f"{c3c['wall']:.1f}s wall")


def write_detail(out, path):
    """The full record (every counter dict, per-stage timings, samples) goes to a file; the
    printed line keeps the figures (the driver reads only the last ~4 KB of stdout)."""
    if not path:
        return None
    try:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(out, f, indent=1)
        return os.path.relpath(os.path.abspath(path), ROOT)
    except OSError:
        return None


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def compact_line(out, detail):
    """The one JSON line rank 0 prints: the contract fields, the headline roofline and CPU
    baseline, and every extra figure (C3, C4, C5, 8f), without the PMC counter dicts and stage
    tables (those are in `detail` and profiles/counters.json)."""
    line = {k: v for k, v in out.items() if k not in ("roofline", "extra", "cpu_baseline", "config")}
    cfg = out["config"]
    line["config"] = _pick(cfg, ("workload", "step", "frames_per_step", "parallelism", "cameras",
                                 "one_camera_8_in_flight_frames_per_s", "keypoints_per_frame"))
    rf = out.get("roofline")
    if rf is not None:
        line["roofline"] = _pick(rf, ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic",
                                      "algorithmic_bytes_per_launch", "bytes_rule", "avg_launch_ms", "launches_timed",
                                      "kernel_own_bytes"))
    ex = out.get("extra")
    if ex is not None:
        e = {}
        for k, v in ex.items():
            if not isinstance(v, (dict, list)) and k not in ("c3_partition", "f8_inputs", "c5_problem",
                                                             "c5_gba_scaling_note", "c3_octree_candidates_per_frame",
                                                             "c4_lba_batch_per_gpu", "c4_lba_batched_trials_mean",
                                                             "c5_gba_iterations", "c3_batches_in_flight"):
                e[k] = v
        rk = ("kernel", "bound", "frac", "avg_launch_ms")
        for k in ("c3_roofline", "c3_hbm_stage", "c4_roofline", "c5_dense_solve_microbench"):
            if isinstance(ex.get(k), dict):
                e[k] = _pick(ex[k], rk + ("stage_ms",))
        if isinstance(ex.get("c5_nd_roofline"), dict):
            e["c5_nd_roofline"] = _pick(ex["c5_nd_roofline"], ("bound", "frac", "avg_solve_ms"))
        if "c5_gba_chi2" in ex:
            e["c5_gba_chi2"] = ex["c5_gba_chi2"]
        line["extra"] = e
    cb = out.get("cpu_baseline")
    if cb is not None:
        c = {k: v for k, v in cb.items() if not isinstance(v, dict) and not k.endswith("_sample")
             and k != "sample"}
        c["sample"] = f"oracle/ (g++ -O3), {cb.get('cores')} threads; bounded samples (see detail)"
        c["host_cpu"] = cb.get("host", {}).get("model", "")
        line["cpu_baseline"] = c
    line["detail"] = detail
    return line


if __name__ == "__main__":
    main()
