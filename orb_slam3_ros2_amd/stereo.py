"""Rectified-stereo frames (U:src/Frame.cc, the stereo constructor) over liborbhip.so: both
ExtractORB calls with vLappingArea {0, 0} and Frame::ComputeStereoMatches in one call.

    ext = ORBextractor(1000, 1.2, 8, 20, 7)
    f = stereo_frame(ext, left, right, bf=mbf, b=mb)        # -> StereoFrame
    f.mvKeys, f.mDescriptors, f.mvKeysRight, f.mDescriptorsRight, f.mvuRight, f.mvDepth

``extract_stereo_device`` is the device-resident form for torch-ROCm tensors (P pairs per call,
asynchronous on a stream).
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._lib import KP_DTYPE, OrbHipError, StereoParams, check, lib, ptr, torch_stream

# the per-keypoint status of ComputeStereoMatches (include/orbhip.h)
STATUS = {1: "accepted", 2: "no candidate row / maxU < 0", 3: "descriptor distance", 4: "iniu / endu",
          5: "best SAD at +-L", 6: "deltaR", 7: "disparity", 8: "median cut", 9: "window or octave guard"}


@dataclass
class StereoFrame:
    mvKeys: np.ndarray              # KP_DTYPE, left
    mDescriptors: np.ndarray        # [N, 32] u8
    mvKeysRight: np.ndarray
    mDescriptorsRight: np.ndarray
    mvuRight: np.ndarray            # [N] float32, -1 where there is no stereo match
    mvDepth: np.ndarray             # [N] float32, -1 likewise
    status: np.ndarray              # [N] int32 (STATUS)
    n_stereo: int


def stereo_frame(ext, left, right, bf: float, b: float, center_patch: bool = False) -> StereoFrame:
    """Frame(imLeft, imRight, ...) up to mvuRight / mvDepth. ``ext`` is an ORBextractor (both
    sides use its parameters); left / right are 2-D uint8 arrays of one size."""
    left = np.ascontiguousarray(left, dtype=np.uint8)
    right = np.ascontiguousarray(right, dtype=np.uint8)
    if left.ndim != 2 or left.shape != right.shape:
        raise OrbHipError(-1, "stereo expects two CV_8UC1 images of one size")
    h, w = left.shape
    cap = ext.max_keypoints(w, h)
    kl, kr = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
    dl, dr = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
    u = np.zeros(cap, np.float32)
    z = np.zeros(cap, np.float32)
    st = np.zeros(cap, np.int32)
    nl, nr, ns = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    prm = StereoParams(float(bf), float(b), int(bool(center_patch)))
    check(lib().orbhip_extract_stereo(ext.ctx.handle, ptr(left), ptr(right), w, h, w, ctypes.byref(prm), ptr(kl),
                                      ptr(dl), ctypes.byref(nl), ptr(kr), ptr(dr), ctypes.byref(nr), cap, ptr(u),
                                      ptr(z), ptr(st), ctypes.byref(ns)), "orbhip_extract_stereo")
    a, c = nl.value, nr.value
    return StereoFrame(kl[:a].copy(), dl[:a].copy(), kr[:c].copy(), dr[:c].copy(), u[:a].copy(), z[:a].copy(),
                       st[:a].copy(), ns.value)


def extract_stereo_device(ext, frames, bf: float, b: float, kps_out, desc_out, n_out, mono_out, u_right_out,
                          depth_out, n_stereo_out, status_out=None, center_patch: bool = False, stream=None):
    """frames: uint8 CUDA tensor [2P, H, W], frame 2p the left and 2p + 1 the right image of pair p
    (rows may be padded: any byte alignment of the view, stride(1) >= W, stride(0) >= stride(1) * H;
    of each row only the first W bytes are read, plus padding up to the next 4-byte boundary when
    that boundary lies within stride(1), and nothing past the last row, as include/orbhip.h states
    for orbhip_extract_batch_device). kps_out / desc_out / n_out / mono_out as ORBextractor.extract_batch_device
    takes them for 2P frames (cap = desc_out.shape[1] >= ext.max_keypoints(W, H)); u_right_out /
    depth_out float32 [P, cap], status_out int32 [P, cap] or None, n_stereo_out int32 [P].
    Asynchronous on ``stream`` (torch stream or None); entries at or past a left frame's keypoint
    count are left untouched."""
    B, H, W = frames.shape
    if B < 2 or B % 2:
        raise OrbHipError(-1, "extract_stereo_device expects an even number of frames")
    cap = desc_out.shape[1]
    prm = StereoParams(float(bf), float(b), int(bool(center_patch)))
    check(lib().orbhip_extract_stereo_device(ext.ctx.handle, ptr(frames), B // 2, W, H, frames.stride(1),
                                             frames.stride(0), ctypes.byref(prm), ptr(kps_out), ptr(desc_out), cap,
                                             ptr(n_out), ptr(mono_out), ptr(u_right_out), ptr(depth_out),
                                             ptr(status_out), ptr(n_stereo_out), torch_stream(stream)),
          "orbhip_extract_stereo_device")


def stereo_match_raw(ctx, left, right, kps_l, desc_l, kps_r, desc_r, bf, b, center_patch=False):
    """Test hook (orbhip_test_stereo_match): the stereo kernels alone on the given keypoints.
    -> (u_right, depth, status, best_r, sad, n_stereo)."""
    left = np.ascontiguousarray(left, dtype=np.uint8)
    right = np.ascontiguousarray(right, dtype=np.uint8)
    h, w = left.shape
    kl, kr = np.ascontiguousarray(kps_l, KP_DTYPE), np.ascontiguousarray(kps_r, KP_DTYPE)
    dl = np.ascontiguousarray(desc_l, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(desc_r, np.uint8).reshape(-1, 32)
    n = len(kl)
    u, z = np.zeros(n, np.float32), np.zeros(n, np.float32)
    st, br, sad = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    ns = ctypes.c_int(0)
    prm = StereoParams(float(bf), float(b), int(bool(center_patch)))
    check(lib().orbhip_test_stereo_match(ctx.handle, ptr(left), ptr(right), w, h, ctypes.byref(prm), ptr(kl), ptr(dl),
                                         n, ptr(kr), ptr(dr), len(kr), ptr(u), ptr(z), ptr(st), ptr(br), ptr(sad),
                                         ctypes.byref(ns)), "orbhip_test_stereo_match")
    return u, z, st, br, sad, ns.value


def stereo_median_raw(ctx, status, sad, u_right, depth):
    """Test hook (orbhip_test_stereo_median): the median-cut kernel alone on one pair's entries.
    -> (status, u_right, depth, n_stereo), the three arrays as the kernel left them."""
    st = np.array(status, np.int32)
    sd = np.ascontiguousarray(sad, np.int32)
    u, z = np.array(u_right, np.float32), np.array(depth, np.float32)
    n = len(st)
    assert len(sd) == n and len(u) == n and len(z) == n
    ns = ctypes.c_int(0)
    check(lib().orbhip_test_stereo_median(ctx.handle, ptr(st), ptr(sd), ptr(u), ptr(z), n, ctypes.byref(ns)),
          "orbhip_test_stereo_median")
    return st, u, z, ns.value
