"""k_pyr_cone's level loop (pyr_cone_body in extract_kernels.hip) on single frames, against the oracle.

The loop takes a thread's pixels of a level in groups of up to four: every table word of the group
is read first, then every source byte, then the arithmetic, then the stores; a wave with fewer
pixels left runs one group of exactly that many (a lane past the end repeats the last pixel and
stores nothing). The level's geometry (pyr_off, pitch, xmax, vend, rz_noclamp, 1 / nw) is fetched
once per launch, one word per lane, and read back per level. Each case below is one frame, so the
cone is the engine; `_traced` asserts that: the trace hook (orbhip_test_trace) holds a start / end
stamp per work-group of kernel id 0 and the per-level phase words that only k_pyr_cone writes, so
the work-group count must equal the tile count ceil(wL / tile) * ceil(hL / tile) of the last level
and the words of the cone's levels must be set.

On every host frame the device equals the oracle stage by stage (helpers.compare_extract_stages:
the pyramid bytes of orbhip_test_extract_debug level by level and exactly, then candidates, kept
keypoints, the error word) and end to end (test_extract_gpu._check: monoIndex, the six keypoint
fields, the order, the descriptor bytes). A device view (the byte staging path) has no pyramid
hook; there the end-to-end result must equal the oracle's.

What reaches which part of the loop (iterations = a thread's pixels of a level at 1024 threads):
  tile 3 (320x240) / 5 (641x479)   the smallest tiles whose grids the cone route still takes (at most
                                   1024 work-groups; one less runs the per-level cascade, asserted):
                                   levels of 9 to 25 pixels, most waves issue nothing, groups of 1
  tile 10, 16                      the one-frame default and the 16-camera choice: groups 2 / 1 and 4 / 3 / 2 / 1
  tile 35 (641x479)                the largest that plans (36 does not, asserted): 10682 pixels at
                                   level 1 = two full groups and a group of 3 per thread; a staging
                                   region of ~4000 dwords (the 8-in-flight loop)
  1.5 / 5 levels, 1.9 / 4 levels   wide row spans (a level reads rows 1.5 / 1.9 apart), few levels
  ORBHIP_CONE_NT 256 / 512         4 and 2 times the iterations per thread (a fresh process each:
                                   the variable is read once)
  ORBHIP_CONE_HI=1 ORBHIP_NO_CONE=1   the same body from pyramid level 2 (s0 = 2) at 256 threads
  constant 255 / 0                 both ends of the output range through the vector form (x < vend)
                                   and the FixedPtCast tail (the columns from vend on)
The saturating middle form runs only where a level's taps fail the host's check (rz_noclamp = 0);
bilinear taps never do, so no frame reaches it: it is the parent's code, kept token for token.
"""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import synthetic_frame
from tests.helpers import (assert_frames_equal_oracle, compare_extract_stages, extract_device_frames,
                           oracle_kps_to_struct, place_frames)
from tests.test_extract_gpu import _check

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORB8 = (1000, 1.2, 8, 20, 7)
TRACE_STRIDE, TRACE_KERNELS = 16384, 8   # orbhip_kernels.h kTraceStride, kTraceKernels
CONE_HI_START = 2                        # extract_plan.h kConeHiStart


def _ext(prm):
    from orb_slam3_ros2_amd import ORBextractor
    return ORBextractor(*prm)   # a fresh context: the plan reads ORBHIP_CONE_TILE at its first lookup


def _traced(call):
    """call() with the trace hook attached: (its result, work-groups of kernel id 0 that stamped,
    the levels whose phase word work-group 0 of k_pyr_cone wrote)."""
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    L = lib()
    L.orbhip_test_trace.argtypes = [ctypes.c_int, ctypes.c_void_p]
    assert L.orbhip_test_trace(1, None) == 0
    try:
        out = call()
    finally:
        buf = np.zeros(TRACE_KERNELS * TRACE_STRIDE, np.uint64)
        assert L.orbhip_test_trace(0, buf.ctypes.data) == 0
    wgs = int((buf[1:8192:2] > 0).sum())
    levels = [int(l) for l in np.flatnonzero(buf[8192 + 1: 8192 + 16]) + 1]
    return out, wgs, levels


def _tiles(ext, w, h, tile):
    info = ext.level_info(w, h)
    return math.ceil(int(info["w"][-1]) / tile) * math.ceil(int(info["h"][-1]) / tile)


def cone_case(oracle, img, prm=ORB8, tile=10, what=""):
    """One host frame through the cone at `tile` (the caller has set ORBHIP_CONE_TILE unless 10):
    stage by stage, end to end, and the cone was the engine of both. Returns the keypoint count."""
    h, w = img.shape
    ext = _ext(prm)
    n, wgs, levels = _traced(lambda: (compare_extract_stages(ext, oracle, img, what=what),
                                      _check(ext, oracle, img, nfeatures=prm[0], scale=prm[1], nlevels=prm[2],
                                             ini=prm[3], mn=prm[4]))[1])
    assert levels == list(range(1, prm[2])), f"{what}: k_pyr_cone did not run every level: {levels}"
    assert wgs == _tiles(ext, w, h, tile), f"{what}: {wgs} work-groups for {_tiles(ext, w, h, tile)} tiles"
    return n


def _cone_levels(img, prm=ORB8):
    """The levels k_pyr_cone ran for one extraction of img ([]: another engine built the pyramid)."""
    ext = _ext(prm)
    return _traced(lambda: ext(img))[2]


@pytest.mark.parametrize("w,h,prm", [(320, 240, ORB8), (641, 479, ORB8), (641, 481, (1000, 1.5, 5, 20, 7)),
                                     (801, 601, (1000, 1.9, 4, 20, 7))],
                         ids=["320x240", "641x479", "641x481-1.5x5", "801x601-1.9x4"])
def test_cone_sizes_and_scales(oracle, w, h, prm):
    assert cone_case(oracle, synthetic_frame(50, w, h), prm, what=f"{w}x{h} {prm[1]}/{prm[2]}") > 100


@pytest.mark.parametrize("w,h,tile", [(320, 240, 3), (641, 479, 5)], ids=["320x240-3", "641x479-5"])
def test_cone_smallest_tile(oracle, monkeypatch, w, h, tile):
    img = synthetic_frame(51, w, h)
    monkeypatch.setenv("ORBHIP_CONE_TILE", str(tile - 1))
    info = _ext(ORB8)
    assert _tiles(info, w, h, tile - 1) > 1024 >= _tiles(info, w, h, tile)
    assert _cone_levels(img) == []   # more than 1024 work-groups: the per-level cascade
    monkeypatch.setenv("ORBHIP_CONE_TILE", str(tile))
    assert cone_case(oracle, img, tile=tile, what=f"{w}x{h} tile {tile}") > 100


@pytest.mark.parametrize("tile", [10, 16, 35])
def test_cone_tiles_641x479(oracle, monkeypatch, tile):
    img = synthetic_frame(52, 641, 479)
    if tile == 35:
        monkeypatch.setenv("ORBHIP_CONE_TILE", "36")
        assert _cone_levels(img) == []   # its largest cone exceeds the LDS budget: no cone tables
    monkeypatch.setenv("ORBHIP_CONE_TILE", str(tile))
    assert cone_case(oracle, img, tile=tile, what=f"641x479 tile {tile}") > 900


def test_batch_cone_single_frame(oracle, monkeypatch):
    """ORBHIP_NO_CONE=1 ORBHIP_CONE_HI=1: k_resize for levels 1 and 2, the body from level 2 on."""
    monkeypatch.setenv("ORBHIP_NO_CONE", "1")
    monkeypatch.setenv("ORBHIP_CONE_HI", "1")
    img = synthetic_frame(53, 641, 479)
    ext = _ext(ORB8)
    n, _, levels = _traced(lambda: (compare_extract_stages(ext, oracle, img, what="batch cone"),
                                    _check(ext, oracle, img))[1])
    assert n > 900 and levels == list(range(CONE_HI_START + 1, ORB8[2]))


@pytest.mark.parametrize("value", [255, 0])
def test_cone_constant_frames(oracle, value):
    img = np.full((240, 320), value, np.uint8)
    assert all((lv == value).all() for lv in oracle.pyramid(img, ORB8[1], ORB8[2]))   # which the device must equal
    assert cone_case(oracle, img, what=f"constant {value}") == 0


# (stride - w, offset): a base pointer off by 1 / 2 / 3 behind an aligned stride, strides that are
# 1 / 3 mod 4, and both at once
BYTE_VIEWS = [(64, 1), (64, 2), (64, 3), (1, 0), (3, 0), (2, 3)]


@pytest.mark.parametrize("tile", [10, 16])
def test_cone_byte_staging_views(oracle, monkeypatch, tile):
    """Device views that take the byte staging path ((pitch & 3) != 0 or (pointer & 3) != 0),
    inside a buffer of random bytes, at the single-shot-sized and the looping staging region."""
    monkeypatch.setenv("ORBHIP_CONE_TILE", str(tile))
    w, h = 320, 240
    img = synthetic_frame(54, w, h)
    mono, k6, d = oracle.extract(img, *ORB8)
    want = [(mono, oracle_kps_to_struct(k6), d)]
    ext = _ext(ORB8)
    for pad, off in BYTE_VIEWS:
        t = place_frames(img[None], w + pad, off, (w + pad) * h, "random")
        assert (t.data_ptr() % 4, t.stride(1) % 4) == (off, pad % 4) != (0, 0)
        got, wgs, levels = _traced(lambda: extract_device_frames(ext, t))
        assert_frames_equal_oracle(got, want, f"tile {tile} stride w+{pad} offset {off}")
        assert levels == list(range(1, 8)) and wgs == _tiles(ext, w, h, tile)


_NT_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import torch
from oracle import pyoracle as O
from orb_slam3_ros2_amd.synthetic import synthetic_frame
from tests.test_cone_chain_gpu import cone_case
O.lib()
print(json.dumps(dict(n=cone_case(O, synthetic_frame(55, 641, 479), tile=16, what="CONE_NT " + sys.argv[2]))))
"""


@pytest.mark.parametrize("nt", ["256", "512"])
def test_cone_threads_per_tile(nt):
    """ORBHIP_CONE_NT is read once per process: 641x479 at tile 16 in a fresh child, one run."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORBHIP_") or k == "ORBHIP_LIB"}
    env.update(ORBHIP_CONE_NT=nt, ORBHIP_CONE_TILE="16")
    p = subprocess.run([sys.executable, "-c", _NT_CHILD, REPO, nt], env=env, capture_output=True, text=True,
                       timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    assert json.loads(p.stdout.strip().splitlines()[-1])["n"] > 900
