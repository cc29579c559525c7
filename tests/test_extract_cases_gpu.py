"""The extraction catalogue (tests/extract_cases.py) on the GPU: on every frame the device must EQUAL
the oracle stage by stage (helpers.compare_extract_stages: pyramid bytes, FAST candidates per level,
kept keypoints per level, the error word) and end to end (test_extract_gpu._check: monoIndex, all
six keypoint fields, the order, the descriptor bytes). tests/test_extract_cases.py asserts on the
CPU that each case reaches the edge it is named for."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import synthetic_frame
from tests.helpers import (assert_frames_equal_oracle, compare_extract_stages, extract_device_frames,
                           oracle_kps_to_struct)
from tests.test_extract_gpu import _check

import extract_cases as C

pytestmark = pytest.mark.gpu


def _ext(prm):
    from orb_slam3_ros2_amd import ORBextractor
    return ORBextractor(*prm)   # a fresh context: the plan reads the switches of the moment


def _end_to_end(ext, oracle, img, prm):
    nf, sf, L, ini, mn = prm
    return _check(ext, oracle, img, nfeatures=nf, scale=sf, nlevels=L, ini=ini, mn=mn)


def _both(ext, oracle, img, prm, what):
    """Stage by stage, then end to end; the number of keypoints."""
    compare_extract_stages(ext, oracle, img, what=what)
    return _end_to_end(ext, oracle, img, prm)


def _envelope(name):
    w, h, nf, sf, L = C.envelope_shape(name)
    frames = [C.frame(kind, seed, w, h) for kind, seed in C.ENVELOPE[name]["frames"]]
    return (nf, sf, L, 20, 7), frames


@pytest.mark.parametrize("name,kind,seed", C.envelope_ids())
def test_envelope_case_stage_by_stage(oracle, name, kind, seed):
    w, h, nf, sf, L = C.envelope_shape(name)
    prm = (nf, sf, L, 20, 7)
    img = C.frame(kind, seed, w, h)
    assert _both(_ext(prm), oracle, img, prm, f"{name} {kind}") > 0


@pytest.mark.parametrize("engine", ["resize", "flow"])
@pytest.mark.parametrize("name", C.PYRAMID_ENGINE_CASES)
def test_envelope_case_batch_pyramid_engines(oracle, monkeypatch, name, engine):
    """The multi-level cases under the batch engines forced on single frames: k_resize per level
    (ORBHIP_NO_CONE=1) and the one-launch dataflow pyramid (+ ORBHIP_RZ_FLOW=1, k_pyr_flow). The
    stage hook runs the same engine, so the pyramid bytes are compared as well."""
    monkeypatch.setenv("ORBHIP_NO_CONE", "1")
    if engine == "flow":
        monkeypatch.setenv("ORBHIP_RZ_FLOW", "1")
    prm, frames = _envelope(name)
    assert prm[2] > 1
    ext = _ext(prm)
    for img in frames:
        assert _both(ext, oracle, img, prm, f"{name} {engine}") > 0


@pytest.mark.parametrize("cap", ["0", None])
@pytest.mark.parametrize("nt", ["128", "1024"])
@pytest.mark.parametrize("name", C.BIG_CELL_CASES)
def test_big_cells_every_fast_variant(oracle, monkeypatch, name, nt, cap):
    """Cells of 64 to 69 px (windows up to 75: the full LDS variant of k_fast_cells) with the threads
    per cell pinned at both ends, with the survivor list and with the dense pass forced (cap 0)."""
    monkeypatch.setenv("ORBHIP_FAST_NT", nt)
    if cap is not None:
        monkeypatch.setenv("ORBHIP_FAST_CLIST_CAP", cap)
    prm, frames = _envelope(name)
    ext = _ext(prm)
    for img in frames:
        assert _both(ext, oracle, img, prm, f"{name} nt {nt} cap {cap}") > 0


@pytest.mark.parametrize("name", C.BIG_CELL_CASES)
def test_big_cells_sweep_octree(oracle, monkeypatch, name):
    monkeypatch.setenv("ORBHIP_OCTREE_SWEEP", "1")
    prm, frames = _envelope(name)
    ext = _ext(prm)
    for img in frames:
        assert _both(ext, oracle, img, prm, f"{name} sweep") > 0


@pytest.mark.parametrize("name", ["67x67", "136x101"])
def test_small_frames_batched(oracle, name):
    """extract_batch_device with B = 3 at the smallest frame and at two roots in one cell row: each
    frame equals the oracle."""
    import torch
    w, h, nf, sf, L = C.envelope_shape(name)
    frames = np.stack([synthetic_frame(5, w, h), C.noise(5, w, h), C.noise(6, w, h)])
    ext = _ext((nf, sf, L, 20, 7))
    got = extract_device_frames(ext, torch.from_numpy(frames).to("cuda"))
    want = []
    for f in frames:
        mono, k6, d = oracle.extract(f, nf, sf, L, 20, 7, (0, 1000))
        want.append((mono, oracle_kps_to_struct(k6), d))
    assert_frames_equal_oracle(got, want, name)


@pytest.mark.parametrize("name", list(C.REJECTED))
def test_rejected_shape_is_unsupported_and_harmless(oracle, name):
    """ORBHIP_ERR_UNSUPPORTED from max_keypoints, from ORBextractor.__call__ and from orbhip_extract
    itself, with no output written; the context and the device stay usable: an extraction that plans
    (on the same context where its parameters plan at 320x240, on a default one otherwise) equals
    the oracle afterwards."""
    from orb_slam3_ros2_amd._lib import KP_DTYPE, OrbHipError, lib, ptr
    w, h, nf, sf, L = C.rejected_shape(name)
    prm = (nf, sf, L, 20, 7)
    ext = _ext(prm)
    img = C.noise(3, w, h)
    with pytest.raises(OrbHipError) as e:
        ext.max_keypoints(w, h)
    assert e.value.code == C.UNSUPPORTED
    with pytest.raises(OrbHipError) as e:
        ext(img)
    assert e.value.code == C.UNSUPPORTED
    kps, desc = np.zeros(64, KP_DTYPE), np.zeros((64, 32), np.uint8)
    n, mono = ctypes.c_int(-7), ctypes.c_int(-7)
    rc = lib().orbhip_extract(ext.ctx.handle, ptr(img), w, h, w, 0, 1000, ptr(kps), ptr(desc), 64, ctypes.byref(n),
                              ctypes.byref(mono))
    assert rc == C.UNSUPPORTED and n.value == 0 and mono.value == -1
    assert not kps.view(np.uint8).any() and not desc.any()
    ok = synthetic_frame(13, 320, 240)
    if C.plan(320, 240, nf, sf, L) is not None:
        assert _end_to_end(ext, oracle, ok, prm) > 0
    assert _end_to_end(_ext(C.ORB8), oracle, ok, C.ORB8) > 0


@pytest.mark.parametrize("name", list(C.CRAFTED))
def test_crafted_frame_stage_by_stage(oracle, name):
    make, prm, _ = C.CRAFTED[name]
    img = make()
    n = _both(_ext(prm), oracle, img, prm, name)
    assert (n == 0) == (name == "contrast-7")   # the one frame whose emptiness is the point


@pytest.mark.parametrize("name", C.SWEEP_CASES)
def test_crafted_frame_sweep_octree(oracle, monkeypatch, name):
    """Every node choice a tie (90 candidates of one response for a quota of 22) on the key-sweep
    engine as well."""
    monkeypatch.setenv("ORBHIP_OCTREE_SWEEP", "1")
    make, prm, _ = C.CRAFTED[name]
    assert _both(_ext(prm), oracle, make(), prm, f"{name} sweep") > 0


@pytest.mark.parametrize("w,h,seed", [(640, 480, 0), (1280, 720, 10), (641, 479, 12)])
def test_everyday_frame_stage_by_stage(oracle, w, h, seed):
    """The stage comparison at the sizes and parameters every other extraction test uses."""
    assert _both(_ext(C.ORB8), oracle, synthetic_frame(seed, w, h), C.ORB8, f"seed {seed}") > 900
