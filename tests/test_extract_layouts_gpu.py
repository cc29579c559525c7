"""Extraction on padded, offset and odd-stride device frames, bit-exact against the CPU oracle.

Every kernel that reads pyramid level 0 reads it from the caller's buffer (level_img() in
extract_kernels.hip) through one of two load paths, chosen per frame at run time by
(pitch & 3) == 0 && (pointer & 3) == 0: aligned dwords, or bytes. The frames here sit inside one
larger buffer whose every other byte is poison (tests/helpers.py place_frames): a constant 0xFF, and
a seeded random stream that would create FAST corners wherever it were sampled. Each case runs with
both poisons; each run must equal the oracle's extraction of the bare frames (n, monoIndex, the six
keypoint fields, the descriptor bytes, per frame, n > 0), so the result cannot depend on the poison.

Layouts (helpers.frame_layout; r4 = w rounded up to 4):
  P   stride w, packed                                   control (the only layout of the other files)
  A   stride r4 + 64, frame stride + 256                 dword path with pitch > w, gaps poisoned
  A4  stride r4, w % 4 != 0                              a row's last dword straddles image and padding
  M1 M2 M3  stride r4 + 64, base pointer + 1 / 2 / 3     aligned pitch, misaligned pointer: byte path
  O O2 O3   smallest stride >= w that is 1 / 2 / 3 mod 4 byte path, rows at all four alignments
  X   stride r4 + 64, frame stride 2 mod 4 (B = 4)       frames 0, 2 dword path, 1, 3 byte path, one launch

Which test covers which (layout class x kernel variant) pair:

  variant \\ class          dword-padded (A, A4)   misaligned (M*)   odd stride (O*)   mixed (X)
  k_pyr_cone (default)      pyramid[cone]          pyramid[cone]     pyramid[cone]     pyramid[cone]
  k_pyr_cone, tile 16       pyramid[cone16]        pyramid[cone16]   pyramid[cone16]   pyramid[cone16]
  k_resize (NO_CONE)        pyramid[resize]        pyramid[resize]   pyramid[resize]   pyramid[resize]
  k_pyr_flow (RZ_FLOW)      pyramid[flow]          pyramid[flow]     pyramid[flow]     pyramid[flow]
  k_fast_cells<128..1024,   fast[nt-320x240]       fast[nt-320x240]  fast[nt-320x240]  fast[nt-320x240]
    kWinMax> (320x240)
  k_fast_cells<128..1024,   fast[nt-640x480]       fast[nt-640x480]  fast[nt-640x480]  fast[nt-640x480]
    50> (640x480)
  k_desc_kp (B <= 4)        every pyramid / fast case above (B = 3 or 4)
  k_desc (B = 16)           wave_desc[A, A4]       wave_desc[M1]     wave_desc[O]      wave_desc[X]
  k_stereo_match            stereo[A]              stereo[M2]        stereo[O]         stereo[X]

  pyramid   = test_pyramid_engines_on_layouts      fast   = test_fast_variants_on_layouts
  wave_desc = test_wave_per_keypoint_desc_on_layouts      stereo = test_stereo_device_on_layouts

k_pyr_cone takes its single-shot branch when a tile's level-0 cone is at most 1024 dwords (and it
runs 1024 threads), its 8-in-flight loop otherwise. At the default tile edge 10 a tile's cone is
about 60 x 60 pixels, close to that bound, with the border tiles below it; at the edge 16
(ORBHIP_CONE_TILE, the front-end's choice for one camera) about 85 x 85, above it; and the 256-
and 512-thread cones of test_static_launch_knobs always loop.

Also here: the host calls with a row stride and an odd image pointer, FrameStream.push of padded
rows, the argument checks of the layout, the level-0 patch in the frame's last rows (the bytes the
descriptor kernels' dword span may hold past the row never reach a result), and the launch knobs
that are read once per process (ORBHIP_DESC_MODE, _OCT_NT, _CONE_NT, _CONE_HI_THREADS, _XCD_RUN,
_CONE_MAX_WG), each value in a fresh child process.
"""
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, StereoParams, lib, ptr
from orb_slam3_ros2_amd.synthetic import synthetic_frame, synthetic_stereo_pair, synthetic_stream
from tests.helpers import (POISONS, assert_frames_equal_oracle, diff_report, extract_device_frames, frame_layout,
                           layout_class, oracle_kps_to_struct, place_frames)

pytestmark = pytest.mark.gpu

ORB = (1000, 1.2, 8, 20, 7)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _new_ext():
    from orb_slam3_ros2_amd import ORBextractor
    return ORBextractor(*ORB)


def _frames(w, h, B):
    """B <= 4: a synthetic frame, a uniform-noise frame, a low-contrast frame, a synthetic frame
    (test_fast_threads_per_cell_batched's mix); B = 16: fifteen synthetic frames and a noise frame."""
    key = ("frames", w, h, B)
    if key not in _cache:
        rng = np.random.default_rng(1000 * w + h)
        noise = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
        low = (128 + rng.integers(-9, 10, size=(h, w))).astype(np.uint8)
        if B <= 4:
            fr = [synthetic_frame(70, w, h), noise, low, synthetic_frame(71, w, h)][:B]
        else:
            fr = [synthetic_frame(60 + i, w, h) for i in range(B - 1)] + [noise]
        _cache[key] = np.stack(fr)
    return _cache[key]


def _oracle_of(oracle, frames, lap=(0, 1000)):
    out = []
    for img in frames:
        mono, k6, d = oracle.extract(img, *ORB, lap)
        out.append((mono, oracle_kps_to_struct(k6), d))
    return out


def _oracle_frames(oracle, w, h, B):
    key = ("oracle", w, h, B)
    if key not in _cache:
        _cache[key] = _oracle_of(oracle, _frames(w, h, B))
    return _cache[key]


def _assert_reaches(t, lid):
    """The view has the alignment its layout class is meant to put in front of the kernels."""
    B = t.shape[0]
    al = [(t[f].data_ptr() % 4 == 0) and (t.stride(1) % 4 == 0) for f in range(B)]
    cls = layout_class(lid)
    if cls == "dword-padded":
        assert all(al) and (t.stride(1) > t.shape[2])
    elif cls == "misaligned-byte":
        assert t.stride(1) % 4 == 0 and not any(al) and t.data_ptr() % 4 == int(lid[1])
    elif cls == "odd-stride-byte":
        assert t.stride(1) % 4 != 0 and not any(al)
        assert {t[0, r].data_ptr() % 4 for r in range(4)} == {0, 1, 2, 3} or t.stride(1) % 4 == 2
    elif cls == "mixed-per-frame":
        assert B == 4 and al == [True, False, True, False]


def _same_results(a, b):
    return all(x[0] == y[0] and x[1] == y[1] and x[2].tobytes() == y[2].tobytes() and np.array_equal(x[3], y[3])
               for x, y in zip(a, b))


def _run_layout(ext, frames, want, lid, what):
    """frames in layout lid under both poisons: each run equals the oracle, hence each other."""
    _, h, w = frames.shape
    S, off, fs = frame_layout(lid, w, h)
    runs = []
    for poison in POISONS:
        t = place_frames(frames, S, off, fs, poison)
        _assert_reaches(t, lid)
        got = extract_device_frames(ext, t)
        assert_frames_equal_oracle(got, want, f"{what} layout {lid} poison {poison}")
        runs.append(got)
    assert _same_results(*runs), f"{what} layout {lid}: the result depends on the poison"


# ---- A. layouts x kernel variants ----

PYR_CASES = [("P", 320, 240), ("A", 320, 240), ("A", 640, 480), ("A4", 641, 479), ("A4", 322, 241), ("A4", 323, 241),
             ("M1", 320, 240), ("M2", 640, 480), ("M3", 320, 240), ("O", 320, 240), ("O2", 640, 480),
             ("O3", 320, 240), ("X", 320, 240), ("X", 640, 480)]


@pytest.mark.parametrize("lid,w,h", PYR_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in PYR_CASES])
@pytest.mark.parametrize("engine", ["cone", "cone16", "resize", "flow"])
def test_pyramid_engines_on_layouts(oracle, monkeypatch, engine, lid, w, h):
    """Level 1 is built from the caller's buffer by k_pyr_cone (the default engine; cone16: at
    the tile edge 16 instead of 10), k_resize (ORBHIP_NO_CONE=1) or k_pyr_flow (+ ORBHIP_RZ_FLOW=1); FAST at its
    default thread count and k_desc_kp read level 0 from the same buffer."""
    if engine == "cone16":
        monkeypatch.setenv("ORBHIP_CONE_TILE", "16")
    elif engine != "cone":
        monkeypatch.setenv("ORBHIP_NO_CONE", "1")
        if engine == "flow":
            monkeypatch.setenv("ORBHIP_RZ_FLOW", "1")
    B = 4 if lid == "X" else 3
    _run_layout(_new_ext(), _frames(w, h, B), _oracle_frames(oracle, w, h, B), lid, f"{engine} {w}x{h}")


FAST_CASES = [("A", 320, 240), ("M2", 320, 240), ("O", 320, 240), ("X", 320, 240), ("A4", 323, 241),
              ("A", 640, 480), ("M3", 640, 480), ("O2", 640, 480), ("X", 640, 480), ("A4", 641, 479)]


@pytest.mark.parametrize("lid,w,h", FAST_CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}" for c in FAST_CASES])
@pytest.mark.parametrize("nt", [128, 256, 512, 1024])
def test_fast_variants_on_layouts(oracle, monkeypatch, nt, lid, w, h):
    """Every k_fast_cells<NT, WR> instantiation (threads per cell pinned per plan by ORBHIP_FAST_NT;
    640x480 cells fit the compact LDS variant, 320x240 has tall one-row cells that take the full
    one) on every layout class. A fresh extractor per value: the plan reads the variable."""
    monkeypatch.setenv("ORBHIP_FAST_NT", str(nt))
    B = 4 if lid == "X" else 3
    _run_layout(_new_ext(), _frames(w, h, B), _oracle_frames(oracle, w, h, B), lid, f"FAST_NT={nt} {w}x{h}")


@pytest.mark.parametrize("lid,w,h", [("A", 640, 480), ("A4", 641, 479), ("M1", 640, 480), ("O", 640, 480),
                                     ("X16", 640, 480)], ids=["A", "A4", "M1", "O", "X"])
def test_wave_per_keypoint_desc_on_layouts(oracle, lid, w, h):
    """B = 16: k_desc (a wave per keypoint; launch_desc takes it once B * kp_slots_total exceeds
    16384), the per-level k_resize cascade and the 256-thread FAST cells. X here alternates aligned
    and misaligned frames over all sixteen."""
    ext = _new_ext()
    B = 16
    assert B * ext.max_keypoints(w, h) > 16384   # kDescKpMaxSlots: beyond it k_desc runs
    frames, want = _frames(w, h, B), _oracle_frames(oracle, w, h, B)
    if lid != "X16":
        return _run_layout(ext, frames, want, lid, f"B=16 {w}x{h}")
    S, off, fs = frame_layout("X", w, h)
    runs = []
    for poison in POISONS:
        t = place_frames(frames, S, off, fs, poison)
        assert [t[f].data_ptr() % 4 for f in range(B)] == [0, 2] * 8 and S % 4 == 0
        got = extract_device_frames(ext, t)
        assert_frames_equal_oracle(got, want, f"B=16 layout X poison {poison}")
        runs.append(got)
    assert _same_results(*runs)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _stereo_device(ext, fr, bf, b):
    import torch
    from orb_slam3_ros2_amd.stereo import extract_stereo_device
    dev = fr.device
    P, H, W = fr.shape[0] // 2, fr.shape[1], fr.shape[2]
    cap = ext.max_keypoints(W, H)
    kps = torch.zeros((2 * P, cap, 6), dtype=torch.float32, device=dev)
    desc = torch.zeros((2 * P, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(2 * P, dtype=torch.int32, device=dev)
    mono = torch.zeros(2 * P, dtype=torch.int32, device=dev)
    u = torch.full((P, cap), -77.0, dtype=torch.float32, device=dev)
    z = torch.full((P, cap), -77.0, dtype=torch.float32, device=dev)
    st = torch.full((P, cap), -77, dtype=torch.int32, device=dev)
    ns = torch.full((P,), -77, dtype=torch.int32, device=dev)
    extract_stereo_device(ext, fr, bf, b, kps, desc, n, mono, u, z, ns, st)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in (kps, desc, n, mono, u, z, st, ns))


def _stereo_case(oracle):
    """Two 320x240 pairs; the packed device call's outputs; the restatement of the first pair."""
    if "stereo" not in _cache:
        import torch
        import stereo_numpy as SN
        assert tuple(SN.ORB.values()) == ORB
        pairs = [synthetic_stereo_pair(20 + p, 320, 240) for p in range(2)]
        frames = np.stack([im for pr in pairs for im in pr])
        packed = _stereo_device(_new_ext(), torch.from_numpy(frames).to("cuda"), 40.0, 1.0)
        kl, dl, kr, dr, pl, pr = SN.extract_pair(oracle, *pairs[0])
        sc, inv = SN.scale_tables(oracle, 320, 240)
        e = SN.compute_stereo_matches(kl, dl, kr, dr, pl, pr, sc, inv, 40.0, 1.0, 0)
        _cache["stereo"] = (frames, packed, (kl, dl, kr, dr, e))
    return _cache["stereo"]


def _check_stereo(got, packed, restated, what):
    kps, desc, n, mono, u, z, st, ns = got
    pk, pd, pn, pmono, pu, pz, pst, pns = packed
    assert np.array_equal(n, pn) and np.array_equal(mono, pmono) and np.array_equal(ns, pns), what
    assert (n > 100).all() and (ns > 20).all(), what
    for f in range(len(n)):
        c = int(n[f])
        assert np.array_equal(kps[f, :c].view(np.uint32), pk[f, :c].view(np.uint32)), (what, f)
        assert np.array_equal(desc[f, :c], pd[f, :c]), (what, f)
    for p in range(len(ns)):
        c = int(n[2 * p])
        assert np.array_equal(_bits(u[p, :c]), _bits(pu[p, :c])) and np.array_equal(_bits(z[p, :c]), _bits(pz[p, :c]))
        assert np.array_equal(st[p, :c], pst[p, :c]), (what, p)
        assert (u[p, c:] == -77).all() and (st[p, c:] == -77).all(), (what, p)
    kl, dl, kr, dr, e = restated
    nl, nr = int(n[0]), int(n[1])
    assert nl == len(kl) and nr == len(kr), what
    assert np.array_equal(np.frombuffer(kps[0, :nl].tobytes(), KP_DTYPE), kl) and np.array_equal(desc[0, :nl], dl)
    assert np.array_equal(np.frombuffer(kps[1, :nr].tobytes(), KP_DTYPE), kr) and np.array_equal(desc[1, :nr], dr)
    assert np.array_equal(st[0, :nl], e.status), what
    assert np.array_equal(_bits(u[0, :nl]), _bits(e.u_right)) and np.array_equal(_bits(z[0, :nl]), _bits(e.depth))
    assert int(ns[0]) == e.n_stereo, what


@pytest.mark.parametrize("lid", ["P", "A", "M2", "O", "X"])
def test_stereo_device_on_layouts(oracle, lid):
    """orbhip_extract_stereo_device on two pairs: k_stereo_match reads its level-0 windows from
    the caller's buffer (both extractions with vLappingArea {0, 0} in front of it). Every output
    bit equals the packed call's, and the first pair's the restatement's (tests/stereo_numpy.py)."""
    frames, packed, restated = _stereo_case(oracle)
    _check_stereo(packed, packed, restated, "packed")   # the packed call itself against the restatement
    S, off, fs = frame_layout(lid, 320, 240)
    ext = _new_ext()
    for poison in POISONS:
        t = place_frames(frames, S, off, fs, poison)
        _assert_reaches(t, lid)
        _check_stereo(_stereo_device(ext, t, 40.0, 1.0), packed, restated, f"stereo layout {lid} poison {poison}")


# ---- host calls, the front-end stream, the argument checks ----

def _host_image(img, stride, poison):
    """img inside a poisoned host buffer, its first pixel at an odd address: (buffer, address)."""
    h, w = img.shape
    size = 8 + h * stride + 64
    buf = (np.random.default_rng(0xB0B).integers(0, 256, size, dtype=np.uint8) if poison == "random"
           else np.full(size, int(poison), np.uint8))
    off = 1 if ptr(buf) % 2 == 0 else 2
    np.lib.stride_tricks.as_strided(buf[off:], (h, w), (stride, 1))[...] = img
    assert (ptr(buf) + off) % 2 == 1
    return buf, ptr(buf) + off


@pytest.mark.parametrize("w,h", [(640, 480), (641, 479)])
def test_host_extract_row_stride_and_odd_pointer(oracle, w, h):
    """orbhip_extract with stride = w + 37 and an odd image address inside a poisoned buffer."""
    ext = _new_ext()
    img = synthetic_frame(75, w, h)
    omono, k6, od = oracle.extract(img, *ORB)
    ok = oracle_kps_to_struct(k6)
    cap = ext.max_keypoints(w, h)
    for poison in POISONS:
        buf, addr = _host_image(img, w + 37, poison)
        kps, desc = np.zeros(cap, KP_DTYPE), np.zeros((cap, 32), np.uint8)
        n, mono = ctypes.c_int(0), ctypes.c_int(0)
        rc = lib().orbhip_extract(ext.ctx.handle, addr, w, h, w + 37, 0, 1000, ptr(kps), ptr(desc), cap,
                                  ctypes.byref(n), ctypes.byref(mono))
        assert rc == 0 and n.value == len(ok) > 0 and mono.value == omono, (rc, n.value, poison)
        assert np.array_equal(kps[:n.value], ok) and np.array_equal(desc[:n.value], od), \
            diff_report(kps[:n.value], desc[:n.value], ok, od)
        del buf


def test_host_stereo_row_stride_and_odd_pointer():
    """orbhip_extract_stereo likewise, against its own packed call."""
    from orb_slam3_ros2_amd.stereo import stereo_frame
    ext = _new_ext()
    w, h, stride = 320, 240, 320 + 37
    left, right = synthetic_stereo_pair(22, w, h)
    f = stereo_frame(ext, left, right, 40.0, 1.0)
    assert len(f.mvKeys) > 100 and f.n_stereo > 20
    cap = ext.max_keypoints(w, h)
    prm = StereoParams(40.0, 1.0, 0)
    for poison in POISONS:
        bl, al = _host_image(left, stride, poison)
        br, ar = _host_image(right, stride, poison)
        kl, kr = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
        dl, dr = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
        u, z, st = np.zeros(cap, np.float32), np.zeros(cap, np.float32), np.zeros(cap, np.int32)
        nl, nr, ns = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        rc = lib().orbhip_extract_stereo(ext.ctx.handle, al, ar, w, h, stride, ctypes.byref(prm), ptr(kl), ptr(dl),
                                         ctypes.byref(nl), ptr(kr), ptr(dr), ctypes.byref(nr), cap, ptr(u), ptr(z),
                                         ptr(st), ctypes.byref(ns))
        a, c = nl.value, nr.value
        assert rc == 0 and a == len(f.mvKeys) and c == len(f.mvKeysRight) and ns.value == f.n_stereo, poison
        assert np.array_equal(kl[:a], f.mvKeys) and np.array_equal(dl[:a], f.mDescriptors)
        assert np.array_equal(kr[:c], f.mvKeysRight) and np.array_equal(dr[:c], f.mDescriptorsRight)
        assert np.array_equal(_bits(u[:a]), _bits(f.mvuRight)) and np.array_equal(_bits(z[:a]), _bits(f.mvDepth))
        assert np.array_equal(st[:a], f.status)
        del bl, br


def test_frontend_push_padded_rows(oracle):
    """FrameStream.push of [H, W] views with a padded row stride (layouts A and M1), 6 frames of a
    640x480 stream with 2 frames in flight: every slot view equals the oracle's extraction, and
    the match counts equal those of the same stream pushed packed."""
    import torch
    from orb_slam3_ros2_amd import FrameStream
    K, w, h = 6, 640, 480
    host = synthetic_stream(K, w, h, 91)
    want = _oracle_of(oracle, host)

    def run(frames_t):
        fs = FrameStream(w, h, 2)
        nm = []
        for k in range(K):
            assert frames_t[k].stride(0) == frames_t.stride(1)
            s = fs.push(frames_t[k])
            fs.wait(s)
            v = fs.view(s)
            c = int(v["n"][0])
            gk = np.frombuffer(v["kps"][:c].cpu().numpy().tobytes(), KP_DTYPE)
            gd = v["desc"][:c].cpu().numpy()
            omono, ok, od = want[k]
            assert v["frame"] == k and c == len(ok) > 0 and int(v["mono"][0]) == omono, k
            assert np.array_equal(gk, ok) and np.array_equal(gd, od), (k, diff_report(gk, gd, ok, od))
            nm.append(int(v["nmatch"][0]))
        fs.close()
        return nm

    packed = run(torch.from_numpy(host).to("cuda"))
    assert packed[0] == -1 and min(packed[1:]) > 100
    for lid in ("A", "M1"):
        S, off, fs_ = frame_layout(lid, w, h)
        for poison in POISONS:
            t = place_frames(host, S, off, fs_, poison)
            _assert_reaches(t, lid)
            assert run(t) == packed, (lid, poison)


def test_layout_argument_checks():
    """stride < w, and frames that overlap (B > 1, frame_stride < stride * h), are ORBHIP_ERR_ARG
    for the batch and the stereo device call, and nothing is launched: no output changes."""
    import torch
    ext = _new_ext()
    L, hd = lib(), ext.ctx.handle
    w, h = 320, 240
    cap = ext.max_keypoints(w, h)
    dev = torch.device("cuda:0")
    fr = torch.from_numpy(np.stack(synthetic_stereo_pair(31, w, h))).to(dev)
    outs = dict(kps=torch.full((2, cap, 6), -5.0, dtype=torch.float32, device=dev),
                desc=torch.full((2, cap, 32), 0xA5, dtype=torch.uint8, device=dev),
                n=torch.full((2,), -5, dtype=torch.int32, device=dev),
                mono=torch.full((2,), -5, dtype=torch.int32, device=dev),
                u=torch.full((cap,), -5.0, dtype=torch.float32, device=dev),
                z=torch.full((cap,), -5.0, dtype=torch.float32, device=dev),
                ns=torch.full((1,), -5, dtype=torch.int32, device=dev))
    before = {k: v.clone() for k, v in outs.items()}
    prm = ctypes.byref(StereoParams(40.0, 1.0, 0))

    def batch(B, stride, fstride):
        return L.orbhip_extract_batch_device(hd, ptr(fr), B, w, h, stride, fstride, 0, 1000, ptr(outs["kps"]),
                                             ptr(outs["desc"]), cap, ptr(outs["n"]), ptr(outs["mono"]), None)

    def stereo(stride, fstride):
        return L.orbhip_extract_stereo_device(hd, ptr(fr), 1, w, h, stride, fstride, prm, ptr(outs["kps"]),
                                              ptr(outs["desc"]), cap, ptr(outs["n"]), ptr(outs["mono"]),
                                              ptr(outs["u"]), ptr(outs["z"]), None, ptr(outs["ns"]), None)

    assert batch(1, w - 1, w * h) == -1 and batch(2, w - 1, w * h) == -1
    assert batch(2, w, w * h - 1) == -1 and batch(2, w + 4, w * h) == -1
    assert stereo(w - 1, w * h) == -1 and stereo(w, w * h - 1) == -1 and stereo(w + 4, w * h) == -1
    torch.cuda.synchronize()
    assert all(torch.equal(outs[k], before[k]) for k in outs)
    # the same arguments with a legal layout run (B = 1 takes any frame stride)
    assert batch(1, w, 0) == 0 and stereo(w, w * h) == 0
    torch.cuda.synchronize()
    assert int(outs["n"][0]) > 100 and int(outs["ns"][0]) > 20


# ---- B. the level-0 patch in the frame's last rows ----

LAST_ROWS = [(1150, 320, 240, 22, "P"), (1202, 320, 240, 23, "P"), (1313, 320, 240, 23, "P"),
             (1323, 320, 240, 23, "P"), (1319, 323, 241, 22, "A4")]


@pytest.mark.parametrize("B", [2, 16], ids=["k_desc_kp", "k_desc"])
@pytest.mark.parametrize("seed,w,h,dx,lid", LAST_ROWS, ids=[f"{c[0]}-{c[4]}" for c in LAST_ROWS])
def test_level0_patch_at_last_rows(oracle, seed, w, h, dx, lid, B):
    """A noise frame whose extraction keeps a level-0 keypoint at (w - dx, h - 22), dx = 22 or 23:
    its 43x43 patch ends in the frame's last row, and the 12 aligned dwords per patch row that the
    descriptor kernels' dword path would load end 4 bytes (w % 4 == 0) or 5 (w % 4 == 3, dx = 22)
    past that row. The kernels take the byte path for such a keypoint (desc_dword_span_ok), so
    nothing past the frame is read; a test cannot see a read, so this pins that whatever follows
    the frame never reaches a result. The frame is the last of a batch whose buffer continues with
    poison (packed, or stride w + 1 at 323x241); k_desc_kp at B = 2, k_desc at B = 16."""
    img = np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)
    mono, k6, d = oracle.extract(img, *ORB)
    at = (k6[:, 5] == 0) & (k6[:, 0] == w - dx) & (k6[:, 1] == h - 22)
    assert at.sum() == 1, "the frame no longer has its keypoint at the last patch row"
    frames = np.stack([synthetic_frame(70 + f, w, h) for f in range(B - 1)] + [img])
    key = ("last", w, h, B)
    if key not in _cache:
        _cache[key] = _oracle_of(oracle, frames[:-1])
    want = _cache[key] + [(mono, oracle_kps_to_struct(k6), d)]
    ext = _new_ext()
    assert (B * ext.max_keypoints(w, h) > 16384) == (B == 16)   # launch_desc's choice of kernel
    _run_layout(ext, frames, want, lid, f"seed {seed} B={B}")


# ---- C. launch knobs read once per process: each value in a fresh child ----

_KNOB_CHILD = r"""
import json, os, sys, time
t0 = time.time()
import numpy as np
sys.path.insert(0, sys.argv[1])
import torch
from oracle import pyoracle as O
from orb_slam3_ros2_amd import ORBextractor
from orb_slam3_ros2_amd.synthetic import synthetic_frame
from tests.helpers import (POISONS, diff_report, extract_device_frames, frame_layout, oracle_kps_to_struct,
                           place_frames)
ORB = (1000, 1.2, 8, 20, 7)
cases = []
def oracle_of(frames):
    out = []
    for img in frames:
        mono, k6, d = O.extract(img, *ORB)
        out.append((mono, oracle_kps_to_struct(k6), d))
    return out
def first_diff(got, want):
    for f, ((n, mono, gk, gd), (omono, ok, od)) in enumerate(zip(got, want)):
        same = (n == len(ok) and n > 0 and mono == omono and gk.tobytes() == ok.tobytes() and np.array_equal(gd, od))
        if not same:
            return "frame %d: n gpu=%d monoIndex gpu=%d oracle=%d\n%s" % (f, n, mono, omono, diff_report(gk, gd, ok, od))
    return None
def record(name, got, want):
    d = first_diff(got, want)
    cases.append(dict(name=name, ok=d is None, diff=d))
def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)
ext = ORBextractor(*ORB)
for (w, h) in ((640, 480), (641, 479)):
    img = synthetic_frame(76, w, h)
    mono, k, d = ext(img)
    record("host %dx%d" % (w, h), [(len(k), mono, k, d)], oracle_of([img]))
fr = np.stack([synthetic_frame(77, 320, 240), noise(320, 240, 1), synthetic_frame(78, 320, 240)])
want = oracle_of(fr)
for poison in POISONS:
    record("B=3 320x240 layout A poison %s" % poison,
           extract_device_frames(ext, place_frames(fr, *frame_layout("A", 320, 240), poison)), want)
fr = np.stack([synthetic_frame(60 + i, 640, 480) for i in range(15)] + [noise(640, 480, 2)])
record("B=16 640x480", extract_device_frames(ext, torch.from_numpy(fr).to("cuda")), oracle_of(fr))
os.environ["ORBHIP_NO_CONE"] = "1"
os.environ["ORBHIP_CONE_HI"] = "1"
fr = np.stack([synthetic_frame(79, 1280, 720), noise(1280, 720, 3), synthetic_frame(80, 1280, 720)])
record("B=3 1280x720 NO_CONE CONE_HI", extract_device_frames(ORBextractor(*ORB), torch.from_numpy(fr).to("cuda")),
       oracle_of(fr))
print(json.dumps(dict(ok=all(c["ok"] for c in cases), cases=cases, seconds=round(time.time() - t0, 2))))
"""

KNOB_ENVS = {
    "child1": dict(ORBHIP_DESC_MODE="0", ORBHIP_OCT_NT="256", ORBHIP_CONE_NT="256", ORBHIP_CONE_HI_THREADS="512",
                   ORBHIP_XCD_RUN="0"),
    "child2": dict(ORBHIP_DESC_MODE="1", ORBHIP_OCT_NT="1024", ORBHIP_CONE_NT="512", ORBHIP_CONE_HI_THREADS="1024",
                   ORBHIP_XCD_RUN="-1"),
    # a run length that divides no grid (xcd_runs' identity tail); no cone by the size rule
    "child3": dict(ORBHIP_XCD_RUN="3", ORBHIP_CONE_MAX_WG="0"),
}


@pytest.mark.parametrize("child", list(KNOB_ENVS))
def test_static_launch_knobs(child):
    """ORBHIP_DESC_MODE (0: a wave per keypoint at every batch size, 1: a work-group per keypoint
    even at B = 16), ORBHIP_OCT_NT, ORBHIP_CONE_NT, ORBHIP_CONE_HI_THREADS, ORBHIP_XCD_RUN and
    ORBHIP_CONE_MAX_WG are read once per process, so each set of values runs in a fresh child:
    host extractions at 640x480 and 641x479, a B = 3 batch at 320x240 in layout A under both
    poisons, a B = 16 batch at 640x480, and a B = 3 batch at 1280x720 through the batch cone
    (ORBHIP_NO_CONE=1 ORBHIP_CONE_HI=1), all against the oracle inside the child. One run each, no
    retry: a non-zero exit or a timeout fails."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("ORBHIP_") or k == "ORBHIP_LIB"}
    env.update(KNOB_ENVS[child])
    t0 = time.time()
    p = subprocess.run([sys.executable, "-c", _KNOB_CHILD, REPO], env=env, capture_output=True, text=True, timeout=240)
    print(f"{child}: wall {time.time() - t0:.1f} s")
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    print(f"{child}: {res['seconds']} s inside the child, {len(res['cases'])} cases")
    bad = [c for c in res["cases"] if not c["ok"]]
    assert res["ok"] and not bad and len(res["cases"]) == 6,"\n".join(f"{c['name']}: {c['diff']}" for c in bad)
