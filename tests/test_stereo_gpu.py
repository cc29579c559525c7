"""Rectified-stereo frames on the GPU against the restatement (tests/stereo_numpy.py): mvuRight and
mvDepth as raw 32-bit patterns, status, the search's winner and the best SAD must all be EQUAL, on
the scenes whose branches tests/test_stereo.py asserts, for both patch normalisations."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, StereoParams, lib, ptr
from orb_slam3_ros2_amd.stereo import extract_stereo_device, stereo_frame, stereo_match_raw
from orb_slam3_ros2_amd.synthetic import synthetic_frame, synthetic_stereo_pair

import stereo_numpy as S
from stereo_numpy import assert_outputs, bits

pytestmark = pytest.mark.gpu
CP = pytest.mark.parametrize("cp", [0, 1])


@pytest.fixture(scope="module")
def ext():
    from orb_slam3_ros2_amd import ORBextractor
    o = S.ORB
    return ORBextractor(o["nfeatures"], o["scale_factor"], o["nlevels"], o["ini_th"], o["min_th"])


def same_kps(a, b):
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in KP_DTYPE.names)


def raw(ext, s, cp, left_idx=None, right_idx=None):
    kl, dl, kr, dr = s["kps_l"], s["desc_l"], s["kps_r"], s["desc_r"]
    if left_idx is not None:
        kl, dl = kl[left_idx], dl[left_idx]
    if right_idx is not None:
        kr, dr = kr[right_idx], dr[right_idx]
    return stereo_match_raw(ext.ctx, s["left"], s["right"], kl, dl, kr, dr, s["bf"], s["b"], cp)


@CP
@pytest.mark.parametrize("k", range(len(S.PARITY_SCENES)))
def test_rule_parity(ext, oracle, k, cp):
    """orbhip_test_stereo_match on every parity scene: everything equal, no keypoint excluded."""
    s = S.parity_scene(oracle, k)
    e = S.restate(s, cp)
    u, z, st, br, sad, ns = raw(ext, s, cp)
    assert_outputs(u, z, st, e, f"scene {k}")
    assert np.array_equal(br, e.best_r) and np.array_equal(sad, e.sad) and ns == e.n_stereo
    if "planted" in s:   # the guard keypoints: rejected, -1 / -1, nothing formed
        g = s["planted"]["guard"]
        assert (st[g] == 9).all() and (u[g] == -1).all() and (z[g] == -1).all() and (sad[g] == -1).all()


@CP
@pytest.mark.parametrize("k", [0, 1])
def test_whole_frame(ext, oracle, k, cp):
    """orbhip_extract_stereo at 320x240 and 640x480: both keypoint and descriptor sets are the
    oracle extractor's with vLappingArea (0, 0), the stereo outputs the restatement's on them."""
    s = S.parity_scene(oracle, k)
    e = S.restate(s, cp)
    f = stereo_frame(ext, s["left"], s["right"], s["bf"], s["b"], cp)
    assert same_kps(f.mvKeys, s["kps_l"]) and np.array_equal(f.mDescriptors, s["desc_l"])
    assert same_kps(f.mvKeysRight, s["kps_r"]) and np.array_equal(f.mDescriptorsRight, s["desc_r"])
    assert_outputs(f.mvuRight, f.mvDepth, f.status, e, f"scene {k}")
    assert f.n_stereo == e.n_stereo


@pytest.mark.parametrize("route", ["resize", "flow", "bands", "cone_hi"])
def test_whole_frame_every_pyramid_route(oracle, monkeypatch, route):
    """The stereo stage reads the pyramid block where the extraction left it: the same result
    whichever engine built it (the default one-launch cone is test_whole_frame's)."""
    from orb_slam3_ros2_amd import ORBextractor
    monkeypatch.setenv("ORBHIP_NO_CONE", "1")
    if route == "flow":
        monkeypatch.setenv("ORBHIP_RZ_FLOW", "1")
    elif route == "bands":
        monkeypatch.setenv("ORBHIP_RZ_BANDS", "5")
    elif route == "cone_hi":
        monkeypatch.setenv("ORBHIP_CONE_HI", "1")
    s = S.parity_scene(oracle, 0)
    e = S.restate(s, 0)
    o = S.ORB
    x = ORBextractor(o["nfeatures"], o["scale_factor"], o["nlevels"], o["ini_th"], o["min_th"])
    f = stereo_frame(x, s["left"], s["right"], s["bf"], s["b"])
    assert same_kps(f.mvKeys, s["kps_l"]) and same_kps(f.mvKeysRight, s["kps_r"])
    assert_outputs(f.mvuRight, f.mvDepth, f.status, e, route)


def _device_call(ext, pairs, bf, b, stream, status=True):
    import torch
    dev = torch.device("cuda:0")
    P = len(pairs)
    H, W = pairs[0][0].shape
    cap = ext.max_keypoints(W, H)
    fr = torch.from_numpy(np.stack([im for pr in pairs for im in pr])).to(dev)
    kps = torch.zeros((2 * P, cap, 6), dtype=torch.float32, device=dev)
    desc = torch.zeros((2 * P, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(2 * P, dtype=torch.int32, device=dev)
    mono = torch.zeros(2 * P, dtype=torch.int32, device=dev)
    u = torch.full((P, cap), -77.0, dtype=torch.float32, device=dev)
    z = torch.full((P, cap), -77.0, dtype=torch.float32, device=dev)
    st = torch.full((P, cap), -77, dtype=torch.int32, device=dev) if status else None
    ns = torch.full((P,), -77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        extract_stereo_device(ext, fr, bf, b, kps, desc, n, mono, u, z, ns, st, stream=stream)
    stream.synchronize()
    c = lambda t: None if t is None else t.cpu().numpy()   # noqa: E731
    return c(kps), c(desc), c(n), c(u), c(z), c(st), c(ns)


@pytest.mark.parametrize("P", [1, 3])
def test_device_form(ext, P):
    """P distinct pairs on a non-default stream equal the host form pair by pair; entries at or past
    n_l keep their sentinel; a second call on the same context at another image size still agrees
    (scratch regrowth)."""
    import torch
    stream = torch.cuda.Stream()
    for (w, h) in ((320, 240), (416, 304)):
        pairs = [synthetic_stereo_pair(20 + p, w, h) for p in range(P)]
        kps, desc, n, u, z, st, ns = _device_call(ext, pairs, 40.0, 1.0, stream)
        for p, (left, right) in enumerate(pairs):
            f = stereo_frame(ext, left, right, 40.0, 1.0)
            nl, nr = int(n[2 * p]), int(n[2 * p + 1])
            assert nl == len(f.mvKeys) and nr == len(f.mvKeysRight) and nl > 100
            assert same_kps(np.frombuffer(kps[2 * p, :nl].tobytes(), KP_DTYPE), f.mvKeys)
            assert same_kps(np.frombuffer(kps[2 * p + 1, :nr].tobytes(), KP_DTYPE), f.mvKeysRight)
            assert np.array_equal(desc[2 * p, :nl], f.mDescriptors)
            assert np.array_equal(bits(u[p, :nl]), bits(f.mvuRight)) and np.array_equal(bits(z[p, :nl]), bits(f.mvDepth))
            assert np.array_equal(st[p, :nl], f.status) and ns[p] == f.n_stereo and f.n_stereo > 20
            assert (u[p, nl:] == -77).all() and (z[p, nl:] == -77).all() and (st[p, nl:] == -77).all()
    # status is optional
    pairs = [synthetic_stereo_pair(20, 320, 240)]
    _, _, n, u2, _, st2, ns2 = _device_call(ext, pairs, 40.0, 1.0, stream, status=False)
    f = stereo_frame(ext, *pairs[0], 40.0, 1.0)
    assert st2 is None and ns2[0] == f.n_stereo and np.array_equal(bits(u2[0, :n[0]]), bits(f.mvuRight))


def test_device_form_behind_a_replayed_extraction(monkeypatch):
    """ORBHIP_GRAPH=1: from the third identical call on, the extraction is one graph replay; the
    stereo kernels are launched behind it and the results stay those of the host form."""
    import torch
    from orb_slam3_ros2_amd import ORBextractor
    monkeypatch.setenv("ORBHIP_GRAPH", "1")
    o = S.ORB
    x = ORBextractor(o["nfeatures"], o["scale_factor"], o["nlevels"], o["ini_th"], o["min_th"])
    dev = torch.device("cuda:0")
    left, right = synthetic_stereo_pair(21, 320, 240)
    cap = x.max_keypoints(320, 240)
    fr = torch.from_numpy(np.stack([left, right])).to(dev)
    kps = torch.zeros((2, cap, 6), dtype=torch.float32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(2, dtype=torch.int32, device=dev)
    mono = torch.zeros(2, dtype=torch.int32, device=dev)
    u = torch.zeros((1, cap), dtype=torch.float32, device=dev)
    z = torch.zeros((1, cap), dtype=torch.float32, device=dev)
    st = torch.zeros((1, cap), dtype=torch.int32, device=dev)
    ns = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    f = stereo_frame(x, left, right, 40.0, 1.0)
    for call in range(4):
        u.fill_(-5.0)
        torch.cuda.synchronize()
        extract_stereo_device(x, fr, 40.0, 1.0, kps, desc, n, mono, u, z, ns, st, stream=stream)
        stream.synchronize()
        nl = int(n[0])
        assert nl == len(f.mvKeys) and int(ns[0]) == f.n_stereo
        assert np.array_equal(bits(u[0, :nl].cpu().numpy()), bits(f.mvuRight)), call
        assert np.array_equal(st[0, :nl].cpu().numpy(), f.status), call
    assert lib().orbhip_launch_graphs(x.ctx.handle) >= 1


def test_constant_images(ext):
    left, _ = synthetic_stereo_pair(30, 320, 240)
    flat = np.full_like(left, 90)
    f = stereo_frame(ext, left, flat, 40.0, 1.0)
    assert len(f.mvKeysRight) == 0 and len(f.mvKeys) > 100
    assert (f.status == 2).all() and f.n_stereo == 0 and (f.mvuRight == -1).all() and (f.mvDepth == -1).all()
    f = stereo_frame(ext, flat, left, 40.0, 1.0)
    assert len(f.mvKeys) == 0 and len(f.mvuRight) == 0 and f.n_stereo == 0 and len(f.mvKeysRight) > 100


def test_max_disparity_below_one(ext, oracle):
    """bf / b = 2^-20, on an identical pair so that every left keypoint finds its twin and reaches
    the disparity test: each gets status 7, except where the disparity is exactly 0 (inside
    [0, maxD): accepted with the 0.01 substitution; these all have SAD 0, so the median is 0 and
    the cut removes them)."""
    left = synthetic_frame(42, 320, 240)
    kl, dl, kr, dr, pl, pr = S.extract_pair(oracle, left, left)
    sc, inv = S.scale_tables(oracle, 320, 240)
    e = S.compute_stereo_matches(kl, dl, kr, dr, pl, pr, sc, inv, 2.0 ** -20, 1.0, 0)
    u, z, st, br, sad, ns = stereo_match_raw(ext.ctx, left, left, kl, dl, kr, dr, 2.0 ** -20, 1.0, 0)
    assert_outputs(u, z, st, e)
    assert np.array_equal(br, e.best_r) and np.array_equal(sad, e.sad) and (sad == 0).all()
    assert ns == 0 and (st == 7).sum() > 500 and set(st.tolist()) == {7, 8}
    assert (st == 8).sum() == e.events["disparity_sub"] and (u == -1).all()
    f = stereo_frame(ext, left, left, 2.0 ** -20, 1.0)
    assert np.array_equal(f.status, st) and f.n_stereo == 0


def test_single_accepted_keypoint_is_its_own_median(ext, oracle):
    """One accepted keypoint alone: it survives the cut iff SAD < 2.1 x SAD, i.e. iff SAD > 0."""
    s = S.parity_scene(oracle, 3)
    e = S.restate(s, 0)
    i = int(np.flatnonzero((e.status == 1) & (e.sad > 0))[0])
    j = s["planted"]["zero_disp"]
    for il, want in ((i, 1), (j, 8)):
        assert (e.sad[il] > 0) == (want == 1)
        u, z, st, br, sad, ns = raw(ext, s, 0, left_idx=[il], right_idx=[int(e.best_r[il])])
        assert st.tolist() == [want] and ns == (want == 1) and br.tolist() == [0] and sad[0] == e.sad[il]
        if want == 1:
            assert bits(u)[0] == bits(e.u_right)[il] and bits(z)[0] == bits(e.depth)[il]
        else:
            assert u[0] == -1 and z[0] == -1


def test_context_isolation(ext, oracle):
    """An orbhip_extract on the same context between two stereo calls changes neither result."""
    s = S.parity_scene(oracle, 0)
    a = stereo_frame(ext, s["left"], s["right"], s["bf"], s["b"])
    other = synthetic_frame(77, 640, 480)
    mono, k, d = ext(other)
    b = stereo_frame(ext, s["left"], s["right"], s["bf"], s["b"])
    mono2, k2, d2 = ext(other)
    assert same_kps(a.mvKeys, b.mvKeys) and same_kps(a.mvKeysRight, b.mvKeysRight)
    assert np.array_equal(bits(a.mvuRight), bits(b.mvuRight)) and np.array_equal(bits(a.mvDepth), bits(b.mvDepth))
    assert np.array_equal(a.status, b.status) and a.n_stereo == b.n_stereo
    assert mono == mono2 and same_kps(k, k2) and np.array_equal(d, d2)
    omono, ok6, od = oracle.extract(other)
    assert mono == omono and same_kps(k, S.kp_struct(ok6)) and np.array_equal(d, od)


def test_argument_errors(ext):
    L, h = lib(), ext.ctx.handle
    left, right = synthetic_stereo_pair(31, 320, 240)
    cap = ext.max_keypoints(320, 240)
    kl, kr = np.zeros(cap, KP_DTYPE), np.zeros(cap, KP_DTYPE)
    dl, dr = np.zeros((cap, 32), np.uint8), np.zeros((cap, 32), np.uint8)
    u, z = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
    nl, nr, ns = ctypes.c_int(5), ctypes.c_int(5), ctypes.c_int(5)

    def call(prm, left_p=ptr(left), u_p=ptr(u), cap_=cap, w=320):
        return L.orbhip_extract_stereo(h, left_p, ptr(right), w, 240, 320, prm, ptr(kl), ptr(dl), ctypes.byref(nl),
                                       ptr(kr), ptr(dr), ctypes.byref(nr), cap_, u_p, ptr(z), None, ctypes.byref(ns))

    ok = ctypes.byref(StereoParams(40.0, 1.0, 0))
    assert call(ok) == 0 and nl.value > 100 and ns.value > 20          # status may be NULL
    assert call(None) == -1
    assert call(ctypes.byref(StereoParams(0.0, 1.0, 0))) == -1 and call(ctypes.byref(StereoParams(40.0, -1.0, 0))) == -1
    assert call(ok, u_p=None) == -1
    assert call(ok, left_p=None) == -6 and call(ok, w=0) == -6 and nl.value == 0
    assert call(ok, cap_=cap - 1) == -2
    import torch
    dev = torch.device("cuda:0")
    fr = torch.zeros((2, 240, 320), dtype=torch.uint8, device=dev)
    kps = torch.zeros((2, cap, 6), dtype=torch.float32, device=dev)
    desc = torch.zeros((2, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.zeros(2, dtype=torch.int32, device=dev)
    mono = torch.zeros(2, dtype=torch.int32, device=dev)
    nst = torch.zeros(1, dtype=torch.int32, device=dev)
    uz = torch.zeros((2, cap), dtype=torch.float32, device=dev)

    def dcall(P=1, prm=ok, cap_=cap, imgs=ptr(fr)):
        return L.orbhip_extract_stereo_device(h, imgs, P, 320, 240, 320, 320 * 240, prm, ptr(kps), ptr(desc), cap_,
                                              ptr(n), ptr(mono), ptr(uz[0]), ptr(uz[1]), None, ptr(nst), None)

    assert dcall(P=0) == -1 and dcall(prm=None) == -1 and dcall(cap_=cap - 1) == -2 and dcall(imgs=None) == -6
    assert dcall() == 0
    torch.cuda.synchronize()
