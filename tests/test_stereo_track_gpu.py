"""Rectified-stereo tracking on the device against the numpy restatement
(tests/stereo_track_numpy.py, pinned to the oracle on the CPU by tests/test_stereo_track.py, which
also shows that every case here is an honest one): PoseOptimization with stereo edges at both
frame-group widths, and the stereo branches of both SearchByProjection forms in all four device
forms, bit-exact."""
import ctypes

import numpy as np
import pytest

import stereo_track_cases as C
from test_pose_opt import _check, _same_bits
from test_projection import PROJ_MODES

pytestmark = pytest.mark.gpu


@pytest.fixture(params=list(PROJ_MODES))
def proj_mode(request, monkeypatch):
    for k, v in PROJ_MODES[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


@pytest.fixture(params=["1", "4"])
def waves(request, monkeypatch):
    # ORBHIP_POSE_WAVES forces the frame-group width (1 = batched layout, 4 = latency layout)
    monkeypatch.setenv("ORBHIP_POSE_WAVES", request.param)
    return request.param


def _run(names, batch=False):
    from orb_slam3_ros2_amd import Optimizer
    opt = Optimizer()
    probs = [C.pose_case(nm) for nm in names]
    return opt.PoseOptimization_batch(probs) if batch else [opt.PoseOptimization(p) for p in probs]


def _check_names(names, results):
    for nm, g in zip(names, results):
        _check(g, C.pose_ref(nm))
        if nm in C.TRIALS_STABLE:
            assert g.lm_trials == C.pose_ref(nm)["lm_trials"], nm


# ---------------------------------------------------------------- 1. pose, device = restatement
def test_pose_mixed_problems(waves):
    names = [f"mixed{n}" for n in C.MIXED_N]
    _check_names(names, _run(names))


@pytest.mark.parametrize("n", C.BOUNDARY_N)
def test_pose_register_cache_boundary(waves, n):
    """n - 1, n, n + 1 around the edges a thread keeps in registers (128 at 1 wave, 1024 at 4),
    with outliers of both kinds inside and past the cached part."""
    _check_names([f"boundary{n}"], _run([f"boundary{n}"]))


def test_pose_all_stereo_and_zero_right_coordinate(waves):
    names = ["allstereo", "zero_ur"]
    rs = _run(names)
    _check_names(names, rs)
    assert rs[1].outlier[[5, 20, 41]].all()


def test_pose_all_outlier_frame_keeps_initial_pose(waves):
    p, o = C.pose_case("alloutlier"), C.pose_ref("alloutlier")
    g = _run(["alloutlier"])[0]
    _check_names(["alloutlier"], [g])
    assert g.n_inliers == 0 and g.outlier.all()
    assert np.array_equal(g.pose_q, o["pose_q"]) and np.array_equal(g.pose_t, p.pose_t)


def test_pose_points_behind_the_camera(waves):
    g = _run(["behind"])[0]
    _check_names(["behind"], [g])
    assert g.outlier[C.behind_camera_problem()[1]].all()


def test_pose_batch_mixes_the_kinds(waves):
    names = [f"batch{i}" for i in range(len(C.BATCH_N))]
    rs = _run(names, batch=True)
    _check_names(names, rs)
    assert [r.n_inliers for r in rs[:3]] == [0, 0, 0] and all(r.lm_trials == 0 for r in rs[:3])
    for nm, r in zip(names[:3], rs[:3]):       # fewer than 3 correspondences: the pose untouched
        assert np.array_equal(r.pose_t, C.pose_case(nm).pose_t)


def test_pose_one_wave_part_filled_group(monkeypatch):
    monkeypatch.setenv("ORBHIP_POSE_WAVES", "1")
    names = [f"part{i}" for i in range(C.PART_B)]
    _check_names(names, _run(names, batch=True))


# ---------------------------------------------------------------- 2. argument errors
def _expect_arg_error(ps, what):
    """ORBHIP_ERR_ARG before anything runs: no result of the batch is written."""
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd._lib import OrbHipError, PoseResultC, PoseStereoProblemC, check, lib, ptr
    opt = Optimizer()
    outl = [np.full(p.points.shape[0], 0xCC, np.uint8) for p in ps]
    cprobs = (PoseStereoProblemC * len(ps))(*[p.to_c_stereo() for p in ps])
    what(cprobs)
    cres = (PoseResultC * len(ps))()
    for r, o in zip(cres, outl):
        r.pose_q[:] = [9.0] * 4
        r.pose_t[:] = [9.0] * 3
        r.outlier, r.n_inliers, r.lm_trials = ptr(o), -77, -77
    with pytest.raises(OrbHipError) as ei:
        check(lib().orbhip_pose_optimization_stereo_batch(opt.ctx.handle, cprobs, len(ps), cres),
              "orbhip_pose_optimization_stereo_batch")
    assert ei.value.code == -1 and "ORBHIP_ERR_ARG" in str(ei.value)
    for r, o in zip(cres, outl):
        assert list(r.pose_q) == [9.0] * 4 and list(r.pose_t) == [9.0] * 3
        assert (r.n_inliers, r.lm_trials) == (-77, -77) and (o == 0xCC).all()


@pytest.mark.parametrize("octave", [-1, 8])
def test_pose_stereo_octave_out_of_range_is_an_argument_error(octave):
    good, bad = C.pose_case("mixed10").normalized(), C.pose_case("mixed63").normalized()
    assert octave == -1 or octave == len(bad.inv_sigma2)
    bad.octave = bad.octave.copy()
    bad.octave[17] = octave
    _expect_arg_error([good, bad], lambda c: None)


def test_pose_stereo_null_right_coordinates_is_an_argument_error():
    ps = [C.pose_case("mixed10").normalized(), C.pose_case("mixed63").normalized()]

    def null(c):
        c[1].u_right = None
    _expect_arg_error(ps, null)


@pytest.mark.parametrize("bf", [0.0, -1.0])
def test_pose_stereo_needs_a_positive_bf_for_a_stereo_edge(bf):
    ps = [C.pose_case("mixed10").normalized(), C.pose_case("mixed63").normalized()]
    assert (ps[1].u_right >= 0).any()

    def set_bf(c):
        c[1].bf = bf
    _expect_arg_error(ps, set_bf)
    # without a stereo edge bf is not read: the all-monocular frames of the batch carry bf = 0
    assert C.pose_case("batch3").bf == 0.0 and _run(["batch3"])[0].n_inliers == C.pose_ref("batch3")["n_inliers"]


def test_matchers_reject_a_frame_without_right_coordinates_or_baseline():
    from orb_slam3_ros2_amd import ORBmatcher
    from orb_slam3_ros2_amd._lib import OrbHipError
    s = C.scene("ragged255_3")
    mt = ORBmatcher(0.8, True)
    for field, v in [("bf", 0.0), ("b", 0.0), ("bf", -1.0), ("b", -2.0)]:
        f = C.frame(s)
        setattr(f, field, v)
        with pytest.raises(OrbHipError) as ei:
            mt.SearchByProjectionLastFrame(f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"], 15.0,
                                           last_pose=C.last_pose(s))
        assert ei.value.code == -1
        with pytest.raises(OrbHipError) as ei:
            mt.SearchLocalPoints(f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"])
        assert ei.value.code == -1
    from orb_slam3_ros2_amd._lib import LocalPointsC, ProjLastC, lib, ptr
    sc = C.frame(s).to_c_stereo()
    sc.u_right = None
    pts, d, oc, an = (np.ascontiguousarray(s[k]) for k in ("points", "mp_desc", "last_octave", "last_angle"))
    lc = ProjLastC(len(pts), ptr(pts), ptr(d), ptr(oc), ptr(an))
    lq, lt = C.last_pose(s)
    match = np.full(len(pts), -5, np.int32)
    dirn = ctypes.c_int32(7)
    rc = lib().orbhip_search_by_projection_last_stereo(mt.ctx.handle, ctypes.byref(sc), ctypes.byref(lc), ptr(lq), ptr(lt),
                                                       15.0, 1, ptr(match), ctypes.byref(dirn))
    assert rc == -1 and (match == -5).all() and dirn.value == 7
    nrm, mn, mx = (np.ascontiguousarray(s[k]) for k in ("normals", "min_dist", "max_dist"))
    mc = LocalPointsC(len(pts), ptr(pts), ptr(nrm), ptr(mn), ptr(mx), ptr(d), None)
    iv, lvl, xr = np.zeros(len(pts), np.uint8), np.zeros(len(pts), np.int32), np.zeros(len(pts), np.float32)
    rc = lib().orbhip_search_local_points_stereo(mt.ctx.handle, ctypes.byref(sc), ctypes.byref(mc), 0.5, 1.0, 0.8, 0, 0.0,
                                                 ptr(iv), ptr(lvl), ptr(xr), ptr(match))
    assert rc == -1 and (match == -5).all()


# ---------------------------------------------------------------- 3. monocular edges are untouched
@pytest.mark.parametrize("name", ["boundary129", "mixed64", "boundary1025"])
def test_monocular_problem_through_the_stereo_entry_has_the_same_bits(waves, name):
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.optimizer import PoseProblem
    p = C.pose_case(name)
    mono = PoseProblem(**{**p.__dict__, "u_right": None, "bf": 0.0})
    through = PoseProblem(**{**p.__dict__, "u_right": np.full(p.points.shape[0], -1.0, np.float32)})
    opt = Optimizer()
    a, b = opt.PoseOptimization(mono), opt.PoseOptimization(through)
    assert a.lm_trials > 0 and _same_bits(a, b)


# ---------------------------------------------------------------- 4. matchers, device = restatement
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _last(mt, s, f, th):
    return mt.SearchByProjectionLastFrame(f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"], th,
                                          last_pose=C.last_pose(s))


def _local(mt, s, f, th, far):
    return mt.SearchLocalPoints(f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"],
                                th=th, far_points=far, th_far=5.0)


def _check_local(r, o, tag):
    assert len(r) == 5 and r[0] == o[0], tag
    for a, b in zip(r[1:4], o[1:4]):
        assert np.array_equal(a, b), tag
    iv = o[2] == 1
    assert np.array_equal(_bits(r[4][iv]), _bits(o[4][iv])) and np.isnan(r[4][~iv]).all(), tag   # untouched elsewhere


@pytest.mark.parametrize("motion", C.MOTIONS)
def test_search_by_projection_last_stereo(proj_mode, motion):
    from orb_slam3_ros2_amd import ORBmatcher
    s = C.scene(motion)
    f = C.frame(s)
    mt = ORBmatcher(0.9, True)
    for th, ori in C.LAST_PARAMS:
        mt.mbCheckOrientation = ori
        n, m = _last(mt, s, f, th)
        on, om, od, _ = C.last_ref(motion, th, ori)
        assert n == on and np.array_equal(m, om) and mt.last_direction == od == s["direction"], (motion, th, proj_mode)


@pytest.mark.parametrize("motion", C.MOTIONS)
def test_search_local_points_stereo(proj_mode, motion):
    from orb_slam3_ros2_amd import ORBmatcher
    s = C.scene(motion)
    f = C.frame(s)
    for th, ratio, far in C.LOCAL_PARAMS:
        r = _local(ORBmatcher(ratio, False), s, f, th, far)
        _check_local(r, C.local_ref(motion, th, ratio, far), (motion, th, proj_mode))


def test_stereo_projection_ragged_and_empty(proj_mode):
    """Keypoint counts around the list kernel's 256-key scan step, map-point counts off its
    4-query work-groups, an empty frame and zero map points."""
    from orb_slam3_ros2_amd import ORBmatcher
    gated = 0
    for n_kp, n_mp in C.RAGGED:
        nm = f"ragged{n_kp}_{n_mp}"
        s = C.scene(nm)
        f = C.frame(s)
        mt = ORBmatcher(0.8, True)
        n, m = _last(mt, s, f, 15.0)
        on, om, od, g1 = C.last_ref(nm, 15.0, True)
        assert n == on and np.array_equal(m, om) and mt.last_direction == od, (nm, proj_mode)
        o = C.local_ref(nm, 3.0, 0.8, False)
        _check_local(_local(mt, s, f, 3.0, False), o, (nm, proj_mode))
        gated += g1 + o[5]
    assert gated > 0
    s = C.scene("nokp")
    mt = ORBmatcher(0.8, True)
    n, m = _last(mt, s, C.frame(s), 15.0)
    assert n == 0 and (m == -1).all() and mt.last_direction == 1
    r = _local(mt, s, C.frame(s), 1.0, False)
    _check_local(r, C.local_ref("nokp", 1.0, 0.8, False), "nokp")
    assert r[0] == 0 and (r[1] == -1).all()
    s = C.scene("nomp")
    n, m = _last(mt, s, C.frame(s), 15.0)
    assert n == 0 and m.size == 0 and mt.last_direction == -1
    r = _local(mt, s, C.frame(s), 1.0, False)
    assert r[0] == 0 and all(a.size == 0 for a in r[1:])


def test_all_monocular_frame_equals_the_monocular_entry(proj_mode):
    """Every keypoint without a right coordinate and a last-frame pose that is neither ahead nor
    behind: the stereo entries return what the monocular ones return on the same frame."""
    from orb_slam3_ros2_amd import ORBmatcher
    s = C.scene("neutral")
    fs = C.frame(s, u_right=np.full(len(s["kps"]), -1.0, np.float32))
    fm = C.frame(s, stereo=False)
    for th, ori in C.LAST_PARAMS:
        mt = ORBmatcher(0.9, ori)
        a, b = _last(mt, s, fs, th), mt.SearchByProjectionLastFrame(fm, s["points"], s["mp_desc"], s["last_octave"],
                                                                    s["last_angle"], th)
        assert mt.last_direction == 0 and a[0] == b[0] and np.array_equal(a[1], b[1]), (th, proj_mode)
        assert a[0] == C.last_ref("neutral", th, ori, dropped=True)[0]
    for th, ratio, far in C.LOCAL_PARAMS:
        mt = ORBmatcher(ratio, False)
        a, b = _local(mt, s, fs, th, far), _local(mt, s, fm, th, far)
        assert len(a) == 5 and len(b) == 4 and a[0] == b[0], (th, proj_mode)
        assert all(np.array_equal(x, y) for x, y in zip(a[1:4], b[1:])), (th, proj_mode)
