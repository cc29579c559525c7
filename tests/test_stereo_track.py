"""Rectified-stereo tracking on the CPU: the numpy restatement (tests/stereo_track_numpy.py) of
PoseOptimization with stereo edges and of the stereo branches of both SearchByProjection forms.

1. With u_right all -1 the restatement is the oracle: equal flags, inlier and trial counts and the
   pose within the existing 1e-4 bound for the optimiser, exact matches for the two searches.
2. Definitional KATs of the stereo rule (the restatement alone; upstream has no fixtures).
3. Every problem and scene tests/test_stereo_track_gpu.py runs on the device is an honest case:
   the restatement's flags of each pose problem do not depend on the edge order (the device sums
   the edges in another order), and in each of the three stereo scenes the gate rejects candidates
   that passed every earlier test, changes at least 5 % of the queries' matches, and the direction
   is decided at least 1 mm away from the baseline. (The ragged, empty and all-monocular frames of
   the GPU file are size and routing cases; the three conditions are asked of the three scenes.)
"""
import numpy as np
import pytest

import stereo_track_cases as C
import stereo_track_numpy as S
from orb_slam3_ros2_amd.matcher import ProjFrame
from orb_slam3_ros2_amd.optimizer import PoseProblem
from orb_slam3_ros2_amd.synthetic import (_mat_to_quat, synthetic_pose_problem, synthetic_projection_scene,
                                          synthetic_stereo_pose_problem, synthetic_stereo_projection_scene)
from test_pose_opt import _check, _qdist


class _R:
    """A restatement result with the attributes _check reads from a device result."""

    def __init__(self, d):
        self.__dict__.update(d)


def _with_ur(p, ur, bf=0.0):
    return PoseProblem(**{**p.__dict__, "u_right": np.asarray(ur, np.float32), "bf": bf})


# ---------------------------------------------------------------- 1. restatement = oracle
@pytest.mark.parametrize("n", [3, 9, 10, 64, 150, 600])
def test_pose_restatement_is_the_oracle_on_monocular_problems(oracle, n):
    p, _ = synthetic_pose_problem(n=n, outlier_frac=0.15, seed=200 + n)
    o = oracle.pose_optimization(p)
    r = S.pose_optimization(_with_ur(p, np.full(n, -1.0)))
    _check(_R(r), o)
    assert r["lm_trials"] == o["lm_trials"]
    assert S.pose_optimization(p)["lm_trials"] == o["lm_trials"]      # u_right None: the same problem


@pytest.mark.parametrize("seed", list(range(10, 15)) + list(range(20, 25)))
def test_matcher_restatements_are_the_oracle_on_monocular_frames(oracle, seed):
    s = synthetic_projection_scene(seed=seed)
    f = ProjFrame(s["kps"], s["desc"], s["pose_q"], s["pose_t"], s["fx"], s["fy"], s["cx"], s["cy"],
                  claimed=s["claimed"], u_right=np.full(len(s["kps"]), -1.0, np.float32), bf=49.0, b=0.1)
    same_pose = (s["pose_q"], s["pose_t"])                            # tlc = 0: neither forward nor backward
    for th, ori in [(15.0, True), (7.0, False)]:
        n, m, d = S.search_by_projection_last(f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"], th, ori,
                                              last_pose=same_pose)
        on, om = oracle.search_by_projection_last(f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"],
                                                  th, ori)
        assert d == 0 and n == on and np.array_equal(m, om), (seed, th)
    for th, ratio, far in [(1.0, 0.8, False), (3.0, 0.8, False), (5.0, 0.6, True)]:
        r = S.search_local_points(f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"],
                                  th=th, nnratio=ratio, far_points=far, th_far=5.0)
        o = oracle.search_local_points(f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"],
                                       s["skip"], th=th, nnratio=ratio, far_points=far, th_far=5.0)
        assert r[0] == o[0] and all(np.array_equal(a, b) for a, b in zip(r[1:4], o[1:])), (seed, th)
        assert np.isfinite(r[4][r[2] == 1]).all() and np.isnan(r[4][r[2] == 0]).all()


# ---------------------------------------------------------------- 2. KATs of the stereo rule
def _exact_stereo_problem(n=300, seed=11):
    p, gt = synthetic_stereo_pose_problem(n=n, outlier_frac=0.0, seed=seed, stereo_frac=1.0, ur_outlier_frac=0.0)
    Xc = p.points.astype(np.float64) @ gt["R"].T + gt["t"]
    fx, fy, cx, cy = (float(np.float32(v)) for v in (p.fx, p.fy, p.cx, p.cy))
    u = fx * Xc[:, 0] / Xc[:, 2] + cx
    p.uv = np.stack([u, fy * Xc[:, 1] / Xc[:, 2] + cy], 1).astype(np.float32)
    ur = (u - p.bf / Xc[:, 2])
    p.u_right = np.where(ur >= 0, ur, -1.0).astype(np.float32)
    return p, gt, Xc


def test_exact_stereo_observations_converge():
    p, gt, _ = _exact_stereo_problem()
    assert (p.u_right >= 0).mean() > 0.9
    r = S.pose_optimization(p)
    assert r["n_inliers"] == 300 and not r["outlier"].any()
    assert _qdist(r["pose_q"], _mat_to_quat(gt["R"])) < 1e-9
    assert np.abs(r["pose_t"] - gt["t"]).max() < 1e-4


def test_right_coordinate_error_is_a_stereo_outlier_only():
    p, _, _ = _exact_stereo_problem(n=100, seed=12)
    e = int(np.nonzero(p.u_right >= 0)[0][7])
    p.u_right[e] += np.float32(3.0 * 1.2 ** int(p.octave[e]))         # chi2 = 9 > 7.815 as a stereo edge
    r = S.pose_optimization(p)
    assert r["outlier"][e] == 1 and r["outlier"].sum() == 1
    mono = S.pose_optimization(_with_ur(p, np.where(np.arange(100) == e, -1.0, p.u_right), p.bf))
    assert not mono["outlier"].any()                                  # the same edge, monocular: u, v are exact


def test_zero_right_coordinate_is_a_stereo_edge_and_ungated():
    p, _, _ = _exact_stereo_problem(n=60, seed=13)
    p.u_right[9] = 0.0                                                # far from u - bf / z: an outlier iff stereo
    r = S.pose_optimization(p)
    assert r["outlier"][9] == 1 and r["outlier"].sum() == 1
    assert not S.pose_optimization(_with_ur(p, np.where(np.arange(60) == 9, -1.0, p.u_right), p.bf))["outlier"].any()
    # the matchers gate u_right > 0 only: 0.0 behaves as -1
    s = C.scene("neutral")
    m = int(np.nonzero(C.last_ref("neutral", 7.0, False)[1] != C.last_ref("neutral", 7.0, False, True)[1])[0][0])
    k = int(C.last_ref("neutral", 7.0, False, True)[1][m])           # gated away from query m
    assert s["u_right"][k] > 0
    for v in (0.0, -1.0):
        ur = s["u_right"].copy()
        ur[k] = v
        r = S.search_by_projection_last(C.frame(s, u_right=ur), s["points"][:m + 1], s["mp_desc"][:m + 1],
                                        s["last_octave"][:m + 1], s["last_angle"][:m + 1], 7.0, False,
                                        last_pose=C.last_pose(s))
        assert r[1][m] == k, v


def test_two_stereo_correspondences_leave_the_pose_untouched():
    p, _, _ = _exact_stereo_problem(n=2, seed=14)
    p.u_right = np.maximum(p.u_right, np.float32(1.0))
    r = S.pose_optimization(p)
    assert r["n_inliers"] == 0 and r["lm_trials"] == 0 and not r["outlier"].any()
    assert np.array_equal(r["pose_t"], p.pose_t)


def test_nine_edges_run_one_round_ten_run_four():
    r9 = S.pose_optimization(synthetic_stereo_pose_problem(n=9, outlier_frac=0.0, seed=15)[0])
    r10 = S.pose_optimization(synthetic_stereo_pose_problem(n=10, outlier_frac=0.0, seed=15)[0])
    assert 0 < r9["lm_trials"] <= 100 and r10["lm_trials"] > r9["lm_trials"]


def _one_query_frame(octaves, u_right, xs, bits):
    """Keypoints on one image row near the centre with descriptors `bits` bits from the query's."""
    from orb_slam3_ros2_amd._lib import KP_DTYPE
    n = len(octaves)
    kps = np.zeros(n, KP_DTYPE)
    kps["x"], kps["y"], kps["octave"], kps["size"] = np.float32(xs), np.float32(240.0), octaves, 31.0
    qd = np.zeros(32, np.uint8)
    desc = np.zeros((n, 32), np.uint8)
    for k, nb in enumerate(bits):
        desc[k, :nb // 8] = 0xFF
        desc[k, nb // 8] = (1 << (nb % 8)) - 1
    f = ProjFrame(kps, desc, [0, 0, 0, 1], [0, 0, 0], 600.0, 600.0, 320.0, 240.0, u_right=np.float32(u_right),
                  bf=48.0, b=0.08)
    return f, qd


def test_candidate_outside_the_right_radius_is_skipped_for_the_next_best():
    # the query projects to (320, 240) at z = 4: ur = 320 - 48 / 4 = 308; radius 15 * 1.2 = 18
    f, qd = _one_query_frame([1, 1, 1], [308.0 + 19.0, 308.0 + 17.0, -1.0], [321.0, 322.0, 323.0], [3, 9, 20])
    P = np.float32([[0.0, 0.0, 4.0]])
    args = (P, qd[None], np.int32([1]), np.float32([0.0]), 15.0, False)
    pose = (np.float32([0, 0, 0, 1]), np.float32([0, 0, 0.02]))       # neither forward nor backward
    st = {}
    n, m, d = S.search_by_projection_last(f, *args, last_pose=pose, stats=st)
    assert (n, m[0], d, st["gated"]) == (1, 1, 0, 1)                  # keypoint 0 is the best but gated
    f.u_right = np.float32([-1.0, -1.0, -1.0])
    assert S.search_by_projection_last(f, *args, last_pose=pose)[1][0] == 0
    # SearchLocalPoints: level 1, viewCos 1: radius 2.5 * 1.2 = 3; keypoint 0's right coordinate is 12 off
    f2, _ = _one_query_frame([0, 0], [308.0 + 12.0, 308.0 + 1.0], [320.5, 321.0], [2, 30])
    r = S.search_local_points(f2, P, np.float32([[0, 0, 1]]), np.float32([1.0]), np.float32([4.0 * 1.2 ** 0.5]), qd[None],
                              nnratio=0.9)
    assert r[2][0] == 1 and r[3][0] == 1 and r[4][0] == np.float32(308.0)
    assert r[1][0] == 1                                               # keypoint 0 gated, next best taken


@pytest.mark.parametrize("tz,octave,want_dir,levels", [
    (0.3, 0, 1, range(0, 8)),        # forward, nLastOctave 0: (0, -1), no level test at all
    (0.3, 3, 1, range(3, 8)),        # forward: nLastOctave and up
    (-0.3, 7, -1, range(0, 8)),      # backward at the top octave: 0 .. 7
    (-0.3, 2, -1, range(0, 3)),      # backward: 0 .. nLastOctave
    (0.02, 3, 0, range(2, 5)),       # neither: nLastOctave - 1 .. + 1
])
def test_direction_selects_the_level_window(tz, octave, want_dir, levels):
    """One query, eight keypoints (one per octave) whose distance grows with the octave: the match
    is the lowest octave the window admits."""
    f, qd = _one_query_frame(list(range(8)), [-1.0] * 8, [320.0 + 0.25 * k for k in range(8)],
                             [2 + 3 * k for k in range(8)])
    P = np.float32([[0.0, 0.0, 4.0]])
    # Tcw = identity: twc = 0, tlc = tlw
    n, m, d = S.search_by_projection_last(f, P, qd[None], np.int32([octave]), np.float32([0.0]), 15.0, False,
                                          last_pose=(np.float32([0, 0, 0, 1]), np.float32([0, 0, tz])))
    assert d == want_dir and n == 1 and m[0] == min(levels)
    f.claimed = np.zeros(8, np.uint8)
    f.claimed[list(levels)] = 1                                       # nothing outside the window is taken
    assert S.search_by_projection_last(f, P, qd[None], np.int32([octave]), np.float32([0.0]), 15.0, False,
                                       last_pose=(np.float32([0, 0, 0, 1]), np.float32([0, 0, tz])))[0] == 0


# ---------------------------------------------------------------- 3. the GPU cases are honest
def test_gpu_pose_cases_are_order_stable():
    unstable = [nm for nm in C.pose_names() if not C.order_stability(nm)[0]]
    assert unstable == []
    for nm in C.TRIALS_STABLE:
        assert C.order_stability(nm)[1], nm


def test_gpu_pose_cases_are_not_trivial():
    for n in C.MIXED_N[1:]:
        st = C.pose_case(f"mixed{n}").u_right >= 0
        assert 0.2 < st.mean() < 0.8, n
    # outliers of both kinds inside the register cache (128 edges at 1 wave, 1024 at 4) and past it
    for n, cache in [(129, 128), (1025, 128), (1030, 128), (1030, 1024)]:
        p, out = C.pose_case(f"boundary{n}"), C.pose_ref(f"boundary{n}")["outlier"].astype(bool)
        st = p.u_right >= 0
        assert (out & st)[:cache].any() and (out & ~st)[:cache].any() and not out[:cache].all()
        assert out[cache:].any()
        if n != 129:
            assert (out & st)[cache:].any() and (out & ~st)[cache:].any()
    assert C.pose_ref("boundary129")["outlier"][128] == 1 and C.pose_case("boundary129").u_right[128] >= 0
    assert C.pose_ref("boundary1025")["outlier"][1024] == 1 and C.pose_case("boundary1025").u_right[1024] < 0
    assert (C.pose_case("allstereo").u_right >= 0).all() and 0 < C.pose_ref("allstereo")["n_inliers"] < 150
    # every edge an outlier after round 0: the normalised initial pose comes back bit for bit
    p, r = C.pose_case("alloutlier"), C.pose_ref("alloutlier")
    assert r["n_inliers"] == 0 and r["outlier"].all() and r["lm_trials"] >= 10 and (p.u_right >= 0).sum() > 10
    q = p.pose_q.astype(np.float64)
    q = q / np.linalg.norm(q) * (1.0 if q[3] >= 0 else -1.0)
    assert np.array_equal(r["pose_q"], q.astype(np.float32)) and np.array_equal(r["pose_t"], p.pose_t)
    # the mirrored points carry stereo observations and end as outliers
    prob, behind = C.behind_camera_problem()
    r = C.pose_ref("behind")
    assert len(behind) == 10 and (prob.u_right[behind] >= 0).all()
    assert r["outlier"][behind].all() and 0 < r["n_inliers"] < 200
    # u_right = 0.0f edges are stereo edges (outliers here; inliers when read as monocular)
    p, r = C.pose_case("zero_ur"), C.pose_ref("zero_ur")
    assert (p.u_right[[5, 20, 41]] == 0).all() and r["outlier"][[5, 20, 41]].all()
    # the batch mixes the kinds, with n = 0, 1, 2 among them
    kinds = [(C.pose_case(f"batch{i}").u_right >= 0) for i in range(len(C.BATCH_N))]
    assert [len(k) for k in kinds][:3] == [0, 1, 2]
    assert any(len(k) > 2 and not k.any() for k in kinds) and any(len(k) > 2 and k.all() for k in kinds)
    assert any(k.any() and not k.all() for k in kinds)


@pytest.mark.parametrize("motion", C.MOTIONS)
def test_gpu_matcher_scenes_are_honest(motion):
    s = C.scene(motion)
    d, z = S.direction(C.frame(s), C.last_pose(s), s["b"])
    assert d == s["direction"] and abs(abs(z) - s["b"]) >= 1e-3
    th, ori = C.LAST_PARAMS[0]
    a, b = C.last_ref(motion, th, ori), C.last_ref(motion, th, ori, dropped=True)
    assert a[2] == d and a[3] >= 1 and (a[1] != b[1]).mean() >= 0.05
    th, ratio, far = C.LOCAL_PARAMS[0]
    a, b = C.local_ref(motion, th, ratio, far), C.local_ref(motion, th, ratio, far, dropped=True)
    assert a[5] >= 1 and (a[1] != b[1]).mean() >= 0.05
    for prm in C.LAST_PARAMS:
        assert C.last_ref(motion, *prm)[3] >= 1
    for prm in C.LOCAL_PARAMS:
        assert C.local_ref(motion, *prm)[5] >= 1


def test_stereo_generators_leave_the_monocular_ones_alone():
    p, _ = synthetic_stereo_pose_problem(n=50, seed=4)
    q, _ = synthetic_pose_problem(n=50, seed=4)
    assert np.array_equal(p.uv, q.uv) and np.array_equal(p.points, q.points) and q.u_right is None and p.bf > 0
    s = synthetic_stereo_projection_scene(n_kp=60, n_mp=40, seed=6, level_frac=0.0)
    t = synthetic_projection_scene(n_kp=60, n_mp=40, seed=6)
    assert all(np.array_equal(s[k], t[k]) for k in t)
    assert q.normalized().u_right is None and q.to_c().n == 50
