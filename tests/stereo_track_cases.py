"""The named problems and scenes of the rectified-stereo tracking tests, built once per process and
never modified. tests/test_stereo_track_gpu.py runs them on the device; tests/test_stereo_track.py
shows on the CPU that each is an honest case for the comparison (see there)."""
import numpy as np

import stereo_track_numpy as S
from orb_slam3_ros2_amd.matcher import ProjFrame
from orb_slam3_ros2_amd.optimizer import PoseProblem
from orb_slam3_ros2_amd.synthetic import (synthetic_pose_problem, synthetic_stereo_pose_problem,
                                          synthetic_stereo_projection_scene)

# ---------------------------------------------------------------- PoseOptimization
MIXED_N = [3, 9, 10, 63, 64, 65]
BOUNDARY_N = [127, 128, 129, 1023, 1024, 1025, 1030]   # EC * NT: 128 edges (1 wave), 1024 (4 waves)
BATCH_N = [0, 1, 2, 3, 10, 40, 64, 100]               # kinds rotate: monocular-only, stereo-only, mixed
PART_B = 5
# name -> seed; a seed whose restatement flags depend on the edge order is replaced here (the CPU
# test asserts the stability of every case), no comparison is loosened and no edge left out
SEEDS = {f"mixed{n}": 700 + n for n in MIXED_N} | {f"boundary{n}": 800 + n for n in BOUNDARY_N} | \
        {"allstereo": 901, "alloutlier": 1000, "behind": 61, "zero_ur": 903} | \
        {f"batch{i}": 920 + i for i in range(len(BATCH_N))} | {f"part{i}": 940 + i for i in range(PART_B)}
TRIALS_STABLE = ["alloutlier"]                         # the cases whose lm_trials are compared too

_POSE = {}


def _force_outlier(p, e, stereo):
    """Edge e becomes a gross outlier of the given kind."""
    if stereo:
        if p.u_right[e] < 0:
            p.u_right[e] = np.float32(max(1.0, p.uv[e, 0] - 15.0))
        p.u_right[e] += np.float32(60.0)
    else:
        p.u_right[e] = -1.0
        p.uv[e] = (p.uv[e] + np.float32([90.0, -70.0])) % np.float32([640.0, 480.0])


def _build_pose(name):
    seed = SEEDS[name]
    if name.startswith("mixed"):
        return synthetic_stereo_pose_problem(n=int(name[5:]), outlier_frac=0.2, seed=seed)[0]
    if name.startswith("boundary"):
        n = int(name[8:])
        p = synthetic_stereo_pose_problem(n=n, outlier_frac=0.2, seed=seed)[0]
        if n == 129:
            _force_outlier(p, 128, True)
        if n == 1025:
            _force_outlier(p, 1024, False)
        if n == 1030:
            _force_outlier(p, 1024, False)
            _force_outlier(p, 1026, True)
        return p
    if name == "allstereo":
        return synthetic_stereo_pose_problem(n=150, outlier_frac=0.1, seed=seed, stereo_frac=1.0)[0]
    if name == "alloutlier":
        return synthetic_stereo_pose_problem(n=64, outlier_frac=1.0, seed=seed)[0]
    if name == "behind":
        return behind_camera_problem()[0]
    if name == "zero_ur":
        p = synthetic_stereo_pose_problem(n=64, outlier_frac=0.1, seed=seed)[0]
        p.u_right[[5, 20, 41]] = 0.0                   # 0.0f is a stereo observation (upstream tests < 0)
        return p
    if name.startswith("batch"):
        i = int(name[5:])
        kind = i % 3
        if kind == 0:                                  # a monocular frame in a stereo batch: all -1
            p = synthetic_pose_problem(n=BATCH_N[i], outlier_frac=0.2, seed=seed)[0]
            p.u_right, p.bf = np.full(BATCH_N[i], -1.0, np.float32), 0.0
            return p
        return synthetic_stereo_pose_problem(n=BATCH_N[i], outlier_frac=0.2, seed=seed,
                                             stereo_frac=1.0 if kind == 1 else 0.5)[0]
    if name.startswith("part"):
        return synthetic_stereo_pose_problem(n=3 + 4 * int(name[4:]), outlier_frac=0.2, seed=seed)[0]
    raise KeyError(name)


def behind_camera_problem(n=200, frac=0.05):
    """5 % of the map points mirrored behind the camera, each carrying a stereo observation."""
    seed = SEEDS["behind"]
    prob, gt = synthetic_stereo_pose_problem(n=n, outlier_frac=0.1, seed=seed)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    behind = np.sort(rng.choice(n, size=int(round(n * frac)), replace=False))
    Xc = prob.points.astype(np.float64) @ gt["R"].T + gt["t"]
    Xc[behind, 2] = -Xc[behind, 2]
    prob.points = ((Xc - gt["t"]) @ gt["R"]).astype(np.float32)
    ur = prob.u_right.copy()
    ur[behind] = np.maximum(prob.uv[behind, 0] - np.float32(12.0), np.float32(1.0))
    prob.u_right = ur
    return prob, behind


def pose_names():
    return list(SEEDS)


def pose_case(name):
    if name not in _POSE:
        _POSE[name] = _build_pose(name)
    return _POSE[name]


_POSE_REF = {}


def pose_ref(name):
    """The restatement's result for a named case, computed once and left unchanged."""
    if name not in _POSE_REF:
        _POSE_REF[name] = S.pose_optimization(pose_case(name))
    return _POSE_REF[name]


def permuted(prob, perm):
    return PoseProblem(prob.pose_q, prob.pose_t, prob.points[perm], prob.uv[perm], prob.octave[perm], prob.inv_sigma2,
                       prob.fx, prob.fy, prob.cx, prob.cy, None if prob.u_right is None else prob.u_right[perm],
                       prob.bf)


def order_stability(name, n_perm=8):
    """(flags stable, lm_trials stable) of the restatement under n_perm random edge permutations."""
    prob, ref = pose_case(name), pose_ref(name)
    rng = np.random.Generator(np.random.PCG64(77))
    flags, trials = True, True
    for _ in range(n_perm):
        perm = rng.permutation(prob.points.shape[0])
        r = S.pose_optimization(permuted(prob, perm))
        out = np.empty_like(r["outlier"])
        out[perm] = r["outlier"]
        flags &= bool(np.array_equal(out, ref["outlier"])) and r["n_inliers"] == ref["n_inliers"]
        trials &= r["lm_trials"] == ref["lm_trials"]
    return flags, trials


# ---------------------------------------------------------------- the projection matchers
MOTIONS = ["forward", "backward", "neutral"]
SCENE_SEED = {"forward": 71, "backward": 72, "neutral": 73}
LAST_PARAMS = [(15.0, True), (7.0, False)]             # (th, check_orientation)
LOCAL_PARAMS = [(1.0, 0.8, False), (3.0, 0.8, False), (5.0, 0.6, True)]   # (th, nnratio, far_points), th_far 5
RAGGED = [(n_kp, n_mp) for n_kp in (255, 256, 257) for n_mp in (1, 3, 5)]

_SCENES = {}


def scene(name):
    """'forward' / 'backward' / 'neutral': the three stereo scenes both searches run;
    'ragged{n_kp}_{n_mp}', 'nokp' (an empty frame), 'nomp' (zero map points)."""
    if name not in _SCENES:
        if name in MOTIONS:
            s = synthetic_stereo_projection_scene(n_kp=800, n_mp=700, seed=SCENE_SEED[name], motion=name)
        elif name.startswith("ragged"):
            n_kp, n_mp = (int(v) for v in name[6:].split("_"))
            s = synthetic_stereo_projection_scene(n_kp=n_kp, n_mp=n_mp, seed=80 + n_kp + n_mp,
                                                  motion=MOTIONS[(n_kp + n_mp) % 3])
        elif name == "nokp":
            s = synthetic_stereo_projection_scene(n_kp=100, n_mp=50, seed=30, motion="forward")
            s = dict(s, kps=s["kps"][:0], desc=s["desc"][:0], claimed=s["claimed"][:0], u_right=s["u_right"][:0])
        elif name == "nomp":
            s = synthetic_stereo_projection_scene(n_kp=300, n_mp=0, seed=31, motion="backward")
        else:
            raise KeyError(name)
        _SCENES[name] = s
    return _SCENES[name]


def frame(s, stereo=True, u_right=None):
    """The scene's ProjFrame; stereo False: the monocular frame (u_right dropped)."""
    f = ProjFrame(s["kps"], s["desc"], s["pose_q"], s["pose_t"], s["fx"], s["fy"], s["cx"], s["cy"],
                  claimed=s["claimed"])
    if stereo:
        f.u_right = s["u_right"] if u_right is None else u_right
        f.bf, f.b = s["bf"], s["b"]
    return f


def last_pose(s):
    return s["last_pose_q"], s["last_pose_t"]


_MATCH_REF = {}


def last_ref(name, th, ori, dropped=False):
    """The restatement's (nmatches, match, direction, gated) of SearchByProjection(last frame);
    dropped: with every u_right -1 (the same direction and level window, no gate)."""
    key = ("last", name, th, ori, dropped)
    if key not in _MATCH_REF:
        s = scene(name)
        ur = np.full(len(s["kps"]), -1.0, np.float32) if dropped else None
        st = {}
        r = S.search_by_projection_last(frame(s, u_right=ur), s["points"], s["mp_desc"], s["last_octave"],
                                        s["last_angle"], th, ori, last_pose=last_pose(s), stats=st)
        _MATCH_REF[key] = r + (st["gated"],)
    return _MATCH_REF[key]


def local_ref(name, th, ratio, far, dropped=False):
    """The restatement's (nmatches, match, in_view, level, proj_xr, gated) of SearchLocalPoints."""
    key = ("local", name, th, ratio, far, dropped)
    if key not in _MATCH_REF:
        s = scene(name)
        ur = np.full(len(s["kps"]), -1.0, np.float32) if dropped else None
        st = {}
        r = S.search_local_points(frame(s, u_right=ur), s["points"], s["normals"], s["min_dist"], s["max_dist"],
                                  s["mp_desc"], s["skip"], th=th, nnratio=ratio, far_points=far, th_far=5.0, stats=st)
        _MATCH_REF[key] = r + (st["gated"],)
    return _MATCH_REF[key]
