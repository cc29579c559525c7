"""The rule of CreateNewMapPoints (DESIGN.md "CreateNewMapPoints") on the CPU: the numpy
restatement (tests/create_points_numpy.py) against cases whose answer follows from the definition,
the accuracy of its fp64 Jacobi against LAPACK, the Conditions on the parity scene set that
tests/test_create_points_gpu.py runs the library on, and the claim rule against a sequential
simulation of upstream's loop. No GPU.

Statuses 4 (null vector with w == 0) and 9 (a point on a camera centre) do not occur in the parity
scenes: they are covered by the direct cases here and, on the device, by the same cases in
tests/test_create_points_gpu.py."""
import collections

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE
from orb_slam3_ros2_amd.matcher import TriKeyFrame
from orb_slam3_ros2_amd.synthetic import orb_scale_tables

import create_points_numpy as C

SF, S2 = orb_scale_tables()
CAM = dict(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
IDENT = (0.0, 0.0, 0.0, 1.0)


def keyframe(pixels, octaves, q=IDENT, t=(0, 0, 0)):
    """A keyframe of the given pixels (descriptors and FeatureVector are not read by the triangulation)."""
    n = len(pixels)
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = np.asarray(pixels, np.float64).reshape(n, 2).T
    k["octave"] = octaves
    return TriKeyFrame(k, np.zeros((n, 32), np.uint8), np.zeros(n, np.int32), np.ones(n), np.zeros(n, np.uint8), q, t,
                       CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])


def rot_y(deg):
    a = np.deg2rad(deg) / 2
    return (0.0, float(np.sin(a)), 0.0, float(np.cos(a)))


def rot64(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def proj(P, q=IDENT, c=(0, 0, 0)):
    """The pixel of world point P in the camera of orientation q centred at c (float64)."""
    X = rot64(q) @ (np.asarray(P, np.float64) - np.asarray(c, np.float64))
    return np.array([CAM["fx"] * X[0] / X[2] + CAM["cx"], CAM["fy"] * X[1] / X[2] + CAM["cy"]])


def pose_t(q, c):
    return tuple(-(rot64(q) @ np.asarray(c, np.float64)))


def direct_cases():
    """name -> (kf1, kf2, expected statuses, keyword arguments): one pair each, KF1 at the origin."""
    P, c2 = np.array([0.3, -0.2, 4.0]), np.array([0.5, 0.0, 0.0])
    cases = {}

    def add(name, p1, p2, want, o1=0, o2=0, q2=IDENT, c=c2, **kw):
        cases[name] = (keyframe([p1], [o1]), keyframe([p2], [o2], q2, pose_t(q2, c)), want, kw)
    add("accepted", proj(P), proj(P, c=c2), (1,))
    Pfar = P / 4.0 * 500.0
    add("at 500 m", proj(Pfar), proj(Pfar, c=c2), (3,))
    add("KF2 turned by 100 degrees", proj(P), (320.0, 240.0), (2,), q2=rot_y(100.0))
    add("swapped rays", proj(P, c=c2), proj(P), (5, 6))
    # The null vector of A leaves half of a shift off the epipolar line in the shifted image, whatever
    # the depths (the other image takes the rest, scaled by the ratio of the depths): a shift of 3 sigma
    # is an error of 1.5 sigma, 2.25 sigma^2 < 5.991 sigma^2, accepted. An ERROR of 3 sigma in the one
    # image (9 sigma^2) takes a shift of 6 sigma; in image 2 the point is also 5 times nearer to KF2,
    # so that image 1's share (0.6 sigma) passes its gate first. (First order, and exact enough in a
    # scene measured in metres; test_status_8_occurs_in_the_parity_set is about where it is not.)
    near1, cb = np.array([0.3, -0.2, 1.0]), np.array([0.5, 0.0, -4.0])
    a, b = proj(near1), proj(near1 + 0.2 * (near1 - cb))      # KF2's ray in image 1
    nrm = np.array([-(b - a)[1], (b - a)[0]]) / np.linalg.norm(b - a)
    add("3 sigma error in image 1", proj(near1) + 6.0 * nrm, proj(near1, c=cb), (7,), c=cb)
    ca = np.array([0.5, 0.0, 3.2])
    a, b = proj(P, c=ca), proj(P * 1.2, c=ca)
    nrm = np.array([-(b - a)[1], (b - a)[0]]) / np.linalg.norm(b - a)
    add("3 sigma error in image 2", proj(P), proj(P, c=ca) + 6.0 * nrm, (8,), c=ca)
    add("octaves 0 against 5", proj(P), proj(P, c=c2), (11,), o1=0, o2=5)
    add("far threshold below the depth", proj(P), proj(P, c=c2), (10,), far=3.0)
    # both rays along the optical axes of two parallel cameras: the null vector is (0, 0, 1, 0) exactly
    add("point at infinity", (320.0, 240.0), (320.0, 240.0), (4,), cos_max=2.0)
    # the same scene in units of 1e-25: z1 > 0, and the squared distance underflows to zero
    add("squared distance underflows", proj(P), proj(P, c=c2), (9,), c=c2 * 1e-25)
    return cases


DIRECT = direct_cases()


@pytest.mark.parametrize("name", list(DIRECT))
def test_direct_case(name):
    k1, k2, want, kw = DIRECT[name]
    st, X = C.triangulate_pair(C.Camera(k1), C.Camera(k2), k1.kps[0], k2.kps[0], SF, S2, **kw)
    assert st in want, (name, st)
    if name == "accepted":
        # pixels and the entries of A carry fp32 roundings (2^-24 relative, a dozen of them per ray):
        # a ray is off by < 1e-6 rad, and at 4 m over a 0.5 m baseline the depth moves by
        # z^2 / b = 32 m per rad: 3.2e-5 m. Bound: 5e-5 m
        assert np.abs(X.astype(np.float64) - [0.3, -0.2, 4.0]).max() < 5e-5
    if st in (2, 3, 4):
        assert not X.any()


def test_gate_on_the_median_depth():
    k1, k2 = keyframe([(1, 1)], [0]), keyframe([(1, 1)], [0], t=pose_t(IDENT, (0.5, 0, 0)))
    assert C.gated(C.Camera(k1), C.Camera(k2), 100 * 0.5 + 1)
    assert not C.gated(C.Camera(k1), C.Camera(k2), 4.0)
    r = C.create_new_map_points(k1, [k2], SF, S2, 0, median_depth=[51.0])
    assert r.gated.tolist() == [1] and r.nmatches.tolist() == [0] and not r.status.any() and (r.match12 == -1).all()
    assert r.n == 0


# ---- the parity scene set ----
PARITY_SEEDS = (0, 1, 2, 3)
_cache = {}


def parity_scene(k):
    """Scene k of the set: n = 300, B = 3 plus the gated neighbour (built once; read-only)."""
    if k not in _cache:
        from orb_slam3_ros2_amd.synthetic import synthetic_new_points_scene
        _cache[k] = synthetic_new_points_scene(300, 3, PARITY_SEEDS[k])
    return _cache[k]


def parity_result(k, ori=0, details=None):
    """The restatement on scene k (check_orientation 0 is cached)."""
    s = parity_scene(k)
    key = ("r", k, ori)
    if details is not None or key not in _cache:
        r = C.create_new_map_points(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], ori,
                                    s["median_depth"], far=s["far_threshold"], details=details)
        if details is not None:
            return r
        _cache[key] = r
    return _cache[key]


def test_parity_scene_conditions():
    total = collections.Counter()
    differs = 0
    for k in range(len(PARITY_SEEDS)):
        s, r = parity_scene(k), parity_result(k)
        assert len(s["neighbours"]) == 4 and s["kf1"].n == 300
        assert r.gated.tolist() == s["gated"].tolist() == [0, 1, 0, 0]
        assert r.nmatches[1] == 0 and (r.nmatches[[0, 2, 3]] > 0).all()
        c = collections.Counter(r.status.ravel().tolist())
        total.update(c)
        assert c[1] >= 100, (k, c)
        assert int(((r.status == 1).sum(0) > 1).sum()) >= 20      # the claim rule decides something
        lowest = np.where((r.match12 >= 0).any(0), (r.match12 >= 0).argmax(0), -1)
        differs += int(((r.first >= 0) & (r.first != lowest)).any())
        assert r.n == int((r.first >= 0).sum()) == int(r.nnew.sum()) <= 300
    for st in (1, 2, 3, 5, 6, 7, 8, 10, 11):
        assert total[st] >= 3, (st, total)
    assert total[4] == 0 and total[9] == 0                        # direct cases only (module docstring)
    assert differs >= 1


def test_status_8_occurs_in_the_parity_set():
    """Image 2 alone fails its 5.991 gate on pairs the search admitted within its 3.84 gate. To first
    order that cannot happen (the triangulated point reprojects no further from the twin than the
    twin lies from the epipolar line), and in a scene measured in metres no searched pair did
    (150,000 sampled). The scenes are in a monocular map's small unit (synthetic_new_points_scene,
    scale): there the null vector, normalised with its fourth component, weighs an image's residual
    with the point's depth in it, and at low parallax the point slides towards KF2 along KF1's ray.
    The generator plants such pairs on the forward neighbour (kind reproj2)."""
    total = collections.Counter()
    for k in range(len(PARITY_SEEDS)):
        s, r = parity_scene(k), parity_result(k)
        total.update(r.status.ravel().tolist())
        planted = [(b, i) for kind, b, i, _ in s["plants"] if kind == "reproj2"]
        assert planted and all(r.match12[b, i] >= 0 for b, i in planted)      # the search took them
    assert total[8] >= 3, total


def test_jacobi_beats_lapack_in_float32():
    """The null vector of the restatement before rounding, against numpy's SVD in float64, on every
    system of the parity scenes that passed the parallax gate: its largest deviation, relative to the
    distance from KF1, is no larger than that of numpy's SVD in float32 on the same A."""
    ours, lapack32, count = 0.0, 0.0, 0
    for k in range(len(PARITY_SEEDS)):
        details = []
        parity_result(k, details=details)
        Ow1 = np.array(C.Camera(parity_scene(k)["kf1"]).Ow, np.float64)
        for _, _, d in details:
            if "v" not in d:
                continue
            A = np.array(d["A"], np.float32)
            v64 = np.linalg.svd(A.astype(np.float64))[2][3]
            x64 = v64[:3] / v64[3]
            v32 = np.linalg.svd(A)[2][3]
            x32 = (v32[:3] / v32[3]).astype(np.float64)
            x = np.array(d["v"][:3]) / d["v"][3]
            dist1 = np.linalg.norm(x64 - Ow1)
            ours = max(ours, np.abs(x - x64).max() / dist1)
            lapack32 = max(lapack32, np.abs(x32 - x64).max() / dist1)
            count += 1
    print(f"systems {count}: Jacobi fp64 {ours:.3g}, LAPACK float32 {lapack32:.3g}")
    assert count >= 1000
    assert ours <= lapack32


@pytest.mark.parametrize("k", range(len(PARITY_SEEDS)))
def test_claim_equals_the_sequence(k):
    """Upstream's sequential loop (a feature triangulated with neighbour b has a MapPoint when
    neighbour b + 1 is searched) yields exactly the list of the batched rule, check_orientation = 0."""
    s, r = parity_scene(k), parity_result(k)
    nbr, idx1, idx2, x3d = C.sequential(s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"], 0,
                                        s["median_depth"], far=s["far_threshold"])
    assert nbr.tolist() == r.new_nbr.tolist() and idx1.tolist() == r.new_idx1.tolist()
    assert idx2.tolist() == r.new_idx2.tolist()
    assert np.array_equal(x3d.view(np.uint32), np.ascontiguousarray(r.new_x3d).view(np.uint32))
    assert len(nbr) >= 80


def test_generator_leaves_the_base_scene_alone():
    """synthetic_triangulation_scene's outputs for the seeds of the SearchForTriangulation parity
    set (n = 300, B = 3, seeds 0-2) are what they were before synthetic_new_points_scene was added
    (digests of every keyframe's arrays, taken on the commit before), also after the new generator
    has run: it draws from a generator of its own."""
    import hashlib
    from orb_slam3_ros2_amd.synthetic import synthetic_new_points_scene, synthetic_triangulation_scene
    synthetic_new_points_scene(120, 3, seed=1)
    for seed, want in ((0, "130b9592e4702d3e"), (1, "685f4faabb9ff276"), (2, "402344765b7dcbbb")):
        s = synthetic_triangulation_scene(300, 3, seed)
        h = hashlib.sha256()
        for k in [s["kf1"]] + s["neighbours"]:
            for a in (k.kps, k.desc, k.node, k.weight, k.has_mp, k.pose_q, k.pose_t):
                h.update(np.ascontiguousarray(a).tobytes())
        assert h.hexdigest()[:16] == want, seed
