"""Crafted OptimizeEssentialGraph scenes, shared by test_essential_graph.py (which proves that each
reaches its edge and is admissible) and test_essential_graph_gpu.py (which runs each on the device).

A scene is admissible when the restatement's result does not hang on the order of its sums: a
permuted edge order and numpy.linalg.solve in place of the LDL^T leave the accept / reject sequence
identical and the estimates within ADMIT in the device tests' metric. Seeds and iteration counts were
searched on the CPU for that; a scene that fails is replaced, not tolerated.
"""
import functools

import numpy as np

import essential_graph_numpy as R
from orb_slam3_ros2_amd import EssentialGraphProblem
from orb_slam3_ros2_amd.synthetic import synthetic_essential_graph

# the route boundaries of the implementation (csrc/essential_graph.h)
TILE = 32                # the solvers' tile: n = 28 | 35 and 63 | 70 lie on both sides of a tile edge
DAG_MIN_N = 70           # kEgDagMinN: 7 x free vertices below it take the blocked solver
MAX_FREE = 585           # 7 x 585 = 4095 <= kDagMaxN
ADMIT = 1e-6
TOL = 1e-4
# every accept / reject decision of a scene is at least this far from a tie (|chi2 - chi2'| / chi2 in
# the restatement): the device's sin / cos / acos / exp / log differ from the host's by an ulp, which
# the numeric Jacobian's 1 / 2e-9 amplifies to about 1e-7 in J; the iteration counts below end each
# scene before its decisions sink to that level
MIN_MARGIN = 1e-5

FREE_COUNTS = (1, 4, 5, 9, 10, 64, 150)          # n = 7, 28, 35, 63, 70, 448, 1050
POINT_COUNTS = (0, 1, 63, 64, 65, 5000)


def _graph(n_kf, seed, iterations, **kw):
    p, _ = synthetic_essential_graph(n_kf=n_kf, seed=seed, **kw)
    p.iterations = iterations
    return p


def _s3(q, t, s):
    return np.concatenate([np.asarray(q, np.float64), np.asarray(t, np.float64), [float(s)]])


def _axis_angle(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    h = np.radians(deg) / 2
    return np.concatenate([np.sin(h) * a, [np.cos(h)]])


def _mul(a, b):
    return R.bmul(a, b)[0]


def _inv(a):
    return R.binv(a)[0]


def _consistent(iterations=20):
    """Identity rotations, integer translations, s = 1: every product is exact, every error is
    exactly zero, so the first trial gives rho == 0 and the estimates stay bit for bit."""
    n = 6
    S = np.array([_s3([0, 0, 0, 1], [k, 2 * k, -k], 1.0) for k in range(n)])
    ij = [(i, i - 1) for i in range(1, n)] + [(5, 0), (4, 1), (2, 4)]
    Sji = [_mul(S[j], _inv(S[i])) for i, j in ij]
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    rng = np.random.default_rng(5)
    return EssentialGraphProblem(S, fixed, np.array(ij, np.int32), np.array(Sji), False, iterations, 1e-16,
                                 rng.uniform(-3, 3, (7, 3)).astype(np.float32), np.arange(7, dtype=np.int32) % n)


def _branches():
    """Vertex 0 fixed, four free vertices with one edge each to it, whose error at the first
    linearisation is the identity, a pure scale, a 60 degree rotation with s = 1, and both; three
    edges among the free vertices that agree with the estimates keep the minimum away from zero."""
    S = np.array([_s3([0, 0, 0, 1], [0, 0, 0], 1.0)] +
                 [_s3(_axis_angle([0.2, 1.0, -0.3], 10.0 * k), [k, 0.5 * k, -0.25 * k], 1.0) for k in range(1, 5)])
    errs = [_s3([0, 0, 0, 1], [0, 0, 0], 1.0), _s3([0, 0, 0, 1], [0.1, -0.05, 0.02], 1.3),
            _s3(_axis_angle([1, 2, 3], 60.0), [0.05, 0.1, -0.1], 1.0),
            _s3(_axis_angle([-1, 0.5, 2], 25.0), [-0.1, 0.02, 0.06], 0.8)]
    ij = [(k, 0) for k in range(1, 5)]
    # e = (Sji Si Sj^-1).log() with Sj = the identity: Sji = err * Si^-1
    Sji = [_mul(errs[k - 1], _inv(S[k])) for k in range(1, 5)]
    for i, j in ((2, 1), (3, 2), (4, 1)):
        ij.append((i, j))
        Sji.append(_mul(S[j], _inv(S[i])))
    fixed = np.zeros(5, np.uint8)
    fixed[0] = 1
    return EssentialGraphProblem(S, fixed, np.array(ij, np.int32), np.array(Sji), False, 3, 1e-16)


def _refixed(p, fixed_ids):
    p.fixed = np.zeros(p.S.shape[0], np.uint8)
    p.fixed[list(fixed_ids)] = 1
    return p


def _reversed(p):
    """Every other edge given as (j, i) with the inverse measurement, so that i < j."""
    ij, Sji = p.edge_ij.copy(), p.edge_S.copy()
    for e in range(0, ij.shape[0], 2):
        ij[e] = ij[e][::-1]
        Sji[e] = _inv(p.edge_S[e])
    p.edge_ij, p.edge_S = ij, Sji
    return p


def _doubled(p):
    p.edge_ij = np.concatenate([p.edge_ij, p.edge_ij[:3]])
    p.edge_S = np.concatenate([p.edge_S, p.edge_S[:3]])
    return p


def _hub(seed, iterations):
    """Keyframe 44 with 40 more edges, to keyframes 0..39, measured from the tracked poses."""
    p, info = synthetic_essential_graph(n_kf=45, seed=seed, k_covis=1, loop_span=3)
    tr = info["tracked"]
    ij = [(44, j) for j in range(40)]
    Sji = [_mul(tr[j], _inv(tr[44])) for j in range(40)]
    p.edge_ij = np.concatenate([p.edge_ij, np.array(ij, np.int32)])
    p.edge_S = np.concatenate([p.edge_S, np.array(Sji)])
    p.iterations = iterations
    return p


def _reject_accept():
    """A larger drift and a caller's lambda0 of 1e-3: the third iteration rejects six trials, then accepts."""
    p = _graph(12, 60, 3, drift=0.05, scale_drift=0.01)
    p.lambda_init = 1e-3
    return p


def _with_points(p, m, seed=3):
    rng = np.random.default_rng(seed)
    n = p.S.shape[0]
    p.points = rng.uniform(-6, 6, (m, 3)).astype(np.float32)
    p.point_ref = rng.integers(0, n, m).astype(np.int32)
    if m:
        p.point_ref[0] = int(np.nonzero(p.fixed)[0][0])   # a point whose reference is a fixed vertex
    return p


def _no_edges():
    p = _graph(6, 1, 20, n_points=9)
    p.edge_ij, p.edge_S = np.zeros((0, 2), np.int32), np.zeros((0, 8))
    return p


_BUILDERS = {
    # free-vertex counts: (n_kf, seed, iterations); keyframe 0 fixed
    "free1": lambda: _graph(2, 52, 5),          # two accepted, nine rejected, the tenth accepted
    "free4": lambda: _graph(5, 12, 5),
    "free5": lambda: _graph(6, 13, 5),
    "free9": lambda: _graph(10, 14, 5),
    "free10": lambda: _graph(11, 15, 5),
    "free64": lambda: _graph(65, 16, 4, n_points=100),
    "free150": lambda: _graph(151, 17, 4, n_points=100),
    # fixed vertices
    "fixed_middle": lambda: _refixed(_graph(12, 21, 5), [6]),
    "fixed_last": lambda: _refixed(_graph(12, 22, 5), [11]),
    "fixed_three": lambda: _refixed(_graph(12, 23, 5), [0, 1, 2]),      # edges (1,0), (2,1), (2,0): chi2 only
    # edge forms
    "reversed": lambda: _reversed(_graph(12, 24, 5)),
    "doubled": lambda: _doubled(_graph(12, 25, 3)),
    "hub40": lambda: _hub(50, 4),
    # sim3_log's branches, fix_scale
    "branches": _branches,
    "fixscale": lambda: _graph(10, 27, 2, fix_scale=True),
    # schedule
    "consistent": _consistent,
    "reject_accept": _reject_accept,
    "iter0": lambda: _graph(8, 28, 0, n_points=9),
    "iter1": lambda: _graph(8, 29, 1),
    # degenerate: the estimates copied through, the points corrected by the identity
    "no_edges": _no_edges,
    "no_free": lambda: _refixed(_graph(6, 30, 20, n_points=9), range(6)),
}
for _m in POINT_COUNTS:
    _BUILDERS[f"points{_m}"] = functools.partial(lambda m: _with_points(_graph(6, 51 + 2 * (m % 2), 4), m), _m)

SCENES = tuple(_BUILDERS)
FREE_SCENES = tuple(f"free{k}" for k in FREE_COUNTS)
BLOCKED_SCENES = ("free10", "free64", "free150")     # n = 70, 448, 1050: the default route is the DAG solver


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]().normalized()


def run(p, **kw):
    return R.optimize_essential_graph(p.S, p.fixed, p.edge_ij, p.edge_S, p.fix_scale, p.iterations, p.lambda_init,
                                      p.points, p.point_ref, **kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    return run(case(name))


def n_free(name):
    return int((case(name).fixed == 0).sum())
