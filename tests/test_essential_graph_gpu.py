"""Optimizer.OptimizeEssentialGraph on the device against tests/essential_graph_numpy.py: the schedule
(iterations_run, lm_trials, lm_rejected) by equality, chi2_initial relative 1e-9, chi2_final relative
1e-4, the estimates in test_sim3_opt_gpu.py's metric (rotation 1 - |q.q'| < tol^2, t by tol max(1,
|t|inf), s relative by tol, tol = 1e-4, the project's Optimizer tolerance), fixed vertices bit for
bit, and the points bit for bit as float32 against the restatement's point formula applied to the
estimates the call returned. Every scene is one of essential_graph_cases.py, which
test_essential_graph.py shows to be admissible: the restatement's own result moves by less than 1e-6
under another summation order or another solver, which leaves two decades for the device's
sin / cos / acos / exp / log (an ulp from the host's, amplified by the numeric Jacobian's 1 / 2e-9).
"""
import ctypes

import numpy as np
import pytest

import essential_graph_cases as C
import essential_graph_numpy as R
import sim3_opt_cases as S3C
from orb_slam3_ros2_amd import EssentialGraphProblem, Optimizer, OrbHipError
from orb_slam3_ros2_amd._lib import Context, EssentialGraphProblemC, EssentialGraphResultC, lib, ptr
from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem

pytestmark = pytest.mark.gpu
TOL = C.TOL
ERR_ARG, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def opt():
    return Optimizer()


def _qdist(a, b):
    return 1.0 - abs(float(np.dot(a / np.linalg.norm(a), b / np.linalg.norm(b))))


def _check(p, g, o, solver=None, tol=TOL):
    print(f"schedule {g.iterations_run}/{g.lm_trials}/{g.lm_rejected} vs {o['iterations_run']}/{o['lm_trials']}/"
          f"{o['lm_rejected']}  chi2 {g.chi2_initial:.17g} -> {g.chi2_final:.17g} vs {o['chi2_initial']:.17g} -> "
          f"{o['chi2_final']:.17g}  distance {R.sim3_distance(g.S, o['S']):.3e}  solver {g.solver}")
    assert (g.iterations_run, g.lm_trials, g.lm_rejected) == (o["iterations_run"], o["lm_trials"], o["lm_rejected"])
    assert abs(g.chi2_initial - o["chi2_initial"]) <= 1e-9 * o["chi2_initial"]
    assert abs(g.chi2_final - o["chi2_final"]) <= 1e-4 * o["chi2_final"]
    for v in range(p.S.shape[0]):
        if p.fixed[v]:
            assert np.array_equal(g.S[v], p.S[v])
            continue
        assert _qdist(g.S[v, 0:4], o["S"][v, 0:4]) < tol * tol
        assert np.abs(g.S[v, 4:7] - o["S"][v, 4:7]).max() <= tol * max(1.0, float(np.abs(o["S"][v, 4:7]).max()))
        assert abs(g.S[v, 7] - o["S"][v, 7]) <= tol * o["S"][v, 7]
    # the point formula is the reference; the Sim3 inputs are whatever the call returned
    want = R.correct_points(p.S, g.S, p.points, p.point_ref)
    assert g.points.dtype == np.float32 and g.points.shape == want.shape
    assert np.array_equal(g.points.view(np.uint32), want.view(np.uint32))
    if solver is not None:
        assert g.solver == solver


def _default_solver(name):
    return 0 if 7 * C.n_free(name) >= C.DAG_MIN_N else 1


@pytest.mark.parametrize("name", C.SCENES)
def test_scene(opt, name):
    p = C.case(name)
    g = opt.OptimizeEssentialGraph(p)
    _check(p, g, C.reference(name), _default_solver(name))


def test_consistent_graph_stops_with_the_estimates_untouched(opt):
    p = C.case("consistent")
    g = opt.OptimizeEssentialGraph(p)
    assert (g.iterations_run, g.lm_trials, g.lm_rejected) == (1, 1, 1) and g.chi2_initial == 0.0
    assert np.array_equal(g.S, p.S)


@pytest.mark.parametrize("name", ("no_edges", "no_free", "iter0"))
def test_degenerate_calls_copy_through(opt, name):
    p = C.case(name)
    g = opt.OptimizeEssentialGraph(p)
    assert np.array_equal(g.S, p.S) and g.lm_trials == 0 and g.iterations_run == 0
    assert g.chi2_initial == g.chi2_final


@pytest.mark.parametrize("name", C.BLOCKED_SCENES)
def test_blocked_solver_route(opt, name, monkeypatch):
    p = C.case(name)
    d = opt.OptimizeEssentialGraph(p)
    assert d.solver == 0
    monkeypatch.setenv("ORBHIP_EG_BLOCKED", "1")
    g = opt.OptimizeEssentialGraph(p)
    monkeypatch.delenv("ORBHIP_EG_BLOCKED")
    _check(p, g, C.reference(name), 1)
    assert (g.iterations_run, g.lm_trials, g.lm_rejected) == (d.iterations_run, d.lm_trials, d.lm_rejected)
    assert R.sim3_distance(g.S, d.S) < TOL


def test_repeated_calls_give_the_same_bits(opt):
    p = C.case("free64")
    a, b = opt.OptimizeEssentialGraph(p), opt.OptimizeEssentialGraph(p)
    assert np.array_equal(a.S, b.S) and np.array_equal(a.points, b.points) and a.chi2_final == b.chi2_final


def test_workspace_regrowth_and_shrink():
    o = Optimizer(ctx=Context())            # a fresh context: the block and the workspace start empty
    for name in ("free4", "free64", "free10", "free150", "free9"):
        p = C.case(name)
        _check(p, o.OptimizeEssentialGraph(p), C.reference(name))


def test_profile_stage_brackets_the_call(opt):
    L = lib()
    assert L.orbhip_profile_stage(opt.ctx.handle, 15) == 0
    for _ in range(3):
        opt.OptimizeEssentialGraph(C.case("free10"))
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(opt.ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(opt.ctx.handle, 0) == 0
    assert cnt.value == 3 and 0.0 < ms.value < 1000.0


# ---- interference: the staging block and the solver buffers of other calls on the same context ----
def test_after_other_optimizer_calls_on_the_same_context():
    o = Optimizer(ctx=Context())
    p = C.case("free64")
    first = o.OptimizeEssentialGraph(p)
    s3 = o.OptimizeSim3(S3C.case("size65"))
    ba = o.LocalBundleAdjustment(synthetic_ba_problem(n_kf=12, n_pts=300, seed=3)[0])
    again = o.OptimizeEssentialGraph(p)
    assert np.array_equal(first.S, again.S) and np.array_equal(first.points, again.points)
    _check(p, again, C.reference("free64"), 0)
    # and the other calls are what they are without it
    o2 = Optimizer(ctx=Context())
    s3b = o2.OptimizeSim3(S3C.case("size65"))
    assert np.array_equal(s3.q, s3b.q) and s3.n_in == s3b.n_in
    assert ba.lm_trials > 0


def test_two_contexts_back_to_back():
    a, b = Optimizer(ctx=Context()), Optimizer(ctx=Context())
    pa, pb = C.case("free150"), C.case("free64")
    ra = a.OptimizeEssentialGraph(pa)
    rb = b.OptimizeEssentialGraph(pb)
    ra2 = a.OptimizeEssentialGraph(pa)
    _check(pa, ra, C.reference("free150"), 0)
    _check(pb, rb, C.reference("free64"), 0)
    assert np.array_equal(ra.S, ra2.S)


# ---- envelope and argument errors ----
def _chain(n_free):
    n = n_free + 1
    S = np.tile(np.array([0, 0, 0, 1, 0, 0, 0, 1.0]), (n, 1))
    S[:, 4] = np.arange(n)
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    ij = np.stack([np.arange(1, n), np.arange(n - 1)], 1).astype(np.int32)
    return EssentialGraphProblem(S, fixed, ij, np.tile(np.array([0, 0, 0, 1, -1.0, 0, 0, 1.0]), (n - 1, 1)))


def test_586_free_vertices_are_unsupported(opt):
    with pytest.raises(OrbHipError) as e:
        opt.OptimizeEssentialGraph(_chain(C.MAX_FREE + 1))
    assert e.value.code == ERR_UNSUPPORTED


POISON = 0xCD


def _raw(opt, p, mutate):
    """The C call on p with `mutate(pc, arrays)` applied to the C problem, the outputs pre-filled with
    a poison value: (return code, every output still poison)."""
    p = p.normalized()
    arrays = dict(S=p.S.copy(), fixed=p.fixed.copy(), edge_ij=p.edge_ij.copy(), edge_S=p.edge_S.copy(),
                  points=p.points.copy(), point_ref=p.point_ref.copy())
    pc = EssentialGraphProblemC(p.S.shape[0], ptr(arrays["S"]), ptr(arrays["fixed"]), p.edge_ij.shape[0],
                                ptr(arrays["edge_ij"]), ptr(arrays["edge_S"]), int(p.fix_scale), p.iterations,
                                p.lambda_init, p.points.shape[0], ptr(arrays["points"]), ptr(arrays["point_ref"]))
    S = np.full(p.S.shape, np.nan)
    S.view(np.uint8)[:] = POISON
    pts = np.zeros(p.points.shape, np.float32)
    pts.view(np.uint8)[:] = POISON
    r = EssentialGraphResultC()
    ctypes.memset(ctypes.byref(r), POISON, ctypes.sizeof(r))
    r.S, r.points = ptr(S), ptr(pts)
    mutate(pc, arrays, r)
    rc = lib().orbhip_optimize_essential_graph(opt.ctx.handle, ctypes.byref(pc), ctypes.byref(r))
    raw = bytes(r)
    skip = {EssentialGraphResultC.S.offset, EssentialGraphResultC.points.offset}
    scal = all(b == POISON for k, b in enumerate(raw) if not any(o <= k < o + 8 for o in skip))
    clean = scal and (S.view(np.uint8) == POISON).all() and (pts.view(np.uint8) == POISON).all()
    return rc, bool(clean)


def _set(field, value):
    def f(pc, arrays, r):
        setattr(pc, field, value)
    return f


def _poke(name, index, value):
    def f(pc, arrays, r):
        arrays[name].reshape(-1)[index] = value
    return f


def _set_row(name, index, value):
    def f(pc, arrays, r):
        arrays[name][index] = value
    return f


def _null_result(field):
    def f(pc, arrays, r):
        setattr(r, field, None)
    return f


ARG_ERRORS = {
    "null_S": _set("S", None), "null_fixed": _set("fixed", None), "null_edge_ij": _set("edge_ij", None),
    "null_edge_S": _set("edge_S", None), "null_points": _set("points", None), "null_point_ref": _set("point_ref", None),
    "null_out_S": _null_result("S"), "null_out_points": _null_result("points"),
    "negative_vertices": _set("n_vertices", -1), "negative_edges": _set("n_edges", -1),
    "negative_points": _set("n_points", -1), "negative_iterations": _set("iterations", -1),
    "edge_index_high": _poke("edge_ij", 5, 10 ** 6), "edge_index_negative": _poke("edge_ij", 4, -1),
    "edge_self": _set_row("edge_ij", 1, (3, 3)),
    "point_ref_high": _poke("point_ref", 3, 10 ** 6), "point_ref_negative": _poke("point_ref", 0, -1),
    "nan_estimate": _poke("S", 11, np.nan), "inf_measurement": _poke("edge_S", 4, np.inf),
    "zero_scale": _poke("S", 15, 0.0), "negative_measurement_scale": _poke("edge_S", 7, -1.0),
    "lambda_zero": _set("lambda_init", 0.0), "lambda_negative": _set("lambda_init", -1e-16),
    "lambda_nan": _set("lambda_init", float("nan")),
}


@pytest.mark.parametrize("what", sorted(ARG_ERRORS))
def test_argument_errors_touch_no_output(opt, what):
    p = C.case("iter0")                                      # 8 vertices, 29 edges, 9 points
    rc, clean = _raw(opt, p, ARG_ERRORS[what])
    assert rc == ERR_ARG and clean


def test_null_problem_or_result(opt):
    p = C.case("iter0")
    pc = p.to_c()
    r = EssentialGraphResultC()
    assert lib().orbhip_optimize_essential_graph(opt.ctx.handle, None, ctypes.byref(r)) == ERR_ARG
    assert lib().orbhip_optimize_essential_graph(opt.ctx.handle, ctypes.byref(pc), None) == ERR_ARG
    assert lib().orbhip_optimize_essential_graph(None, ctypes.byref(pc), ctypes.byref(r)) == ERR_ARG


def test_a_valid_raw_call_writes_every_output(opt):
    rc, clean = _raw(opt, C.case("iter0"), lambda pc, arrays, r: None)
    assert rc == 0 and not clean
