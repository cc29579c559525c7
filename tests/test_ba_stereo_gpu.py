"""GPU parity: Local / Global BundleAdjustment with EdgeStereoSE3ProjectXYZ edges
(orbhip_ba_solve_stereo, orbhip_ba_solve_stereo_batch) on gfx950 against the fp64 numpy restatement
of the oracle with the stereo edge added (tests/ba_stereo_numpy.py, proven in test_ba_stereo.py).

Tolerances are the suite's: REL (1e-4) on poses, points and chi2, the LM schedule equal for runs that
end on the iteration budget, erase flags equal except where the reference's chi2 is within 1e-3 of
the edge's threshold (7.815 stereo, 5.991 monocular)."""
import ctypes
import functools

import numpy as np
import pytest

from orb_slam3_ros2_amd.optimizer import StereoBAProblem
from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem, synthetic_stereo_ba_problem
from tests.ba_stereo_cases import compare_ba_stereo, edge_count_problem, wide_pose_problem
from tests.ba_stereo_numpy import ba_solve as ref_solve
from tests.helpers import REL, qsign

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def opt():
    from orb_slam3_ros2_amd import Optimizer
    return Optimizer()


def _mixed(nkf, npts, seed):
    return synthetic_stereo_ba_problem(n_kf=nkf, n_pts=npts, seed=seed, stereo_frac=0.7)[0]


def _rejecting():
    # a large initial perturbation: the restatement rejects 2 of its 12 trials over optimize(10)
    p = synthetic_stereo_ba_problem(n_kf=12, n_pts=300, seed=30, stereo_frac=0.7, rot_noise=0.1, trans_noise=0.2,
                                    pt_noise=0.5)[0]
    p.pose_fixed[:2] = 1
    return p


_CASES = {"8x100": lambda: _mixed(8, 100, 1), "20x600": lambda: _mixed(20, 600, 2), "counts": edge_count_problem,
          "wide": wide_pose_problem, "rejecting": _rejecting}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(problem, the restatement's solve of it): computed once, shared by the tests, never changed."""
    p = _CASES[name]()
    return p, ref_solve(p)


@pytest.mark.parametrize("name", ["8x100", "20x600"])
def test_mixed_problems(opt, name):
    p, o = _case(name)
    st = p.edge_ur >= 0
    assert st.any() and (~st).any()
    g = opt.LocalBundleAdjustment(p)
    compare_ba_stereo(g, o, p)
    assert g.final_chi2 < 0.1 * g.initial_chi2


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("ppw", ["1", "4"])
@pytest.mark.parametrize("name", ["counts", "wide"])
def test_edge_count_shapes(opt, monkeypatch, name, ppw, fused):
    """Every loop form of the edge kernels. `counts`: landmarks with 1, 2, 3, 4, 5 and 9 observations,
    one 9-observation landmark with its stereo edge past the two preloaded edges of its lane in
    k_ba_backsub_errs, one with them among the preloaded. `wide`: 400 edges per pose (several
    rounds of lin_pose's wave and of lin_pose_wg's work-group), a pose with only stereo edges, one
    with only monocular ones, a fixed pose with stereo edges. Both pose linearisations
    (ORBHIP_LIN_PPW) and both trial forms (ORBHIP_BA_FUSED)."""
    monkeypatch.setenv("ORBHIP_LIN_PPW", ppw)
    monkeypatch.setenv("ORBHIP_BA_FUSED", fused)
    p, o = _case(name)
    compare_ba_stereo(opt.solve_stereo(p), o, p)


def test_large_problem_path(opt, monkeypatch):
    """ORBHIP_BA_SMALL_WORDS=0: the rejected trial's points come back in k_ba_pop, not in the trial's
    last work-group."""
    monkeypatch.setenv("ORBHIP_BA_SMALL_WORDS", "0")
    p, o = _case("20x600")
    compare_ba_stereo(opt.solve_stereo(p), o, p)


def test_zero_right_coordinate_is_a_stereo_edge(opt):
    """edge_ur == 0.0f exactly: a stereo edge (the rule is >= 0), here a gross one, since the true
    right coordinates are far from 0. Read as monocular edges they would leave chi2 small."""
    p = _mixed(8, 100, 3)
    p.edge_ur[::17] = 0.0
    o = ref_solve(p)
    assert (o["edge_chi2"][::17] > 7.815).all()
    g = opt.solve_stereo(p)
    compare_ba_stereo(g, o, p)
    assert (g.edge_chi2[::17] > 7.815).all()


@pytest.mark.parametrize("kind", ["ur", "uv"])
def test_gross_errors_take_each_huber_branch(opt, kind):
    """+35 px on the right coordinate of every 23rd stereo edge (the stereo edges' Huber branch
    alone), or on the keypoint of every 23rd edge (both kinds'): the robust weights differ from 1 on
    edges of the kind meant, and the flagged edges agree."""
    p = _mixed(12, 300, 4)
    st = np.nonzero(p.edge_ur >= 0)[0]
    if kind == "ur":
        p.edge_ur[st[::23]] += 35.0
        hit_s, hit_m = st[::23], np.zeros(0, np.int64)
    else:
        p.edge_uv[::23] += 35.0
        hit = np.arange(p.edge_ur.shape[0])[::23]
        hit_s, hit_m = hit[p.edge_ur[hit] >= 0], hit[p.edge_ur[hit] < 0]
        assert len(hit_m) > 0
    o = ref_solve(p)
    assert len(hit_s) > 0 and (o["edge_chi2"][hit_s] > 7.815).all() and (o["edge_chi2"][hit_m] > 5.991).all()
    g = opt.solve_stereo(p)
    compare_ba_stereo(g, o, p)
    flagged = g.outlier_edges(p.edge_thresholds())
    assert set(hit_s.tolist()) | set(hit_m.tolist()) <= set(flagged.tolist())


def test_gba_no_robust_kernel(opt):
    """BundleAdjustment(bRobust = false): both deltas 0, 20 iterations (run to convergence, where the
    stop on rho == 0 is rounding noise: exact_schedule=False as in test_ba_gpu.py)."""
    p = _mixed(12, 300, 10)
    g = opt.BundleAdjustment(p, nIterations=20, bRobust=False)
    q = StereoBAProblem(**{**p.__dict__, "iterations": 20, "huber_delta": 0.0, "huber_delta_stereo": 0.0})
    compare_ba_stereo(g, ref_solve(q), q, exact_schedule=False)


@pytest.mark.parametrize("fused", ["0", "1"])
def test_rejected_trials(opt, monkeypatch, fused):
    """A perturbation large enough for the LM to reject trials: the pushed state comes back (both
    trial forms). Points to 1e-3, as in test_ba_gpu.py::test_rejected_trials_restore_across_workgroups
    and for its reason (a few landmarks stay weakly constrained after a start this far off); poses
    and chi2 to REL."""
    monkeypatch.setenv("ORBHIP_BA_FUSED", fused)
    p, o = _case("rejecting")
    assert o["lm_trials"] > o["iterations_done"]   # the test's condition: rejected trials happened
    compare_ba_stereo(opt.solve_stereo(p), o, p, point_rel=1e-3)


def test_batch(opt):
    """B = 3 of different sizes: all stereo, mixed, no stereo edge. Each equals the restatement and
    its own single solve (another Cholesky route: REL, the same schedule)."""
    probs = [synthetic_stereo_ba_problem(n_kf=8, n_pts=150, seed=21, stereo_frac=1.0)[0], _mixed(16, 400, 22),
             synthetic_stereo_ba_problem(n_kf=12, n_pts=300, seed=24, stereo_frac=0.0)[0]]
    assert (probs[0].edge_ur >= 0).all() and (probs[2].edge_ur < 0).all()
    res = opt.solve_stereo_batch(probs)
    for p, g in zip(probs, res):
        compare_ba_stereo(g, ref_solve(p), p)
        s = opt.solve_stereo(p)
        compare_ba_stereo(g, dict(pose_q=s.pose_q, pose_t=s.pose_t, points=s.points, edge_chi2=s.edge_chi2,
                                  edge_depth_ok=s.edge_depth_ok, initial_chi2=s.initial_chi2,
                                  final_chi2=s.final_chi2, iterations_done=s.iterations_done, lm_trials=s.lm_trials),
                          p)


def _same_bits(a, b):
    assert (a.iterations_done, a.lm_trials) == (b.iterations_done, b.lm_trials)
    assert a.initial_chi2 == b.initial_chi2 and a.final_chi2 == b.final_chi2
    for k in ("pose_q", "pose_t", "points", "edge_chi2", "edge_depth_ok"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k


def test_all_monocular_problem_is_orbhip_ba_solve(opt):
    """Every edge_ur = -1 and bf = 0 through the stereo entries: orbhip_ba_solve's kernels, so the
    same bits in poses, points, edge_chi2 and the schedule; the same for a stereo batch that holds
    only such problems against orbhip_ba_solve_batch."""
    monos = [synthetic_ba_problem(n_kf=nkf, n_pts=npts, seed=s)[0] for s, nkf, npts in [(1, 8, 100), (2, 20, 600)]]
    ster = [StereoBAProblem(**m.__dict__, edge_ur=np.full(m.edge_pose.shape[0], -1.0, np.float32), bf=0.0)
            for m in monos]
    for m, s in zip(monos, ster):
        _same_bits(opt.solve_stereo(s), opt.solve(m))
    for a, b in zip(opt.solve_stereo_batch(ster), opt.solve_batch(monos)):
        _same_bits(a, b)


def test_argument_errors_leave_the_result_untouched(opt):
    """NULL edge_ur with edges, and bf 0 / -1 with a stereo edge: ORBHIP_ERR_ARG before anything
    runs, nothing written to the result."""
    from orb_slam3_ros2_amd._lib import BAResultC, BAStereoProblemC, lib, ptr
    p = _mixed(8, 100, 1).normalized()
    P, M, E = p.pose_q.shape[0], p.points.shape[0], p.edge_pose.shape[0]

    def call(pc):
        bufs = [np.full((P, 4), 7.0, np.float32), np.full((P, 3), 7.0, np.float32), np.full((M, 3), 7.0, np.float32),
                np.full(E, 7.0, np.float32), np.full(E, 7, np.uint8)]
        rc = BAResultC(*[ptr(b) for b in bufs], -1.0, -2.0, -3, -4)
        code = lib().orbhip_ba_solve_stereo(opt.ctx.handle, ctypes.byref(pc), ctypes.byref(rc), None)
        assert code == -1, code   # ORBHIP_ERR_ARG
        assert all((b == 7).all() for b in bufs)
        assert (rc.initial_chi2, rc.final_chi2, rc.iterations_done, rc.lm_trials) == (-1.0, -2.0, -3, -4)
        code = lib().orbhip_ba_solve_stereo_batch(opt.ctx.handle, ctypes.byref(pc), 1, ctypes.byref(rc), None)
        assert code == -1 and all((b == 7).all() for b in bufs)

    pc = p.to_c()
    pc.edge_ur = None
    call(pc)
    for bf in (0.0, -1.0):
        pc = p.to_c()
        pc.bf = bf
        call(pc)
    # bf <= 0 is no error without a stereo edge, and the monocular argument checks still hold
    pc = p.to_c()
    pc.mono.edge_uv = None
    call(pc)


def test_stop_flag_raised_before_the_call(opt):
    p, _ = _case("8x100")
    flag = ctypes.c_int(1)
    r = opt.solve_stereo(p, stop_flag=flag)
    assert r.iterations_done == 0 and r.final_chi2 == r.initial_chi2
    for r in opt.solve_stereo_batch([p, p], stop_flag=flag):
        assert r.iterations_done == 0
