"""GPU: the nested-dissection solve (ba_nd.hip) on wide bands and at the edges of its plan.

k_nd_backsolve holds two tiles per wave and interior column in registers and loads further ones
inside the step; the systems of tests/test_nd_gpu.py (w <= 19 poses) never go past the registers
(tests/test_nd_model.py). The systems here reach phase 1's in-step loads (w >= 22) and phase 2's
second slot and in-step loads (w >= 43), interiors of even and odd tile counts, an interior with
no padding, a line's first / middle / last segment, the 84-tile segment that fills the kernel's
128 KiB of LDS (also the automatic plan of that band), the second level, and the failure path.
Which path a case takes is asserted on the case's own blocks with the plan model
(tests/nd_model.py), and the device's plan (segment starts, w) is compared with the model's.

Accuracy: helpers.check_solve (backward error in long double <= ETA_CAP u, the yardstick of the
other Cholesky paths) and the forward bound 1e-9 against numpy's fp64 solve of test_nd_gpu.py.
Reference level on these matrices: numpy's solve has a backward error of 0.12 .. 0.31 u, cond_2 is
8e2 .. 3.4e3."""
import ctypes
import functools

import numpy as np
import pytest

import nd_model as M
from helpers import ETA_CAP, U, check_solve

pytestmark = pytest.mark.gpu

UNSUPPORTED, NOT_SPD = -5, -4
COND_MAX = 3.4e3   # the largest cond_2 of the systems below

# (n_pose, w, cyclic, K); the figures each reaches are pinned in tests/test_nd_model.py
SOLVES = [(100, 24, True, 2), (192, 48, True, 2), (203, 48, True, 2), (264, 65, True, 2), (150, 24, False, 2),
          (300, 48, False, 3), (576, 48, True, 6)]
CEILING = (664, 114, True, 2)
CEILING_LAND = 1200   # landmarks of the 664-pose system (the default 6 n_pose takes 20 s to build)


@functools.lru_cache(maxsize=None)
def system(n_pose, w, cyclic, n_land=None):
    """(A, b, bi, bj) of synthetic.banded_pose_system, built once and never written (the tests
    that change an entry copy A); its measured band is the w it was asked for."""
    from orb_slam3_ros2_amd.synthetic import banded_pose_system
    A, b, bi, bj = banded_pose_system(n_pose, w, cyclic, seed=n_pose + w, n_land=n_land)
    assert M.band_of(n_pose, bi, bj) == (w, cyclic)
    for a in (A, b, bi, bj):
        a.setflags(write=False)
    return A, b, bi, bj


@functools.lru_cache(maxsize=None)
def numpy_solve(n_pose, w, cyclic):
    A, b, _, _ = system(n_pose, w, cyclic)
    return np.linalg.solve(A, b)


def _args(A, b, x, n_pose, bi, bj, K, reps, ms, ku):
    return (A.ctypes.data, b.ctypes.data, x.ctypes.data, n_pose, bi.ctypes.data, bj.ctypes.data, bi.size, K, reps,
            ctypes.byref(ms), ctypes.byref(ku))


def nd_solve(A, b, n_pose, bi, bj, K):
    """orbhip_test_nd_solve: (rc, x, K used); x starts as ones, so a zeroed x was written."""
    from orb_slam3_ros2_amd._lib import lib
    f = lib().orbhip_test_nd_solve
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p] * 2
    A = np.ascontiguousarray(A)
    x = np.ones(A.shape[0])
    ms, ku = ctypes.c_float(0), ctypes.c_int(0)
    rc = f(*_args(A, b, x, n_pose, bi, bj, K, 1, ms, ku))
    return rc, x, ku.value


def nd_stages(A, b, n_pose, bi, bj, K):
    """orbhip_test_nd_stages: a whole solve, each half alone, a whole solve again; (rc, x, K used,
    segment starts, w)."""
    from orb_slam3_ros2_amd._lib import lib
    f = lib().orbhip_test_nd_stages
    f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] + [ctypes.c_void_p] * 2 + [ctypes.c_int] * 3 + \
        [ctypes.c_void_p] * 4
    A = np.ascontiguousarray(A)
    x = np.ones(A.shape[0])
    ms, ku = ctypes.c_float(0), ctypes.c_int(0)
    stage = (ctypes.c_float * 2)()
    seg = (ctypes.c_int * 65)()
    rc = f(*_args(A, b, x, n_pose, bi, bj, K, 1, ms, ku), stage, seg)
    k = ku.value
    return rc, x, k, list(seg[:k + 1]), seg[k + 1]


def figures_on_blocks(p, bi, bj):
    """The model's per-segment figures under the system's own pose blocks."""
    return M.segment_figures(p, M.block_adjacency(p.n_pose, bi, bj))


def check_plan_and_paths(case, bi, bj, ku, seg, w):
    """The device planned what the model plans, and the system's own envelope (inside the full
    band's: a corner tile of it may hold no block) reaches the paths the full band's does
    (tests/test_nd_model.py pins those): registers only, or the in-step loads too."""
    K = case[3]
    p = M.plan(*case)
    assert p.ok and ku == K and seg == p.seg and w == p.w
    fig, full = figures_on_blocks(p, bi, bj), M.segment_figures(p)
    print("ND", case, "per segment (interior poses, nti, NT, phase 1, phase 2, padding):", fig)
    for f, g in zip(fig, full):
        assert (f[:3], f[5]) == (g[:3], g[5]), (fig, full)
        for ph in (3, 4):
            assert f[ph] <= g[ph] and min(f[ph], M.REG_TILES + 1) == min(g[ph], M.REG_TILES + 1), (fig, full)


@pytest.mark.parametrize("case", SOLVES)
def test_nd_wide_band_solve(case):
    n_pose, w, cyclic, K = case
    A, b, bi, bj = system(n_pose, w, cyclic)
    rc, x, ku = nd_solve(A, b, n_pose, bi, bj, K)
    assert rc == 0 and ku == K, (rc, ku)
    rc2, x2, ku2, seg, w_dev = nd_stages(A, b, n_pose, bi, bj, K)
    assert rc2 == 0, rc2
    check_plan_and_paths(case, bi, bj, ku2, seg, w_dev)
    ref = numpy_solve(n_pose, w, cyclic)
    for y in (x, x2):
        err = np.abs(y - ref).max() / np.abs(ref).max()
        print("ND", case, "forward error against numpy", err)
        check_solve(A, y, b)
        assert err < 1e-9, err


def test_nd_lds_ceiling_solve():
    """664 poses, w = 114, K = 2: segments of 84 tiles, 130 640 bytes of dynamic LDS, the most
    k_nd_backsolve takes; phase 1 meets 11 tiles per wave and column, phase 2 6. It is also the
    automatic plan (K = 0): one solve by each. n = 3984: the backward error only."""
    n_pose, w, cyclic, K = CEILING
    A, b, bi, bj = system(n_pose, w, cyclic, CEILING_LAND)
    assert M.bs_lds_bytes(M.plan(*CEILING).max_NT) == 130640
    rc, x, ku, seg, w_dev = nd_stages(A, b, n_pose, bi, bj, K)
    assert rc == 0, rc
    check_plan_and_paths(CEILING, bi, bj, ku, seg, w_dev)
    check_solve(A, x, b)
    rc, x0, ku = nd_solve(A, b, n_pose, bi, bj, 0)
    assert rc == 0 and ku == M.automatic_plan(n_pose, w, cyclic).K == 2, (rc, ku)
    check_solve(A, x0, b)


@pytest.mark.parametrize("levels", ["1", "2"])
def test_nd_second_level_on_a_wide_band(levels, monkeypatch):
    """576 poses, w = 48, K = 6: six separators of 288 rows. ORBHIP_ND_LEVELS=2 dissects the
    separator system once more (three inner segments: interior 9 tiles, 27 tiles in all, phase 2
    on both register slots), 1 solves it densely (n = 1728). The stages hook's last whole solve,
    after the two halves ran alone on the same workspace, leaves the x of the plain solve: two
    solutions of backward error <= ETA_CAP u lie within about 2 cond ETA_CAP u of each other (6e-12
    here), while anything the half-runs left behind in the flags or buffers would show at the size
    of x itself."""
    case = (576, 48, True, 6)
    n_pose, w, cyclic, K = case
    monkeypatch.setenv("ORBHIP_ND_LEVELS", levels)
    assert M.second_level(M.plan(*case)) is not None
    A, b, bi, bj = system(n_pose, w, cyclic)
    rc, x, ku = nd_solve(A, b, n_pose, bi, bj, K)
    assert rc == 0 and ku == K, (rc, ku)
    rc, xs, ku, seg, w_dev = nd_stages(A, b, n_pose, bi, bj, K)
    assert rc == 0 and ku == K and seg == M.plan(*case).seg and w_dev == w, (rc, ku, seg, w_dev)
    ref = numpy_solve(n_pose, w, cyclic)
    for y in (x, xs):
        check_solve(A, y, b)
        assert np.abs(y - ref).max() / np.abs(ref).max() < 1e-9
    diff = np.abs(x - xs).max() / np.abs(x).max()
    print("ND levels", levels, "stages against plain solve", diff)
    assert diff <= 2 * COND_MAX * ETA_CAP * U, diff


@pytest.mark.parametrize("case,K", [((191, 48, True), 2), ((666, 114, True), 2), ((666, 114, True), 0)])
def test_nd_refused_plans(case, K):
    """191 / 48 / K = 2: interiors of 47 and 48 poses, one narrower than the band. 666 / 114: K = 2
    needs 85 tiles per segment and no other K leaves interiors of w poses, so neither the forced
    nor the automatic plan is made. The answer comes from the plan alone (the pose blocks): the
    matrix is never read, so a zero one stands in for it."""
    n_pose, w, cyclic = case
    assert not M.plan(n_pose, w, cyclic, 2).ok and M.automatic_plan(n_pose, w, cyclic) is None
    bi, bj = np.nonzero(np.triu(np.ones((n_pose, n_pose), bool)))
    d = bj - bi
    keep = np.minimum(d, n_pose - d) <= w
    bi, bj = bi[keep].astype(np.int32), bj[keep].astype(np.int32)
    assert M.band_of(n_pose, bi, bj) == (w, cyclic)
    A = np.zeros((6 * n_pose, 6 * n_pose))
    rc, x, _ = nd_solve(A, np.zeros(6 * n_pose), n_pose, bi, bj, K)
    assert rc == UNSUPPORTED, rc
    assert np.all(x == 1.0)   # untouched


def _bad_rows(case, levels):
    """S rows whose diagonal is made negative, by name."""
    p = M.plan(*case)
    last = p.segments[-1]
    rows = {"interior": 6 * ((last.interior[0] + last.interior[1]) // 2) + 3,
            "separator": 6 * p.separator_poses(0)[0] + 6 * (p.w // 2) + 1}
    if p.K >= 6:   # separator 0 above is an even one: an inner interior at level 2; an odd one: an inner separator
        assert (M.second_level(p) is not None) and levels in ("1", "2")
        rows["odd separator"] = 6 * p.separator_poses(1)[0] + 6 * (p.w // 3) + 5
        rows["last separator"] = 6 * p.separator_poses(p.K - 1)[1] - 1
    return rows


@pytest.mark.parametrize("levels", ["1", "2"])
@pytest.mark.parametrize("case", [(203, 48, True, 2), (576, 48, True, 6)])
def test_nd_not_positive_definite_rejected(case, levels, monkeypatch):
    """One negative diagonal entry, in turn in an interior row of the last segment and in rows of
    separators (K = 6 at level 2: an even separator is an interior of the separator system's own
    dissection, an odd one a separator of it): rc = -4 (flag 0) and x = 0, then the unchanged
    system solves in the same process to the backward bound. A handled rejection, not a fault.

    How the solve ends in that state, read in ba_chol_dag.hip and ba_nd.hip: a non-positive pivot
    stops nothing. diag16 / diag32 replace it by 1 and clear the chain's `ok` word only, so the
    values stay finite, the chain of k_chol_dag_multi runs every interval of its segment and
    publishes every flag whatever the values, the helpers run every task (their waits look at
    flags, never at values) and the partial solve ends by writing flag[0] = ok. Every wait is
    bounded besides (ORBHIP_DAG_SPIN_MAX polls, then the abort word ends all others: that would
    be rc = -7 here, not -4). The other segments of the launch share nothing with the failed one.
    k_nd_assemble then sums finite wrong contributions, the separator solve runs on them like on
    any matrix, and k_nd_backsolve reads every segment's flag and the separator system's before it
    writes: any zero gives x = 0 and flag = 0. At level 2 the inner dissection's k_nd_backsolve
    writes the separator system's flag by the same rule. Nothing had to change."""
    n_pose, w, cyclic, K = case
    monkeypatch.setenv("ORBHIP_ND_LEVELS", levels)
    A, b, bi, bj = system(n_pose, w, cyclic)
    for name, row in _bad_rows(case, levels).items():
        B = A.copy()
        B[row, row] = -1e3
        rc, x, _ = nd_solve(B, b, n_pose, bi, bj, K)
        assert rc == NOT_SPD, (name, row, rc)
        assert not x.any(), (name, row)
        rc, x, ku = nd_solve(A, b, n_pose, bi, bj, K)
        assert rc == 0 and ku == K, (name, rc, ku)
        check_solve(A, x, b)


def test_gba_wide_band_dissected(monkeypatch):
    """A 200-keyframe loop with a 49-keyframe co-visibility window as a GlobalBundleAdjustment: 199
    optimised poses, w = 48, forced to K = 2 (interiors of 51 and 52 poses; phase 2 of the
    back-substitution meets 3 tiles per wave and column, phase 1 5). Equal to the plain DAG solve
    (same LM schedule, chi2 to 1e-9); two persistent solves per trial show the dissection ran."""
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem
    prob, _ = synthetic_ba_problem(n_kf=200, n_pts=6000, layout="loop", window=49, seed=23)
    # the optimised poses' blocks (keyframe 0 is fixed: pose = keyframe - 1), as the solver forms them
    kfs = {}
    for k, m in zip(prob.edge_pose.tolist(), prob.edge_point.tolist()):
        if k > 0:
            kfs.setdefault(m, []).append(k - 1)
    blocks = {(min(a, c), max(a, c)) for v in kfs.values() for a in v for c in v}
    bi, bj = [e[0] for e in blocks], [e[1] for e in blocks]
    w, cyclic = M.band_of(199, bi, bj)
    assert cyclic and 43 <= w <= 48, w
    p = M.plan(199, w, True, 2)
    fig = figures_on_blocks(p, bi, bj)
    print("ND GBA w", w, fig)
    assert p.ok and min(f[3] for f in fig) >= 3 and min(f[4] for f in fig) >= 3, fig
    monkeypatch.setenv("ORBHIP_ND_MIN", "0")
    res = {}
    for nd in ("1", "0"):
        monkeypatch.setenv("ORBHIP_ND", nd)
        if nd == "1":
            monkeypatch.setenv("ORBHIP_ND_K", "2")
        else:
            monkeypatch.delenv("ORBHIP_ND_K")
        opt = Optimizer()
        l0 = opt.stats()["dag_launches"]
        g = opt.BundleAdjustment(prob, nIterations=3, bRobust=True)
        per = (opt.stats()["dag_launches"] - l0) / g.lm_trials
        assert per >= 2 if nd == "1" else per < 2, (nd, per)
        res[nd] = g
    g, r = res["1"], res["0"]
    assert g.lm_trials == r.lm_trials and g.final_chi2 < g.initial_chi2
    assert abs(g.final_chi2 - r.final_chi2) <= 1e-9 * abs(r.final_chi2)
