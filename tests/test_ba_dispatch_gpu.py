"""GPU: every row of the BA Cholesky dispatch (ba_solve_batch, DESIGN.md "BA Cholesky dispatch")
reached from the LM and compared with the oracle, and the LDS panel solver (k_ba_cholesky /
chol_solve) on its own.

The solver yardstick (tests/helpers.py::check_solve, also applied to the register, DAG and blocked
solver tests of test_ba_gpu.py), with u = 2^-53:
    backward error  eta = |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf)  <= 8 u
    forward error   max|x - x_ld| / max|x_ld|                          <= 8 cond u   (x_ld: long double)
The caps come from references, not from the kernels. On spd_with_spectrum's family (n up to 1201,
cond up to 1e12) fp64 LAPACK stays below 0.37 u / 0.42 cond u and an fp64 numpy model of this
project's panel algorithm (explicit inverses of the 32x32 diagonal factors) below 0.82 u /
0.46 cond u. On band_spd's family (cond = its bound 5, helpers.BAND_COND) LAPACK's Cholesky has up
to 2.1 u (n = 2394, loop) / 1.3 cond u and the model 3.3 u / 1.4 cond u.

Measured on the MI355X, worst case per solver over the cases of this module and of
test_ba_gpu.py's solver tests (eta / u, forward / (cond u); where it occurred):
    register   0.41 (n = 6, cond 1e8)            0.39 (n = 294, cond 1e2)
    LDS        0.91 (n = 1), 0.66 (n = 479)      0.74 (n = 479, cond 1e2)
    DAG        0.25 on the 8-decade spectra      0.16
               5.4  (n = 2394, loop)             5.0  (n = 96, dense, 1 helper)
    blocked    0.07 on the 8-decade spectrum     0.05
               2.4  (n = 2394, loop)             1.3  (n = 600, dense)
Before the updates' products were summed from zero ("Update accumulation") the DAG
solver had 8.3 u and the blocked solver 9.0 u at n = 2394, loop: over the cap.

LM parity: every problem is synthetic_ba_problem with keyframe 0 fixed, compared with
oracle.ba_solve (never with another GPU path): schedule, chi2, poses and points to 1e-4."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem
from tests.helpers import check_solve, compare_ba, spd_with_spectrum

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_NOT_PD = -1, -4
PERTURBED = dict(rot_noise=0.1, trans_noise=0.2, pt_noise=0.5)
# id: (n_kf, n_pts, seed, extra arguments); n = 6 (n_kf - 1)
CASES = {"A0": (60, 600, 51, {}), "A1": (75, 800, 112, PERTURBED), "A2": (8, 100, 75, {}), "A3": (81, 800, 72, {}),
         "B0": (90, 900, 74, {}), "B1": (52, 500, 71, {}), "B2": (20, 300, 76, {}), "D0": (70, 700, 78, {}),
         "E0": (20, 300, 79, {}), "E1": (60, 600, 118, PERTURBED), "E2": (90, 900, 81, {}), "F0": (50, 500, 82, {})}


def make_case(key, iterations=10):
    n_kf, n_pts, seed, kw = CASES[key]
    prob, _ = synthetic_ba_problem(n_kf=n_kf, n_pts=n_pts, seed=seed, **kw)
    assert prob.pose_fixed.sum() == 1 and prob.pose_fixed[0] == 1
    prob.iterations = iterations
    return prob


def make_e3():
    """E3: a 100-KF loop with a 20-KF window (n = 594: a band envelope with a loop-closure corner),
    as BundleAdjustment(nIterations=10, bRobust=True) poses it."""
    from orb_slam3_ros2_amd.optimizer import BAProblem
    prob, _ = synthetic_ba_problem(n_kf=100, n_pts=1000, seed=83, layout="loop", window=20)
    return prob, BAProblem(**{**prob.__dict__, "iterations": 10, "huber_delta": float(np.sqrt(5.99))})


def n_of(prob):
    return 6 * int((np.asarray(prob.pose_fixed) == 0).sum())


@pytest.fixture(scope="module")
def opt():
    from orb_slam3_ros2_amd import Optimizer
    return Optimizer()


@pytest.fixture(scope="module")
def solved(oracle):
    """(problem, oracle solve) per case id and budget, solved once per module."""
    cache = {}

    def get(key, iterations=10):
        if (key, iterations) not in cache:
            p = make_case(key, iterations)
            cache[key, iterations] = (p, oracle.ba_solve(p))
        return cache[key, iterations]
    return get


# ---------------------------------------------------------------------------------------------
# the LDS panel solver on its own (orbhip_test_cholesky)
# ---------------------------------------------------------------------------------------------
def _lds_solve(A, b, x):
    from orb_slam3_ros2_amd._lib import lib
    ph = np.zeros(8, np.uint64)
    ms = ctypes.c_float(0)
    A = np.ascontiguousarray(A)
    return lib().orbhip_test_cholesky(A.ctypes.data, b.ctypes.data, x.ctypes.data, A.shape[0], ph.ctypes.data,
                                      ctypes.byref(ms))


@pytest.mark.parametrize("cond", [1e2, 1e8])
@pytest.mark.parametrize("n", [1, 6, 31, 32, 33, 63, 64, 65, 306, 330, 450, 479, 480])
def test_lds_cholesky_solves_spd(n, cond):
    """One partial panel (1, 6, 31), one exact panel (32), a last panel of 1 / 31 columns (33, 65 /
    63, 479), 16-row block padding past the last row (nr_pad > nr), the production sizes 306..480
    and the LDS capacity limit (480); eigenvalues over 2 and over 8 decades."""
    rng = np.random.default_rng(1000 + n)
    A = spd_with_spectrum(n, cond, rng)
    b = rng.normal(size=n)
    x = np.zeros(n)
    assert _lds_solve(A, b, x) == 0
    check_solve(A, x, b, cond)


def test_lds_cholesky_rejects_bad_arguments():
    from orb_slam3_ros2_amd._lib import lib
    rng = np.random.default_rng(481)
    A = spd_with_spectrum(481, 1e2, rng)
    b = rng.normal(size=481)
    x = np.zeros(481)
    assert _lds_solve(A, b, x) == ERR_ARG        # past the LDS envelope
    ms = ctypes.c_float(0)
    ph = np.zeros(8, np.uint64)
    A6, b6, x6 = np.eye(6), np.ones(6), np.zeros(6)
    L = lib()
    assert L.orbhip_test_cholesky(A6.ctypes.data, b6.ctypes.data, x6.ctypes.data, 6, None, ctypes.byref(ms)) == ERR_ARG
    assert L.orbhip_test_cholesky(A6.ctypes.data, b6.ctypes.data, x6.ctypes.data, 6, ph.ctypes.data, None) == ERR_ARG


@pytest.mark.parametrize("j,value", [(0, -1e6), (40, -1e6), (329, -1e6), (40, float("nan"))])
def test_lds_cholesky_non_spd_rejected(j, value):
    """Not positive definite at n = 330: a bad pivot in the first panel, in the second panel and in
    the last column, and a NaN pivot: ORBHIP_ERR_NOT_PD and x = 0 (the kernel leaves its panel loop
    with a break; it has no spin-wait)."""
    n = 330
    rng = np.random.default_rng(330)
    A = spd_with_spectrum(n, 1e2, rng)
    A[j, j] = value
    b = rng.normal(size=n)
    x = np.ones(n)
    assert _lds_solve(A, b, x) == ERR_NOT_PD
    assert not x.any()


# ---------------------------------------------------------------------------------------------
# LM parity through the dispatch rows
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fused", ["0", "1"])
def test_batch_lds_solver_parity(opt, solved, monkeypatch, fused):
    """A batch whose largest small problem has n = 480 > 304: all four problems, the 42-column one
    (a single partial panel) included, go through k_ba_cholesky. It factors S in place, so every
    trial zeroes S (k_ba_zero_s) and rebuilds the Schur complement: A1's rejected trials prove the
    rebuild after a rejection."""
    monkeypatch.setenv("ORBHIP_BA_FUSED", fused)
    keys = ["A0", "A1", "A2", "A3"]
    cases = [solved(k) for k in keys]
    for k in ("A0", "A1", "A3"):
        assert 304 < n_of(solved(k)[0]) <= 480
    assert n_of(solved("A2")[0]) == 42
    o1 = solved("A1")[1]
    assert o1["lm_trials"] > o1["iterations_done"]   # the oracle rejects trials on A1
    l0 = opt.stats()["dag_launches"]
    res = opt.solve_batch([p for p, _ in cases])
    assert opt.stats()["dag_launches"] == l0         # no problem of the batch took the DAG solver
    for k, (p, o), g in zip(keys, cases, res):
        print("case", k)
        compare_ba(g, o, p)


@pytest.mark.parametrize("big_budget", [10, 2])
def test_batch_with_one_dag_problem(opt, solved, big_budget):
    """A 534-column problem inside a batch: one k_chol_dag launch per trial for it, gated on its own
    phase word, while the 306- and 114-column problems share the LDS solver's launch. With a budget
    of 10 the large problem finishes last (the others run 3 and 10 iterations), with 2 first."""
    cases = [solved("B0", big_budget), solved("B1", 3), solved("B2")]
    assert n_of(cases[0][0]) == 534 and n_of(cases[1][0]) == 306 and n_of(cases[2][0]) == 114
    l0 = opt.stats()["dag_launches"]
    res = opt.solve_batch([p for p, _ in cases])
    assert opt.stats()["dag_launches"] - l0 >= cases[0][1]["lm_trials"]
    for k, (p, o), g in zip(("B0", "B1", "B2"), cases, res):
        print("case", k)
        compare_ba(g, o, p)


@pytest.mark.parametrize("nshards", [2, 3])
def test_local_shards_lds_solver(opt, solved, nshards):
    """Landmark shards of a 70-KF problem summed on the device: every shard factors the summed S
    (n = 414) with the LDS solver, in place, so every trial re-sums it."""
    from orb_slam3_ros2_amd.sharding import merge_results, shard_bounds, shard_problem
    p, o = solved("D0")
    assert n_of(p) == 414
    parts = [shard_problem(p, r, nshards) for r in range(nshards)]
    l0 = opt.stats()["dag_launches"]
    res = opt.solve_shards_local([q[0] for q in parts])
    assert opt.stats()["dag_launches"] == l0
    for r in res[1:]:   # replicated poses agree bit for bit
        assert np.array_equal(r.pose_t, res[0].pose_t) and np.array_equal(r.pose_q, res[0].pose_q)
    compare_ba(merge_results(p, res, shard_bounds(p, nshards), [q[3] for q in parts]), o, p)


def _run_child(code, env_name):
    """One fresh child process with a switch that the library reads once per process."""
    r = subprocess.run([sys.executable, "-c", code, ROOT], env={**os.environ, env_name: "1"}, timeout=120,
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stderr[-4000:]


_CHILD_HEAD = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from oracle import pyoracle as oracle
from orb_slam3_ros2_amd import Optimizer
from tests.helpers import BAND_COND, band_spd, check_solve, compare_ba
from tests.test_ba_dispatch_gpu import make_case, make_e3, n_of
"""

_CHILD_BLOCKED = _CHILD_HEAD + r"""
opt = Optimizer()
for key, n in (("E0", 114), ("E1", 354), ("E2", 534)):   # register, lone LDS, blocked (dense)
    p = make_case(key)
    assert n_of(p) == n
    o = oracle.ba_solve(p)
    if key == "E1":
        assert o["lm_trials"] > o["iterations_done"]   # the in-place factor is rebuilt after a rejection
    print("case", key)
    compare_ba(opt.solve(p), o, p)
prob, p = make_e3()                                      # blocked, band envelope + loop corner
assert n_of(p) == 594
o = oracle.ba_solve(p)
g = opt.BundleAdjustment(prob, nIterations=10, bRobust=True)
print("case E3")
compare_ba(g, o, p)
assert g.final_chi2 < 0.2 * g.initial_chi2
assert opt.stats()["dag_launches"] == 0, opt.stats()
"""

_CHILD_TAIL = _CHILD_HEAD + r"""
from orb_slam3_ros2_amd._lib import lib
L = lib()
def hook(n, shape):
    rng = np.random.default_rng(n)
    A = band_spd(n, shape, rng)
    b = rng.normal(size=n)
    x = np.zeros(n)
    ms = ctypes.c_float(0)
    rc = L.orbhip_test_cholesky_dag(A.ctypes.data, b.ctypes.data, x.ctypes.data, n, 3, 0, ctypes.byref(ms), None)
    assert rc == 0, rc
    check_solve(A, x, b, BAND_COND)
p = make_case("F0")
assert n_of(p) == 294
o = oracle.ba_solve(p)
# the hook solves on the null stream, the two contexts on their own: every change of stream is a
# hand-off, which this form makes behind an event at the previous stream's tail
a, b = Optimizer(), Optimizer()
h0 = a.stats()["dag_handoffs"]
hook(294, "dense")
compare_ba(a.LocalBundleAdjustment(p), o, p)
hook(600, "band")
compare_ba(b.LocalBundleAdjustment(p), o, p)
compare_ba(a.LocalBundleAdjustment(p), o, p)
s = a.stats()
assert s["dag_handoffs"] - h0 >= 4 and s["dag_timeouts"] == 0 and b.stats()["dag_timeouts"] == 0, s
"""


def test_forced_blocked_solver_paths():
    """ORBHIP_CHOL_BLOCKED (read once per process, hence a fresh child): a lone problem takes the
    register solver up to n = 304 (E0), the LDS solver up to 480 (E1, with rejected trials) and
    the one-launch-per-panel blocked solver above, on a dense S (E2) and on a band envelope with a
    loop-closure corner (E3: cb_envelope_tiles); no k_chol_dag launch in the whole process."""
    _run_child(_CHILD_BLOCKED, "ORBHIP_CHOL_BLOCKED")


def test_dag_handoff_tail_form():
    """ORBHIP_DAG_HANDOFF_TAIL (read once per process): the hand-off between streams waits for the
    previous stream's tail. The DAG solver's hook at n = 294 dense and n = 600 band (3 repetitions,
    the solver yardstick) and F0's LBA on two contexts, each against the oracle."""
    _run_child(_CHILD_TAIL, "ORBHIP_DAG_HANDOFF_TAIL")


def test_rccl_full_s_allreduce(oracle, monkeypatch):
    """ORBHIP_SHARD_FULL_S (read per call): a sharded solve of n = 594 all-reduces the full S
    instead of its packed union envelope. One RCCL rank, against the oracle."""
    from orb_slam3_ros2_amd import Optimizer
    monkeypatch.setenv("ORBHIP_SHARD_FULL_S", "1")
    _, p = make_e3()
    assert n_of(p) == 594
    o = oracle.ba_solve(p)
    opt = Optimizer()
    opt.comm_init(1, 0, Optimizer.comm_unique_id())
    compare_ba(opt.solve_sharded(p), o, p)
