"""Optimizer::OptimizeSim3 on the device (orbhip_optimize_sim3 / _batch, k_sim3_opt) against the float64
restatement tests/sim3_opt_numpy.py: n_in, n_bad and keep by equality, the rotation by
1 - |q.q'| < tol^2, t by tol max(1, |t|inf), s relative by tol, tol = 1e-4 (the project's Optimizer
tolerance). Every problem is one of sim3_opt_cases.py, which test_sim3_opt.py shows to be independent
of the edge order on the CPU. Outputs of the error cases are pre-filled with a poison value."""
import ctypes

import numpy as np
import pytest

import sim3_opt_cases as C
from orb_slam3_ros2_amd import Optimizer, Sim3Problem, Sim3Result  # noqa: F401
from orb_slam3_ros2_amd._lib import Context, Sim3OptProblemC, Sim3OptResultC, lib, ptr

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -5
TOL = 1e-4
WAVES = ["1", "4"]                       # every group width of k_sim3_opt (ORBHIP_SIM3_OPT_WAVES)
MAX_B, MAX_N = 64, 8192                  # the envelope of orbhip_optimize_sim3_batch


@pytest.fixture(scope="module")
def opt():
    return Optimizer(ctx=Context())


def _qdist(a, b):
    return 1.0 - abs(float(np.dot(a / np.linalg.norm(a), b / np.linalg.norm(b))))


def _check(g, o, tol=TOL):
    assert g.n_in == o["n_in"] and g.n_bad == o["n_bad"]
    assert np.array_equal(g.keep, o["keep"])
    assert _qdist(g.q, o["q"]) < tol * tol
    assert np.abs(g.t - o["t"]).max() <= tol * max(1.0, float(np.abs(o["t"]).max()))
    assert abs(g.s - o["s"]) <= tol * o["s"]


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("n", C.SIZE_N)
def test_size_edges(opt, monkeypatch, waves, n):
    monkeypatch.setenv("ORBHIP_SIM3_OPT_WAVES", waves)
    _check(opt.OptimizeSim3(C.case(f"size{n}")), C.reference(f"size{n}"))


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("n", C.BOUNDARY_N + [1000])
def test_register_cache_boundaries(opt, monkeypatch, waves, n):
    """One below, at and one above EC x 64 W pairs (W = 1: 256, W = 4: 1024), in both widths, and n = 1000."""
    assert C.BOUNDARY_N == [C.CAP_W1 - 1, C.CAP_W1, C.CAP_W1 + 1, C.CAP_W4 - 1, C.CAP_W4, C.CAP_W4 + 1]
    monkeypatch.setenv("ORBHIP_SIM3_OPT_WAVES", waves)
    name = "large1000" if n == 1000 else f"boundary{n}"
    g = opt.OptimizeSim3(C.case(name))
    _check(g, C.reference(name))
    assert g.n_bad > 0 and g.n_in > n // 2


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("B", C.BATCH_B)
def test_batch_edges(opt, monkeypatch, waves, B):
    """A different n, camera pair, scale mode and outlier share per problem."""
    monkeypatch.setenv("ORBHIP_SIM3_OPT_WAVES", waves)
    names = [f"batch{i}" for i in range(B)]
    rs = opt.OptimizeSim3_batch([C.case(k) for k in names])
    assert len(rs) == B
    for k, r in zip(names, rs):
        _check(r, C.reference(k))
        if C.case(k).fix_scale:
            assert r.s == C.case(k).s      # bit-identical


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("name", ["left9", "left10", "allbad", "stale", "behind", "fixed200"])
def test_cpu_scenes(opt, monkeypatch, waves, name):
    monkeypatch.setenv("ORBHIP_SIM3_OPT_WAVES", waves)
    p, o = C.case(name), C.reference(name)
    g = opt.OptimizeSim3(p)
    _check(g, o)
    if name in ("left9", "allbad"):        # return 0: g2oS12 untouched, bit for bit
        assert g.n_in == 0 and np.array_equal(g.q, p.q) and np.array_equal(g.t, p.t) and g.s == p.s
    if name == "left10":
        assert g.n_in == 10
    if name == "behind":
        assert not g.keep[:5].any() and np.isfinite(g.t).all()
    if name == "stale":
        assert o["round1_last_rejected"]


def test_default_width_needs_no_switch(opt, monkeypatch):
    monkeypatch.delenv("ORBHIP_SIM3_OPT_WAVES", raising=False)
    _check(opt.OptimizeSim3(C.case("fixed200")), C.reference("fixed200"))


def _raw(ctx, probs, keep=True, single=False):
    ps = [p.normalized() for p in probs]
    cprobs = (Sim3OptProblemC * len(ps))(*[p.to_c() for p in ps])
    cres = (Sim3OptResultC * len(ps))()
    keeps = [np.full(p.X1c.shape[0], 0xAB, np.uint8) for p in ps]
    for i, k in enumerate(keeps):
        cres[i].keep = ptr(k) if keep else None
    if single:
        rc = lib().orbhip_optimize_sim3(ctx.handle, cprobs, cres)
    else:
        rc = lib().orbhip_optimize_sim3_batch(ctx.handle, cprobs, len(ps), cres)
    return rc, cres, keeps, ps


def _bytes(cres, keeps):
    return b"".join(bytes(memoryview(r))[:ctypes.sizeof(Sim3OptResultC) - 8] for r in cres) + b"".join(k.tobytes() for k in keeps)


def test_keep_may_be_null_and_calls_repeat_bit_for_bit(opt):
    probs = [C.case("batch0"), C.case("batch2"), C.case("size65")]
    rc, cres, keeps, _ = _raw(opt.ctx, probs)
    assert rc == 0
    rc2, cres2, keeps2, _ = _raw(opt.ctx, probs)
    assert rc2 == 0 and _bytes(cres, keeps) == _bytes(cres2, keeps2)
    rc3, cres3, keeps3, _ = _raw(opt.ctx, probs, keep=False)
    assert rc3 == 0 and all((k == 0xAB).all() for k in keeps3)
    assert _bytes(cres3, []) == _bytes(cres, [])
    # the one-problem call returns n_in
    rc4, cres4, _, _ = _raw(opt.ctx, probs[:1], single=True)
    assert rc4 == cres4[0].n_in == C.reference("batch0")["n_in"]
    assert lib().orbhip_optimize_sim3_batch(opt.ctx.handle, None, 0, None) == 0


def test_workspace_regrowth():
    o = Optimizer(ctx=Context())           # a fresh context: the block starts empty
    for k in ("regrow0", "regrow1", "regrow2"):
        _check(o.OptimizeSim3(C.case(k)), C.reference(k))


def test_profile_stage_brackets_the_launch(opt):
    L = lib()
    assert L.orbhip_profile_stage(opt.ctx.handle, 13) == 0
    for _ in range(3):
        opt.OptimizeSim3(C.case("size65"))
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(opt.ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(opt.ctx.handle, 0) == 0
    assert cnt.value == 3 and 0.0 < ms.value < 1000.0
    assert L.orbhip_profile_stage(opt.ctx.handle, 14) == ERR_ARG


# ---- argument errors ----
def _poisoned(n):
    r = Sim3OptResultC()
    ctypes.memset(ctypes.byref(r), 0xCD, ctypes.sizeof(r))
    keep = np.full(n, 0xCD, np.uint8)
    r.keep = ptr(keep)
    return r, keep


def _untouched(r, keep):
    raw = bytes(memoryview(r))[:ctypes.sizeof(Sim3OptResultC) - 8]
    return raw == b"\xcd" * len(raw) and (keep == 0xCD).all()


def test_argument_errors_leave_the_outputs_untouched(opt):
    L, h = lib(), opt.ctx.handle
    base = C.case("size65").normalized()
    nan, inf = float("nan"), float("inf")

    def with_(**kw):
        c = base.to_c()
        for k, v in kw.items():
            if k in ("cam1", "cam2", "q", "t"):
                i, x = v
                getattr(c, k)[i] = x
            else:
                setattr(c, k, v)
        return c

    cases = [(ERR_ARG, with_(**{k: None})) for k in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")]
    cases += [(ERR_ARG, with_(n=-1))]
    cases += [(ERR_ARG, with_(**{cam: (i, v)})) for cam in ("cam1", "cam2") for i in (0, 1) for v in (0.0, -500.0, nan, inf)]
    cases += [(ERR_ARG, with_(th2=v)) for v in (0.0, -10.0, nan, inf)]
    cases += [(ERR_ARG, with_(s=v)) for v in (0.0, -1.0, nan, inf)]
    cases += [(ERR_ARG, with_(q=(i, v))) for i in range(4) for v in (nan, inf)]
    cases += [(ERR_ARG, with_(t=(i, v))) for i in range(3) for v in (nan, -inf)]
    cases += [(ERR_UNSUPPORTED, with_(n=MAX_N + 1))]     # refused before any array is read
    for want, c in cases:
        r, keep = _poisoned(65)
        assert L.orbhip_optimize_sim3(h, ctypes.byref(c), ctypes.byref(r)) == want
        assert _untouched(r, keep)
        # as the second problem of a batch: the first one's outputs stay untouched too
        cp = (Sim3OptProblemC * 2)(base.to_c(), c)
        cr = (Sim3OptResultC * 2)()
        ctypes.memset(cr, 0xCD, ctypes.sizeof(cr))
        k0, k1 = np.full(65, 0xCD, np.uint8), np.full(65, 0xCD, np.uint8)
        cr[0].keep, cr[1].keep = ptr(k0), ptr(k1)
        assert L.orbhip_optimize_sim3_batch(h, cp, 2, cr) == want
        assert _untouched(cr[0], k0) and _untouched(cr[1], k1)
    # a NULL pointer is no error without correspondences: S12 is copied through
    c = with_(n=0, X1c=None, X2c=None, obs1=None, obs2=None, inv_sigma2_1=None, inv_sigma2_2=None)
    r, keep = _poisoned(65)
    assert L.orbhip_optimize_sim3(h, ctypes.byref(c), ctypes.byref(r)) == 0
    assert r.n_in == 0 and r.n_bad == 0 and r.lm_trials == 0 and (keep == 0xCD).all()
    assert list(r.q) == list(base.q) and list(r.t) == list(base.t) and r.s == base.s
    # the envelope: B = 65, and B = 64 passes; NULL arrays; a negative count
    many = (Sim3OptProblemC * (MAX_B + 1))(*[base.to_c()] * (MAX_B + 1))
    mres = (Sim3OptResultC * (MAX_B + 1))()
    ctypes.memset(mres, 0xCD, ctypes.sizeof(mres))
    for i in range(MAX_B + 1):
        mres[i].keep = None
    assert L.orbhip_optimize_sim3_batch(h, many, MAX_B + 1, mres) == ERR_UNSUPPORTED
    assert all(_untouched(mres[i], np.full(1, 0xCD, np.uint8)) for i in range(MAX_B + 1))
    assert L.orbhip_optimize_sim3_batch(h, many, MAX_B, mres) == 0
    assert L.orbhip_optimize_sim3_batch(h, None, 1, mres) == ERR_ARG
    assert L.orbhip_optimize_sim3_batch(h, many, 1, None) == ERR_ARG
    assert L.orbhip_optimize_sim3_batch(h, many, -1, mres) == ERR_ARG
    assert L.orbhip_optimize_sim3(h, None, None) == ERR_ARG
    assert L.orbhip_optimize_sim3_batch(None, many, 1, mres) == ERR_ARG


def test_largest_problem_of_the_envelope(opt):
    """n = 8192 is accepted and runs."""
    g = opt.OptimizeSim3(C.case("max8192"))
    _check(g, C.reference("max8192"))
    assert g.n_in > 8000
