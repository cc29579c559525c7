"""orbhip_sim3_solve_batch on the GPU against the numpy restatement (tests/sim3_solver_numpy.py):
every output must be EQUAL, for every hypothesis and every correspondence, with no tolerance (a NaN
matches a NaN at the same place). Outputs are pre-filled with a poison value."""
import ctypes
import itertools

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import Context, Sim3ProblemC, Sim3ResultC, lib, ptr
from orb_slam3_ros2_amd.sim3solver import Sim3Solver
from orb_slam3_ros2_amd.synthetic import synthetic_sim3_solver_scene

import sim3_solver_numpy as S

pytestmark = pytest.mark.gpu
POISON = -7
ERR_ARG, ERR_UNSUPPORTED = -1, -5


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _raw(ctx, scenes, want_hyp=True, want_inl=True, single=False, B=None):
    """The C entry point itself on a list of scenes -> (return value, [outputs per problem])."""
    n_p = len(scenes)
    probs, ress = (Sim3ProblemC * max(n_p, 1))(), (Sim3ResultC * max(n_p, 1))()
    keep, outs = [], []
    for b, s in enumerate(scenes):
        arrs = [np.ascontiguousarray(s[k], np.float32) for k in ("X1", "X2", "max_err1", "max_err2")]
        tri = np.ascontiguousarray(s["triples"], np.int32)
        n, H = s.get("n", arrs[0].shape[0]), s.get("n_hyp", tri.shape[0])
        n_inl = np.full(max(H, 1), POISON, np.int32)
        hyp = np.full((max(H, 1), 13), POISON, np.float32) if want_hyp else None
        inl = np.full(max(n, 1), 0xAB, np.uint8) if want_inl else None
        nulls = s.get("null", ())
        pp = {k: (None if k in nulls else ptr(a)) for k, a in zip(("X1", "X2", "max_err1", "max_err2"), arrs)}
        probs[b] = Sim3ProblemC((ctypes.c_float * 4)(*s["cam1"]), (ctypes.c_float * 4)(*s["cam2"]), n, pp["X1"],
                                pp["X2"], pp["max_err1"], pp["max_err2"], int(s["fix_scale"]), int(s["min_inliers"]),
                                H, None if "triples" in nulls else ptr(tri))
        ress[b].n_inliers = None if "n_inliers" in nulls else ptr(n_inl)
        ress[b].hyp, ress[b].inliers = ptr(hyp), ptr(inl)
        ress[b].sel = (ctypes.c_float * 13)(*([POISON] * 13))
        ress[b].converged = ress[b].best = POISON
        keep.append((arrs, tri))
        outs.append((n_inl, hyp, inl))
    if single:
        rc = lib().orbhip_sim3_solve(ctx.handle, probs, ress)
    else:
        rc = lib().orbhip_sim3_solve_batch(ctx.handle, probs, n_p if B is None else B, ress)
    got = [dict(n_inliers=o[0], hyp=o[1], inliers=o[2], sel=np.array(ress[b].sel, np.float32),
                converged=int(ress[b].converged), best=int(ress[b].best)) for b, o in enumerate(outs)]
    return rc, got


def _same_floats(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _assert_equal(got, want, what=""):
    H = len(want["n_inliers"])
    bad = np.nonzero(got["n_inliers"][:H] != want["n_inliers"])[0]
    assert bad.size == 0, f"{what} n_inliers: {len(bad)} hypotheses differ, first {bad[:5].tolist()}: gpu " \
                          f"{got['n_inliers'][bad[:5]].tolist()} restatement {want['n_inliers'][bad[:5]].tolist()}"
    if got["hyp"] is not None:
        assert _same_floats(got["hyp"][:H], want["hyp"]), f"{what} hyp"
    assert (got["converged"], got["best"]) == (want["converged"], want["best"]), what
    assert _same_floats(got["sel"], want["sel"]), f"{what} sel"
    if got["inliers"] is not None:
        assert np.array_equal(got["inliers"][:len(want["inliers"])], want["inliers"].astype(np.uint8)), f"{what} inliers"


def _untouched(got):
    for g in got:
        assert (g["n_inliers"] == POISON).all() and (g["hyp"] == POISON).all() and (g["inliers"] == 0xAB).all()
        assert (g["sel"] == POISON).all() and g["converged"] == POISON and g["best"] == POISON


def _mirror_of(s, ctx, max_its=None):
    m = Sim3Solver(s["X1"], s["X2"], s["octaves1"], s["octaves2"], s["level_sigma2"], s["level_sigma2"], s["cam1"],
                   s["cam2"], s["fix_scale"], s["indices1"], s["n1"], ctx=ctx)
    m.SetRansacParameters(0.99, s["min_inliers"], len(s["triples"]) if max_its is None else max_its)
    return m


def _prefix(e, H, min_inliers):
    """The restatement's result for the first H hypotheses of a solved scene."""
    conv, best = S.select(e["n_inliers"][:H], min_inliers)
    return dict(n_inliers=e["n_inliers"][:H], hyp=e["hyp"][:H], converged=conv, best=best, sel=e["hyp"][best],
                inliers=e["masks"][best])


# ---- the parity scenes ----

@pytest.mark.parametrize("k,fs", [(k, fs) for k in range(len(S.PARITY_CASES)) for fs in (False, True)])
def test_parity_scene_set(ctx, k, fs):
    """n in {257, 100, 30, 20} x both fix_scale values, 300 hypotheses: the scenes whose conditions
    tests/test_sim3_solver.py asserts, through the C call and through the mirror (which solves the
    mRansacMaxIts hypotheses upstream's clamp leaves)."""
    s = S.parity_scene(k, fs)
    want = s["expected"]
    rc, got = _raw(ctx, [s])
    assert rc == int(want["converged"] >= 0)
    _assert_equal(got[0], want)
    m = _mirror_of(s, ctx)
    m.solve(s["triples"])
    H = m.mRansacMaxIts
    r = dict(m._solved, inliers=m._solved["inliers"].astype(np.uint8))
    assert len(r["n_inliers"]) == H
    _assert_equal(r, _prefix(want, H, s["min_inliers"]), "mirror")


# ---- edges ----

@pytest.mark.parametrize("n", [3, 4, 63, 64, 65, 127, 128, 129])
def test_correspondence_count_edges(ctx, n):
    """Correspondences at the wave boundaries (one mask word per 64), both scale modes in one call."""
    scenes = [synthetic_sim3_solver_scene(n, 0.3, 40 + n, fs, n_hyp=12, min_inliers=min(6, n - 1)) for fs in (False, True)]
    want = [S.solve_scene(s) for s in scenes]
    rc, got = _raw(ctx, scenes)
    assert rc == sum(w["converged"] >= 0 for w in want)
    for g, w in zip(got, want):
        _assert_equal(g, w)
    assert n < 20 or any(w["n_inliers"].max() > 0 for w in want)


@pytest.mark.parametrize("H", [1, 2, 3, 4, 5, 63, 64, 65])
def test_hypothesis_count_edges(ctx, H):
    """Hypotheses at the work-group boundary (four waves each) and the select kernel's stride."""
    s = synthetic_sim3_solver_scene(70, 0.4, 60 + H, H % 2 == 0, n_hyp=H, min_inliers=12)
    want = S.solve_scene(s)
    rc, got = _raw(ctx, [s])
    assert rc == int(want["converged"] >= 0)
    _assert_equal(got[0], want)


@pytest.mark.parametrize("B", [1, 2, 3, 64])
def test_batch_edges(ctx, B):
    """A different n, H, camera pair, scale mode and minimum per problem of one call."""
    scenes = []
    for b in range(B):
        cam1 = dict(fx=500.0 + 3 * b, fy=510.0 - b, cx=320.0 + b, cy=240.5)
        cam2 = dict(fx=450.0 + b, fy=455.0 + 2 * b, cx=300.25, cy=230.0 - b)
        scenes.append(synthetic_sim3_solver_scene(3 + (7 * b) % 131, 0.35, 500 + b, b % 2 == 1, n_hyp=1 + (5 * b) % 23,
                                                  min_inliers=3 + b % 5, cam1=cam1, cam2=cam2))
    want = [S.solve_scene(s) for s in scenes]
    rc, got = _raw(ctx, scenes)
    assert rc == sum(w["converged"] >= 0 for w in want)
    for b, (g, w) in enumerate(zip(got, want)):
        _assert_equal(g, w, f"problem {b}")


# ---- degenerate inputs ----

def _hand_scene(X1, X2, triples, fix_scale, min_inliers=1, bound=20.0):
    n = len(X1)
    return dict(X1=np.array(X1, np.float32), X2=np.array(X2, np.float32), max_err1=np.full(n, bound, np.float32),
                max_err2=np.full(n, bound, np.float32), cam1=np.array([500, 500, 320, 240], np.float32),
                cam2=np.array([480, 490, 310, 250], np.float32), fix_scale=fix_scale, min_inliers=min_inliers,
                triples=np.array(triples, np.int32))


@pytest.mark.parametrize("fs", [False, True])
def test_degenerate_triples_and_points(ctx, fs):
    """Three copies of one point (M = 0: a NaN scale when it is free, the identity and a translation
    when it is fixed), a collinear triple (a double largest eigenvalue), a correspondence with z = 0 as
    a member of a triple and as a point to check: the counts and the bits of the restatement, with no
    special case on either side."""
    p, d = (0.5, -0.25, 4.0), (0.25, 0.5, 0.125)
    X1 = [p, p, p] + [tuple(p[j] + k * d[j] for j in range(3)) for k in range(3)] + [(0.75, 0.5, 0.0), (1.0, -1.0, 5.0),
                                                                                    (-1.5, 0.25, 3.0), (0.0, 0.0, 6.0)]
    q = (0.25, 0.125, 3.5)
    X2 = [q, q, q] + [tuple(q[j] + k * d[(j + 1) % 3] for j in range(3)) for k in range(3)] + \
         [(0.5, 0.25, 0.0), (1.25, -0.75, 5.5), (-1.25, 0.5, 3.25), (0.125, -0.125, 6.5)]
    tri = [(0, 1, 2), (3, 4, 5), (2, 1, 0), (6, 7, 8), (7, 8, 9), (5, 6, 9), (0, 3, 7), (9, 8, 7)]
    s = _hand_scene(X1, X2, tri, fs)
    want = S.solve_scene(s)
    assert np.isnan(want["hyp"][0]).any() == (not fs) and (fs or want["n_inliers"][0] == 0)
    if fs:   # M = 0 leaves the Jacobi nothing to rotate: the first column, the identity
        assert np.array_equal(want["hyp"][0][1:10].reshape(3, 3), np.eye(3, dtype=np.float32))
    assert np.isfinite(want["hyp"][7]).all()
    rc, got = _raw(ctx, [s])
    assert rc == int(want["converged"] >= 0)
    _assert_equal(got[0], want)


def test_three_exact_correspondences(ctx):
    """n = 3 with X1 = s R X2 + t exactly (a quarter turn, s = 2, dyadic coordinates): every
    permutation of the one triple finds all three."""
    X2 = np.array([(0.5, 0.25, 2.0), (-0.75, 0.5, 3.0), (0.25, -0.5, 2.5)], np.float32)
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    X1 = (2.0 * X2 @ R.T + np.array([0.5, -0.25, 1.0], np.float32)).astype(np.float32)
    s = _hand_scene(X1, X2, list(itertools.permutations(range(3))), False, min_inliers=2, bound=9.0)
    want = S.solve_scene(s)
    assert (want["n_inliers"] == 3).all() and want["converged"] == 0 and want["inliers"].all()
    rc, got = _raw(ctx, [s])
    assert rc == 1
    _assert_equal(got[0], want)


# ---- selection ----

def test_selection_ties_minimum_and_no_convergence(ctx):
    """A repeated triple (the later one wins), the minimum at an attained count (strict >), one below
    it (the FIRST hypothesis of that count converges), and a minimum nothing reaches: four problems
    of one call."""
    s = S.parity_scene(3, True)
    e = s["expected"]
    top = int(e["n_inliers"].max())
    first = int(np.argmax(e["n_inliers"]))
    tri = s["triples"].copy()
    later = S.PARITY_H - 3
    tri[later] = tri[first]
    scenes = [dict(s, triples=tri), dict(s, min_inliers=top), dict(s, min_inliers=top - 1), dict(s, min_inliers=10 ** 6)]
    want = [S.solve_scene(x) for x in scenes[:1]] + [dict(_prefix(e, S.PARITY_H, x["min_inliers"])) for x in scenes[1:]]
    assert (want[0]["converged"], want[0]["best"]) == (-1, later)
    assert want[1]["converged"] == -1 and want[1]["best"] == int(np.nonzero(e["n_inliers"] == top)[0][-1])
    assert want[2]["converged"] == want[2]["best"] == first
    assert want[3]["converged"] == -1 and want[3]["best"] == want[1]["best"]
    rc, got = _raw(ctx, scenes)
    assert rc == 1
    for b, (g, w) in enumerate(zip(got, want)):
        _assert_equal(g, w, f"problem {b}")


# ---- calling conventions ----

def test_optional_outputs_and_repeatability(ctx):
    s = S.parity_scene(2, False)
    want = s["expected"]
    for want_hyp, want_inl in ((False, False), (True, False), (False, True)):
        rc, got = _raw(ctx, [s], want_hyp, want_inl)
        assert rc == 1
        _assert_equal(got[0], want)
    a, b = _raw(ctx, [s, S.parity_scene(1, True)]), _raw(ctx, [s, S.parity_scene(1, True)])
    assert a[0] == b[0]
    for ga, gb in zip(a[1], b[1]):
        for key in ("n_inliers", "hyp", "inliers", "sel"):
            assert ga[key].tobytes() == gb[key].tobytes()
        assert (ga["converged"], ga["best"]) == (gb["converged"], gb["best"])
    rc, got = _raw(ctx, [s], single=True)   # the B = 1 entry point
    assert rc == 1
    _assert_equal(got[0], want)
    assert _raw(ctx, [], B=0)[0] == 0


@pytest.mark.parametrize("k,fs", [(0, False), (1, True), (2, True), (3, False)])
def test_iterate_in_chunks_equals_the_literal_loop(ctx, k, fs):
    """Sim3Solver.iterate(20) called until it converges or gives up, over ONE device call, against
    upstream's loop computed hypothesis by hypothesis: matrix, flags, nInliers, vbInliers through
    indices1."""
    s = S.parity_scene(k, fs)
    m = _mirror_of(s, ctx)
    m.solve(s["triples"])
    lit = S.LiteralSolver(s, s["min_inliers"], m.mRansacMaxIts, s["triples"])
    for _ in range(m.mRansacMaxIts // 20 + 2):
        a, b = lit.iterate(20), m.iterate(20)
        assert _same_floats(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2]) and a[3:] == b[3:]
        assert len(b[2]) == s["n1"] and lit.mnIterations == m.mnIterations
        if a[1] or a[4]:
            break
    assert a[1] or a[4]


def test_solve_batch_serves_several_candidates(ctx):
    scenes = [S.parity_scene(0, False), S.parity_scene(1, True), S.parity_scene(2, False)]
    ms = [_mirror_of(s, ctx) for s in scenes]
    rc = Sim3Solver.solve_batch(ms, [s["triples"] for s in scenes])
    assert rc == sum(m._solved["converged"] >= 0 for m in ms) == 2
    for m, s in zip(ms, scenes):
        r = dict(m._solved, inliers=m._solved["inliers"].astype(np.uint8))
        _assert_equal(r, _prefix(s["expected"], m.mRansacMaxIts, s["min_inliers"]))
    own = _mirror_of(scenes[2], None)   # without a context the solver makes its own at the first call, and keeps it
    assert own.ctx is None
    own.solve(scenes[2]["triples"])
    made = own.ctx
    assert made is not None and own.solve(scenes[2]["triples"]).ctx is made
    assert own._solved["n_inliers"].tobytes() == ms[2]._solved["n_inliers"].tobytes()
    made.close()


def test_profile_stage_brackets_the_two_launches(ctx):
    L = lib()
    s = S.parity_scene(2, True)
    assert L.orbhip_profile_stage(ctx.handle, 11) == 0
    for _ in range(3):
        assert _raw(ctx, [s])[0] == 1
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(ctx.handle, 0) == 0
    assert cnt.value == 3 and 0.0 < ms.value < 1000.0
    assert L.orbhip_profile_stage(ctx.handle, 12) == ERR_ARG


# ---- argument errors ----

def _bad(s, **changes):
    return dict(s, **changes)


def test_argument_errors_leave_the_outputs_untouched(ctx):
    s = synthetic_sim3_solver_scene(40, 0.3, 9, False, n_hyp=6, min_inliers=5)
    ok = _raw(ctx, [s])
    assert ok[0] >= 0
    nan, inf = float("nan"), float("inf")

    def tri_with(h, triple):
        t = s["triples"].copy()
        t[h] = triple
        return t

    def cam_with(i, v):
        c = s["cam1"].copy()
        c[i] = v
        return c
    cases = [(ERR_ARG, _bad(s, n=2)), (ERR_ARG, _bad(s, n=0)), (ERR_ARG, _bad(s, n=-1)),
             (ERR_ARG, _bad(s, n_hyp=0)), (ERR_ARG, _bad(s, min_inliers=-1))]
    cases += [(ERR_ARG, _bad(s, null=(k,))) for k in ("X1", "X2", "max_err1", "max_err2", "triples", "n_inliers")]
    cases += [(ERR_ARG, _bad(s, triples=tri_with(h, t))) for h, t in
              ((0, (0, 1, 40)), (5, (-1, 2, 3)), (3, (7, 7, 9)), (2, (4, 8, 4)), (5, (1, 6, 6)))]
    cases += [(ERR_ARG, _bad(s, cam1=cam_with(i, v))) for i in (0, 1) for v in (0.0, -500.0, nan, inf)]
    cases += [(ERR_ARG, _bad(s, cam2=cam_with(1, nan)))]
    big_n = 8193
    big = dict(s, X1=np.ones((big_n, 3), np.float32), X2=np.ones((big_n, 3), np.float32),
               max_err1=np.ones(big_n, np.float32), max_err2=np.ones(big_n, np.float32))
    cases += [(ERR_UNSUPPORTED, big),
              (ERR_UNSUPPORTED, _bad(s, triples=np.tile(s["triples"], (700, 1))[:4097]))]
    for code, bad in cases:
        for scenes in ([bad], [s, bad]):   # alone, and behind a valid problem: nothing of the call runs
            rc, got = _raw(ctx, scenes)
            assert rc == code, (rc, code, {k: v for k, v in bad.items() if k in ("n", "n_hyp", "min_inliers", "null")})
            _untouched(got)
    rc, got = _raw(ctx, [s] * 65)
    assert rc == ERR_UNSUPPORTED
    _untouched(got)
    rc, got = _raw(ctx, [s], B=-1)
    assert rc == ERR_ARG
    _untouched(got)
    assert lib().orbhip_sim3_solve_batch(ctx.handle, None, 1, None) == ERR_ARG
    assert lib().orbhip_sim3_solve(ctx.handle, None, None) == ERR_ARG
    # the envelope's last sizes are inside it
    edge = dict(big, X1=big["X1"][:8192], X2=big["X2"][:8192], max_err1=big["max_err1"][:8192],
                max_err2=big["max_err2"][:8192], triples=s["triples"][:2])
    assert _raw(ctx, [edge])[0] >= 0
    after = _raw(ctx, [s])   # and the context is as good as before
    assert after[0] == ok[0]
    _assert_equal(after[1][0], dict(ok[1][0], inliers=ok[1][0]["inliers"].astype(bool)))
