"""orbhip_two_view_reconstruct_batch on the GPU against the numpy restatement
(tests/two_view_numpy.py): the integer and boolean outputs must be EQUAL and the fp32 outputs equal
bit for bit (a NaN matches a NaN at the same place); only `parallax`, which goes through the
device's acosf, may differ, by PARALLAX_ULPS. Outputs are pre-filled with a poison value.

CheckRT's gates are reached through whole scenes: tests/test_two_view.py shows that the scene set
meets points behind a camera on both sides of the cosine limit, and that th2_at / th2_above put th2
exactly on one match's reprojection error and one step below it."""
import ctypes

import numpy as np
import pytest

from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, TwoViewProblemC, TwoViewResultC, lib, ptr
from orb_slam3_ros2_amd.two_view import TwoViewReconstruction

import two_view_cases as C
import two_view_numpy as T

pytestmark = pytest.mark.gpu
POISON = -7
ERR_ARG, ERR_UNSUPPORTED = -1, -5
# parallax = acos(cos_sel) * 180 / pi in degrees: the device's acosf against numpy's. Measured on
# the first GPU run over every case of this file: at most 3 ulp of the result; asserted at 4x that.
PARALLAX_ULPS = 12


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


def _kps(xy):
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    return k


def _raw(ctx, problems, want_masks=True, single=False, B=None):
    """The C entry point itself on a list of problems -> (return value, [outputs per problem])."""
    n_p = len(problems)
    probs, ress = (TwoViewProblemC * max(n_p, 1))(), (TwoViewResultC * max(n_p, 1))()
    keep, outs = [], []
    for b, p in enumerate(problems):
        k1, k2 = _kps(np.asarray(p["kps1"], np.float32)), _kps(np.asarray(p["kps2"], np.float32))
        m = np.ascontiguousarray(p["matches12"], np.int32)
        sets = np.ascontiguousarray(p["sets"], np.int32)
        n1, n2, H = p.get("n1", len(k1)), p.get("n2", len(k2)), p.get("n_hyp", len(sets))
        N = max(int((m >= 0).sum()), 1)
        p3d = np.full((max(len(k1), 1), 3), POISON, np.float32)
        tri = np.full(max(len(k1), 1), 0xAB, np.uint8)
        ih = np.full(N, 0xAB, np.uint8) if want_masks else None
        jf = np.full(N, 0xAB, np.uint8) if want_masks else None
        nulls = p.get("null", ())
        pp = {k: (None if k in nulls else ptr(a)) for k, a in
              (("kps1", k1), ("kps2", k2), ("matches12", m), ("sets", sets), ("p3d", p3d), ("triangulated", tri))}
        probs[b] = TwoViewProblemC(n1, n2, pp["kps1"], pp["kps2"], pp["matches12"], (ctypes.c_float * 4)(*p["K"]),
                                   float(p.get("sigma", 1.0)), H, pp["sets"])
        r = ress[b]
        r.p3d, r.triangulated, r.inliers_h, r.inliers_f = pp["p3d"], pp["triangulated"], ptr(ih), ptr(jf)
        r.success = r.model = r.best_h = r.best_f = r.chosen = POISON
        r.SH = r.SF = POISON
        for name, cnt in (("H21", 9), ("F21", 9), ("R21", 9), ("t21", 3), ("parallax", 8), ("cos_sel", 8)):
            setattr(r, name, (ctypes.c_float * cnt)(*([POISON] * cnt)))
        r.n_good = (ctypes.c_int32 * 8)(*([POISON] * 8))
        keep.append((k1, k2, m, sets))
        outs.append((p3d, tri, ih, jf))
    if single:
        rc = lib().orbhip_two_view_reconstruct(ctx.handle, probs, ress)
    else:
        rc = lib().orbhip_two_view_reconstruct_batch(ctx.handle, probs, n_p if B is None else B, ress)
    got = []
    for b, (p3d, tri, ih, jf) in enumerate(outs):
        r = ress[b]
        got.append(dict(success=int(r.success), model=int(r.model), best_h=int(r.best_h), best_f=int(r.best_f),
                        chosen=int(r.chosen), SH=np.float32(r.SH), SF=np.float32(r.SF), H21=np.array(r.H21, np.float32),
                        F21=np.array(r.F21, np.float32), R21=np.array(r.R21, np.float32), t21=np.array(r.t21, np.float32),
                        n_good=np.array(r.n_good, np.int32), parallax=np.array(r.parallax, np.float32),
                        cos_sel=np.array(r.cos_sel, np.float32), p3d=p3d, triangulated=tri, inl_h=ih, inl_f=jf))
    return rc, got


def _same_floats(a, b):
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def _ulps(a, b):
    """distance in fp32 steps between finite values of one sign (both NaN: 0)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


WORST = {"parallax_ulps": 0}


def _assert_equal(got, want, what=""):
    for k in ("success", "model", "best_h", "best_f", "chosen"):
        assert got[k] == int(want[k]), f"{what} {k}: gpu {got[k]} restatement {want[k]}"
    assert np.array_equal(got["n_good"], want["n_good"]), f"{what} n_good: gpu {got['n_good']} restatement {want['n_good']}"
    for k in ("SH", "SF", "H21", "F21", "R21", "t21", "cos_sel"):
        assert _same_floats(got[k], want[k]), f"{what} {k}: gpu {got[k]} restatement {np.asarray(want[k]).reshape(-1)}"
    if got["inl_h"] is not None:
        assert np.array_equal(got["inl_h"], want["inl_h"].astype(np.uint8)), f"{what} inliers_h"
        assert np.array_equal(got["inl_f"], want["inl_f"].astype(np.uint8)), f"{what} inliers_f"
    n1 = len(want["triangulated"])
    assert np.array_equal(got["triangulated"][:n1], want["triangulated"].astype(np.uint8)), f"{what} triangulated"
    assert _same_floats(got["p3d"][:n1], want["p3d"]), f"{what} p3d"
    u = _ulps(got["parallax"], want["parallax"])
    WORST["parallax_ulps"] = max(WORST["parallax_ulps"], int(u.max()))
    print(f"{what} parallax: largest difference {int(u.max())} ulp (worst so far {WORST['parallax_ulps']})")
    assert (u <= PARALLAX_ULPS).all(), f"{what} parallax: gpu {got['parallax']} restatement {want['parallax']}"


# ---- the parity scenes ----

@pytest.mark.parametrize("name", C.PARITY)
def test_parity_scene_set(ctx, name):
    p, _, want = T.expected(name)
    rc, got = _raw(ctx, [p])
    assert rc == want["success"]
    _assert_equal(got[0], want, name)


@pytest.mark.parametrize("name", C.EXITS)
def test_each_exit_of_the_reconstructions(ctx, name):
    """The crafted scenes whose exits tests/test_two_view.py asserts on the restatement"""
    p, _, want = T.expected(name)
    rc, got = _raw(ctx, [p])
    assert rc == 0 and want["success"] == 0
    _assert_equal(got[0], want, name)


@pytest.mark.parametrize("name", ["good_le_50", "good_51", "good_many"])
def test_both_arms_of_the_cosine_index(ctx, name):
    """At most 50 counted points (index size - 1), exactly 51 (both agree), more (index 50)"""
    p, _, want = T.expected(name)
    rc, got = _raw(ctx, [p])
    assert rc == want["success"]
    _assert_equal(got[0], want, name)


# ---- size edges ----

@pytest.mark.parametrize("n", [8, 9, 63, 64, 65, 128, 129])
def test_match_count_edges(ctx, n):
    p = C.sized(n, 12, seed=n)
    want = T.reconstruct(p)
    rc, got = _raw(ctx, [p])
    assert rc == want["success"]
    _assert_equal(got[0], want, f"n={n}")


@pytest.mark.parametrize("H", [1, 2, 63, 64, 65, 200])
def test_hypothesis_count_edges(ctx, H):
    p = C.sized(70, H, seed=H)
    want = T.reconstruct(p)
    rc, got = _raw(ctx, [p])
    assert rc == want["success"]
    _assert_equal(got[0], want, f"H={H}")


@pytest.mark.parametrize("B", [1, 2, 3, 64])
def test_batch_edges(ctx, B):
    """A different match count, set count, camera and unmatched share per problem of one call"""
    ps = [C.batch_problem(b) for b in range(B)]
    want = [T.reconstruct(p) for p in ps]
    rc, got = _raw(ctx, ps)
    assert rc == sum(w["success"] for w in want)
    for b, (g, w) in enumerate(zip(got, want)):
        _assert_equal(g, w, f"problem {b}")


# ---- degenerate sets ----

def test_degenerate_sets(ctx):
    """Eight copies of one point in a set (the Gram matrix has rank 2: the Jacobi yields a finite
    vector of its null space, whatever its score it does not beat the sound sets), two identical
    sets (the first wins), a problem whose matches all coincide (every matrix NaN: SH + SF == 0,
    model -1, failure), and one whose every set is drawn from eight coincident matches among distinct
    ones (every hypothesis from a null space of several dimensions; whatever the restatement gives)."""
    D = C.degenerate_problems()
    names = ("twins", "identical", "coincident", "all_sets_degenerate")
    want = {k: T.reconstruct(D[k]) for k in names}
    p = D["twins"]
    assert want["twins"]["best_h"] != p["twin_h"] and want["twins"]["best_f"] != p["twin_h"]
    assert want["identical"]["best_f"] == 0 and want["identical"]["SF"] == want["twins"]["SF"]
    w = want["coincident"]
    assert w["model"] == -1 and w["success"] == 0 and w["SH"] == 0 and w["SF"] == 0
    rc, got = _raw(ctx, [D[k] for k in names])
    assert rc == sum(want[k]["success"] for k in names)
    for g, k in zip(got, names):
        _assert_equal(g, want[k], k)


@pytest.mark.parametrize("name", C.TH2)
def test_reprojection_error_exactly_at_th2(ctx, name):
    """sigma puts th2 on a match's fp32 reprojection error (counted) and one step below it (not
    counted): tests/test_two_view.py asserts that on the restatement"""
    p, _, want = T.expected(name)
    rc, got = _raw(ctx, [p])
    assert rc == want["success"] == 1
    _assert_equal(got[0], want, name)
    assert want["n_good"][C.TH2_MATCH["hypothesis"]] == (208 if name == "th2_at" else 207)


# ---- calling conventions ----

def test_optional_outputs_and_repeatability(ctx):
    p, _, want = T.expected("general")
    rc, got = _raw(ctx, [p], want_masks=False)
    assert rc == 1
    _assert_equal(got[0], want)
    q = T.expected("planar")[0]
    a, b = _raw(ctx, [p, q]), _raw(ctx, [p, q])
    assert a[0] == b[0] == 2
    for ga, gb in zip(a[1], b[1]):
        for key, va in ga.items():
            assert (va.tobytes() == gb[key].tobytes()) if isinstance(va, np.ndarray) else (va == gb[key]), key
    rc, got = _raw(ctx, [p], single=True)   # the B = 1 entry point
    assert rc == 1
    _assert_equal(got[0], want)
    assert _raw(ctx, [], B=0)[0] == 0


def test_profile_stage_brackets_the_launches(ctx):
    L = lib()
    p = T.expected("general")[0]
    assert L.orbhip_profile_stage(ctx.handle, 16) == 0
    for _ in range(3):
        assert _raw(ctx, [p])[0] == 1
    ms, cnt = ctypes.c_double(), ctypes.c_int32()
    assert L.orbhip_profile_collect(ctx.handle, ctypes.byref(ms), ctypes.byref(cnt)) == 0
    assert L.orbhip_profile_stage(ctx.handle, 0) == 0
    assert cnt.value == 3 and 0.0 < ms.value < 1000.0
    assert L.orbhip_profile_stage(ctx.handle, 17) == ERR_ARG


def _untouched(got):
    for g in got:
        assert (g["p3d"] == POISON).all() and (g["triangulated"] == 0xAB).all()
        assert (g["inl_h"] == 0xAB).all() and (g["inl_f"] == 0xAB).all()
        for k in ("success", "model", "best_h", "best_f", "chosen", "SH", "SF"):
            assert g[k] == POISON, k
        for k in ("H21", "F21", "R21", "t21", "n_good", "parallax", "cos_sel"):
            assert (g[k] == POISON).all(), k


def test_argument_errors_leave_the_outputs_untouched(ctx):
    s = C.sized(40, 6, seed=9, unmatched_frac=0.25)
    ok = _raw(ctx, [s])
    assert ok[0] >= 0
    nan, inf = float("nan"), float("inf")
    N = int((s["matches12"] >= 0).sum())

    def sets_with(h, k, v):
        t = s["sets"].copy()
        t[h, k] = v
        return t

    def K_with(i, v):
        c = s["K"].copy()
        c[i] = v
        return c

    def match_with(v):
        m = s["matches12"].copy()
        m[np.nonzero(m >= 0)[0][3]] = v
        return m
    few = s["matches12"].copy()
    few[np.nonzero(few >= 0)[0][7:]] = -1          # 7 matches are left
    cases = [(ERR_ARG, dict(s, matches12=few)), (ERR_ARG, dict(s, n_hyp=0)), (ERR_ARG, dict(s, n_hyp=-1))]
    cases += [(ERR_ARG, dict(s, null=(k,))) for k in ("kps1", "kps2", "matches12", "sets", "p3d", "triangulated")]
    cases += [(ERR_ARG, dict(s, matches12=match_with(v))) for v in (-2, len(s["kps2"]), 2 ** 30)]
    cases += [(ERR_ARG, dict(s, sets=sets_with(h, k, v))) for h, k, v in
              ((0, 0, N), (5, 7, -1), (3, 2, int(s["sets"][3, 6])), (2, 7, int(s["sets"][2, 0])))]
    cases += [(ERR_ARG, dict(s, K=K_with(i, v))) for i in (0, 1) for v in (0.0, -500.0, nan, inf)]
    cases += [(ERR_ARG, dict(s, sigma=v)) for v in (0.0, -1.0, nan, inf)]
    big_n = 8193
    big = dict(s, kps1=np.ones((big_n, 2), np.float32), kps2=np.ones((big_n, 2), np.float32),
               matches12=np.arange(big_n, dtype=np.int32))
    cases += [(ERR_UNSUPPORTED, big), (ERR_UNSUPPORTED, dict(s, sets=np.tile(s["sets"], (700, 1))[:4097]))]
    for code, bad in cases:
        for ps in ([bad], [s, bad]):   # alone, and behind a valid problem: nothing of the call runs
            rc, got = _raw(ctx, ps)
            assert rc == code, (rc, code, {k: v for k, v in bad.items() if k in ("n_hyp", "null", "sigma")})
            _untouched(got)
    rc, got = _raw(ctx, [s] * 65)
    assert rc == ERR_UNSUPPORTED
    _untouched(got)
    rc, got = _raw(ctx, [s], B=-1)
    assert rc == ERR_ARG
    _untouched(got)
    assert lib().orbhip_two_view_reconstruct_batch(ctx.handle, None, 1, None) == ERR_ARG
    assert lib().orbhip_two_view_reconstruct(ctx.handle, None, None) == ERR_ARG
    # the envelope's last sizes are inside it
    edge = dict(big, kps1=big["kps1"][:8192], kps2=big["kps2"][:8192], matches12=big["matches12"][:8192],
                sets=s["sets"][:2])
    assert _raw(ctx, [edge])[0] >= 0
    after = _raw(ctx, [s])   # and the context is as good as before
    assert after[0] == ok[0]
    for key, va in ok[1][0].items():
        assert (va.tobytes() == after[1][0][key].tobytes()) if isinstance(va, np.ndarray) else (va == after[1][0][key])


# ---- the Python class ----

@pytest.mark.parametrize("name", C.PARITY)
def test_python_class_gives_what_the_literal_solver_gives(ctx, name):
    """TwoViewReconstruction.Reconstruct against upstream's sequential loop with its fp32 running
    score (tests/test_two_view.py shows that it picks the same hypotheses on these scenes)"""
    p = C.scene(name)
    ok, T21, vP3D, vbTri, o = T.LiteralSolver(p).Reconstruct()
    tv = TwoViewReconstruction(p["K"], p["sigma"], len(p["sets"]), ctx=ctx)
    got = tv.Reconstruct(p["kps1"], p["kps2"], p["matches12"], p["sets"])
    assert got[0] == ok
    assert _same_floats(got[1], T21) and _same_floats(got[2], vP3D) and np.array_equal(got[3], vbTri)
    assert tv.last["best_h"] == o["best_h"] and tv.last["best_f"] == o["best_f"] and tv.last["model"] == o["model"]


def test_reconstruct_batch_serves_several_pairs(ctx):
    names = ("general", "planar", "rotation")
    ps = [C.scene(n) for n in names]
    tvs = [TwoViewReconstruction(p["K"], p["sigma"], len(p["sets"]), ctx=ctx) for p in ps]
    got = TwoViewReconstruction.reconstruct_batch(tvs, [(p["kps1"], p["kps2"], p["matches12"], p["sets"]) for p in ps])
    for n, g in zip(names, got):
        w = T.expected(n)[2]
        assert g[0] == bool(w["success"]) and _same_floats(g[2], w["p3d"]) and np.array_equal(g[3], w["triangulated"])
