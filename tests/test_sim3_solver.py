"""Sim3Solver on the CPU: the rule the device call reproduces (tests/sim3_solver_numpy.py), checked
against upstream's literal sequential loop; the Python mirror's state machine; the scene set the GPU
tests compare on. No device is used."""
import math

import numpy as np
import pytest

import sim3_solver_numpy as S
from orb_slam3_ros2_amd import _lib
from orb_slam3_ros2_amd.sim3solver import Sim3Solver, draw_triples, error_bounds

SCENES = [(k, fs) for k in range(len(S.PARITY_CASES)) for fs in (False, True)]


def _mirror_of(s, ctx=None):
    m = Sim3Solver(s["X1"], s["X2"], s["octaves1"], s["octaves2"], s["level_sigma2"], s["level_sigma2"], s["cam1"],
                   s["cam2"], s["fix_scale"], s["indices1"], s["n1"], ctx=ctx)
    return m


def _inject(m, r, triples):
    """The mirror's stored results as the device call would leave them (here: the restatement's)."""
    m._solved = dict(triples=triples, n_inliers=r["n_inliers"], hyp=r["hyp"], inliers=r["inliers"], sel=r["sel"],
                     converged=r["converged"], best=r["best"])


def _same_iterate(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) or
            (np.array_equal(np.isnan(a[0]), np.isnan(b[0])) and
             np.array_equal(a[0][~np.isnan(a[0])], b[0][~np.isnan(b[0])]))) and a[1] == b[1] and \
        np.array_equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


# ---- the selection: the literal loop and its order-free form ----

@pytest.mark.parametrize("k,fs", SCENES)
def test_selection_equals_the_literal_loop_on_counts(k, fs):
    """For every chunk size the sequential rule, applied to the scene's counts, ends where the
    order-free form says; so does it at a minimum equal to an attained count (strict >) and one below."""
    n = S.parity_scene(k, fs)["expected"]["n_inliers"]
    attained = sorted(set(int(c) for c in n if c > 0))
    mins = {S.PARITY_MIN_INLIERS, 0, int(n.max()), max(int(n.max()) - 1, 0)}
    if attained:
        mins |= {attained[len(attained) // 2], max(attained[len(attained) // 2] - 1, 0)}
    for min_inliers in sorted(mins):
        want = S.select(n, min_inliers)
        for chunk in (1, 5, 20, 300):
            assert S.literal_from_counts(n, min_inliers, chunk) == want, (min_inliers, chunk)
    # strict >: at the largest count nothing converges and the last hypothesis that attains it is the best
    conv, best = S.select(n, int(n.max()))
    assert conv == -1 and best == int(np.nonzero(n == n.max())[0][-1])
    conv, best = S.select(n, int(n.max()) - 1) if n.max() > 0 else (0, 0)
    assert n.max() == 0 or conv == best == int(np.nonzero(n == n.max())[0][0])


@pytest.mark.parametrize("k,fs", SCENES)
@pytest.mark.parametrize("chunk", [1, 5, 20, 300])
def test_mirror_iterate_equals_the_literal_solver(k, fs, chunk):
    """Upstream's iterate(), one hypothesis after the other with its state kept across chunked calls,
    against the mirror's walk over the results of ONE call (here the restatement's): the same matrix,
    bNoMore, vbInliers through indices1, nInliers and bConverge after every chunk."""
    s = S.parity_scene(k, fs)
    m = _mirror_of(s)
    m.SetRansacParameters(0.99, S.PARITY_MIN_INLIERS, S.PARITY_H)
    max_its = m.mRansacMaxIts   # upstream's clamp: 300 at n = 257 and 100, 35 at n = 30, 9 at n = 20
    assert max_its == {257: 300, 100: 300, 30: 35, 20: 9}[s["X1"].shape[0]]
    lit = S.LiteralSolver(s, S.PARITY_MIN_INLIERS, max_its, s["triples"])
    e = s["expected"]
    _inject(m, e, s["triples"])
    for _ in range(max_its // chunk + 2):
        a, b = lit.iterate(chunk), m.iterate(chunk)
        assert _same_iterate(a, b), (lit.mnIterations, a[1:], b[1:])
        assert lit.mnIterations == m.mnIterations and lit.mnBestInliers == m.mnBestInliers
        if a[1] or a[4]:
            break
    assert a[1] or a[4]
    conv, best = S.select(e["n_inliers"][:max_its], S.PARITY_MIN_INLIERS)
    assert lit.best_h == best
    if conv >= 0:
        assert a[4] and conv == e["converged"] and a[3] == e["n_inliers"][conv]
        assert np.array_equal(a[2][s["indices1"]], e["masks"][conv]) and a[2].sum() == e["masks"][conv].sum()
    else:
        assert a[1] and not a[4] and a[3] == 0 and not a[2].any()
        assert np.array_equal(a[0].view(np.uint32), S.T12_of(e["hyp"][best]).view(np.uint32))


def test_repeated_triple_the_later_one_wins():
    """Ties made by repeating a triple: without a convergence the LAST hypothesis of the largest
    count is the best (upstream replaces on >=), in the loop and in the order-free form."""
    s = S.parity_scene(3, True)
    e = s["expected"]
    assert e["converged"] == -1
    first = int(np.argmax(e["n_inliers"]))
    last_at_max = int(np.nonzero(e["n_inliers"] == e["n_inliers"].max())[0][-1])
    tri = s["triples"].copy()
    later = S.PARITY_H - 3
    assert later > last_at_max
    tri[later] = tri[first]
    r = S.solve_scene(s, triples=tri)
    assert r["n_inliers"][later] == r["n_inliers"][first] == r["n_inliers"].max()
    assert r["converged"] == -1 and r["best"] == later
    lit = S.LiteralSolver(s, S.PARITY_MIN_INLIERS, S.PARITY_H, tri)
    out = lit.iterate(S.PARITY_H)
    assert lit.best_h == later and out[1] and not out[4]
    assert np.array_equal(out[0].view(np.uint32), S.T12_of(r["hyp"][later]).view(np.uint32))
    for chunk in (1, 5, 20, 300):
        assert S.literal_from_counts(r["n_inliers"], S.PARITY_MIN_INLIERS, chunk) == (-1, later)


def test_iterate_gives_up_below_the_minimum_and_past_the_cap():
    s = S.parity_scene(3, False)
    m = _mirror_of(s)
    m.SetRansacParameters(0.99, s["X1"].shape[0] + 1, 300)   # N < mRansacMinInliers
    T, no_more, vb, n, conv = m.iterate(5)
    assert no_more and not conv and n == 0 and not vb.any() and np.array_equal(T, np.eye(4, dtype=np.float32))
    m.SetRansacParameters(0.99, S.PARITY_MIN_INLIERS, 300)
    with pytest.raises(RuntimeError):
        m.iterate(5)   # nothing solved yet: there is no host fall-back


# ---- SetRansacParameters, error bounds, draw_triples ----

def _solver(N):
    z = np.zeros((N, 3), np.float32)
    o = np.zeros(N, np.int64)
    return Sim3Solver(z, z, o, o, [1.0], [1.0], (500, 500, 320, 240), (500, 500, 320, 240), False)


@pytest.mark.parametrize("N,min_inl,max_its,want", [
    (100, 20, 300, 300),   # epsilon 0.2: log(0.01) / log(1 - 0.008) = 573.3 -> 574, clamped to 300
    (20, 15, 300, 9),      # epsilon 0.75: log(0.01) / log(0.578125) = 8.404 -> 9
    (10, 6, 300, 19),      # epsilon 0.6: log(0.01) / log(0.784) = 18.92 -> 19
    (10, 6, 12, 12),       # the same, clamped by maxIterations
    (20, 20, 300, 1),      # minInliers == N: one iteration
    (257, 15, 300, 300),   # the parity scenes' setting: 23163 -> 300
])
def test_set_ransac_parameters(N, min_inl, max_its, want):
    m = _solver(N)
    assert (m.mRansacProb, m.mRansacMinInliers) == (0.99, 6)   # the constructor's defaults
    m.SetRansacParameters(0.99, min_inl, max_its)
    assert m.mRansacMaxIts == want and m.mnIterations == 0
    if min_inl != N:   # the arithmetic, restated: a float epsilon, the rest in double
        eps = float(np.float32(min_inl) / np.float32(N))
        assert want == max(1, min(math.ceil(math.log(1 - 0.99) / math.log(1 - eps ** 3)), max_its))


def test_error_bounds_are_truncated():
    """upstream keeps 9.210 * sigma2 in a vector<size_t>."""
    s2 = np.array([1.0, 1.44, 2.0736, 17.0], np.float32)
    got = error_bounds([0, 1, 2, 3, 1], s2)
    assert got.dtype == np.float32 and got.tolist() == [9.0, 13.0, 19.0, 156.0, 13.0]


def test_draw_triples_swap_remove_order():
    calls = []
    script = iter([0, 0, 0, 4, 1, 2, 2, 2, 2])

    def randint(lo, hi):
        calls.append((lo, hi))
        return next(script)
    t = draw_triples(5, 3, randint)
    # [0 1 2 3 4] -0-> 0, [4 1 2 3] -0-> 4, [3 1 2] -0-> 3;  -4-> 4, [0 1 2 3] -1-> 1, [0 3 2] -2-> 2;
    # -2-> 2, [0 1 4 3] -2-> 4, [0 1 3] -2-> 3
    assert t.tolist() == [[0, 4, 3], [4, 1, 2], [2, 4, 3]] and t.dtype == np.int32
    assert calls == [(0, 4), (0, 3), (0, 2)] * 3
    rng = np.random.default_rng(5)
    for N in (3, 4, 64, 300):
        t = draw_triples(N, 200, lambda lo, hi: int(rng.integers(lo, hi + 1)))
        assert t.min() >= 0 and t.max() < N
        assert (t[:, 0] != t[:, 1]).all() and (t[:, 0] != t[:, 2]).all() and (t[:, 1] != t[:, 2]).all()
    with pytest.raises(ValueError):
        draw_triples(2, 1, lambda lo, hi: 0)


# ---- the Jacobi: sweep count and accuracy ----

def _eig_bits(s, sweeps):
    out = [S.jacobi_eigvec(S.horn_matrix(s["X1"], s["X2"], [int(i) for i in tri])[0], sweeps) for tri in s["triples"]]
    return np.array(out, np.float64).view(np.uint64)


def test_sweep_count():
    """The least number of sweeps after which another sweep changes no bit of any hypothesis'
    eigenvector, over the parity scenes: 5 (measured; the hypotheses that still change at 4 -> 5 are
    printed). The library and the restatement ship that number plus one."""
    need = 0
    for k, fs in SCENES:
        s = S.parity_scene(k, fs)
        prev = _eig_bits(s, 1)
        changed = []
        for j in range(2, S.SWEEPS + 3):
            cur = _eig_bits(s, j)
            changed.append(int((cur != prev).any(1).sum()))
            prev = cur
        print(f"scene {k} fix_scale {fs}: hypotheses that change from j to j + 1 sweeps, j = 1..: {changed}")
        stable = next(j for j in range(1, len(changed) + 1) if not any(changed[j - 1:]))
        need = max(need, stable)
    assert need == S.SWEEPS_NEEDED == 5
    assert S.SWEEPS == S.SWEEPS_NEEDED + 1


def test_accuracy_against_the_literal_closed_form():
    """R, s and t of every non-degenerate hypothesis of the parity scenes against upstream's literal
    form in float64 (np.linalg.eigh, the angle-axis vector, exp), next to the same literal form in
    float32 with LAPACK. Both carry the fp32 M, so the float32 form shows what the input precision
    allows. The bound is on the largest and on the mean error over the hypotheses (a ratio per
    hypothesis says nothing: either form is exact by luck on some): at most twice the float32 form's.
    Measured: R 2.5e-7 / 6.3e-8 (max / mean) against 1.9 / 7.7e-3 (float32 LAPACK picks another
    eigenvector on near-degenerate outlier triples), s 3.2e-7 / 6.9e-8 against 3.7e-7 / 7.1e-8,
    t 1.4e-6 / 1.1e-7 against 4.8 / 9.0e-3."""
    rest, f32, free = [], [], []
    for k, fs in SCENES:
        s = S.parity_scene(k, fs)
        for h, tri in enumerate(s["triples"]):
            if h in s["degenerate_h"]:
                continue
            N, P1, P2, O1, O2 = S.horn_matrix(s["X1"], s["X2"], [int(i) for i in tri])
            R64, s64, t64 = S.literal_sim3(N, P1, P2, O1, O2, fs, np.float64)
            R32, s32, t32 = S.literal_sim3(N, P1, P2, O1, O2, fs, np.float32)
            hy = s["expected"]["hyp"][h].astype(np.float64)

            def err(R, sc, t):
                return (np.abs(np.asarray(R, np.float64) - R64).max(), abs(float(sc) - s64) / abs(s64),
                        np.abs(np.asarray(t, np.float64) - t64).max() / max(1.0, np.abs(t64).max()))
            rest.append(err(hy[1:10].reshape(3, 3), hy[0], hy[10:13]))
            f32.append(err(R32, s32, t32))
            free.append(not fs)
    rest, f32, free = np.array(rest), np.array(f32), np.array(free)
    assert np.isfinite(rest).all() and len(rest) == len(SCENES) * (S.PARITY_H - 2)
    for j, name in enumerate(("R", "s", "t")):
        sel = free if name == "s" else np.ones(len(rest), bool)   # a fixed scale is exactly 1 in both
        a, b = rest[sel, j], f32[sel, j]
        print(f"{name}: restatement max {a.max():.3e} mean {a.mean():.3e}; float32 LAPACK max {b.max():.3e} "
              f"mean {b.mean():.3e}")
        assert a.max() <= 2 * b.max() and a.mean() <= 2 * b.mean()
    assert rest[:, 0].max() < 1e-6   # and a rotation is a rotation to float32's resolution


# ---- the scene set ----

def test_parity_scene_conditions():
    """What the GPU parity test relies on: a scene whose first convergence is at h > 0 with later
    ones behind it, a scene where nothing converges, ties at the largest count, many hypotheses
    without an inlier, and degenerate hypotheses (a planted coincident triple: NaN when the scale is
    free, a finite hypothesis when it is fixed)."""
    nan_hyps = 0
    for k, fs in SCENES:
        s = S.parity_scene(k, fs)
        e = s["expected"]
        n = e["n_inliers"]
        assert len(s["triples"]) == S.PARITY_H and s["X1"].shape == (S.PARITY_CASES[k][0], 3)
        assert 0.5 < (n == 0).mean() < 1.0
        assert s["degenerate_h"] == [1, 150]
        for h in s["degenerate_h"]:
            a, b, c = s["triples"][h]
            assert np.array_equal(s["X1"][a], s["X1"][b]) and np.array_equal(s["X1"][a], s["X1"][c])
            assert np.isfinite(e["hyp"][h]).all() == bool(fs) or not fs
        nan_hyps += int(np.isnan(e["hyp"]).any(1).sum())
        at_max = np.nonzero(n == n.max())[0]
        if k == 0:     # n = 257, 60 % outliers
            assert e["converged"] > 0 and (n > S.PARITY_MIN_INLIERS).sum() >= 10 and len(at_max) >= 2
            assert (n[:e["converged"]] <= S.PARITY_MIN_INLIERS).all()
        elif k == 1:   # n = 100, 85 % outliers
            assert e["converged"] == -1 and n.max() <= 3 and e["best"] == at_max[-1]
        elif k == 2:   # n = 30, 40 % outliers
            assert e["converged"] > 0 and len(at_max) >= 3 and n.max() > S.PARITY_MIN_INLIERS
        else:          # n = 20, 30 % outliers
            assert e["converged"] == -1 and 0 < n.max() < S.PARITY_MIN_INLIERS and len(at_max) >= 2
            assert e["best"] == at_max[-1] and np.array_equal(e["inliers"], e["masks"][at_max[-1]])
    assert nan_hyps >= 4


def test_the_boundary_declares_the_call():
    for name in ("orbhip_sim3_solve", "orbhip_sim3_solve_batch"):
        assert name in _lib.EXPORTED and hasattr(_lib.lib(), name)
    assert _lib.lib().orbhip_abi_version() == 1
