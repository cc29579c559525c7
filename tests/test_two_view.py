"""TwoViewReconstruction on the CPU: the conditions under which the GPU test's exact comparison
with tests/two_view_numpy.py means what it should.

  * the restatement's H and F agree with np.linalg.svd solutions up to sign and scale, and its pose
    with the scene's ground truth up to the scale of t, within measured tolerances
  * the fixed Jacobi sweep counts are the measured need + 1
  * the score is exact in fp64, hence the same in any order
  * upstream's literal loop (a running fp32 score) picks the same hypotheses and the same model on
    every scene the GPU test compares
  * no decision of a scene falls within a relative 1e-3 of its threshold
  * draw_sets restates upstream's draw; the Python class validates its arguments
"""
import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import synthetic_two_view_scene
from orb_slam3_ros2_amd.two_view import TwoViewReconstruction, draw_sets

import two_view_cases as C
import two_view_numpy as T

F, D = np.float32, np.float64
NAMED = tuple(C.SCENES) + ("good_le_50",)
SOUND = tuple(n for n in NAMED if not C.SCENES.get(n, {}).get("doubled"))   # sets with a one-dimensional null space for F


def _bits(a):
    return np.asarray(a, F).view(np.uint32)


def _systems(name):
    p = C.scene(name)
    _, _, pn, T1, T2, T2i = T.prepare(p)
    u1, v1, u2, v2 = (q[np.asarray(p["sets"], np.int64)] for q in pn)
    return T.rows_h(u1, v1, u2, v2), T.rows_f(u1, v1, u2, v2)


# ---- accuracy against np.linalg.svd and the ground truth ----

def _align(v, ref):
    """v scaled and signed onto ref (both flattened): the largest deviation relative to |ref|"""
    v, ref = np.asarray(v, D).reshape(-1), np.asarray(ref, D).reshape(-1)
    s = (v @ ref) / (v @ v)
    return np.abs(s * v - ref).max() / np.abs(ref).max()


# measured here over the scene set (printed by the test), against the fp64 SVD of the same fp32
# system: H 3.5e-14, F 2.7e-11 at the worst set whose smallest singular values are separated;
# asserted at 4x
TOL_H, TOL_F = 1.5e-13, 1.1e-10
# measured: the rotation within 0.0152 (largest entry) and the unit translation within 0.0575 of the
# truth at the worst scene (0.3 px of noise on both frames); asserted at 4x
TOL_R, TOL_T = 0.061, 0.23


def test_null_vectors_agree_with_lapack():
    worst_h = worst_f = 0.0
    compared = {"h": 0, "f": 0}
    sampled = 0
    for name in SOUND:
        rh, rf = _systems(name)
        vh = T.null_vector(rh)
        vf = T.null_vector(rf)
        for h in range(0, len(rh), 7):
            sampled += 1
            # against the fp64 SVD of the same fp32 system; only sets whose smallest singular values
            # are separated say anything about a null VECTOR
            for rows, v, kind in ((rh[h], vh[h], "h"), (rf[h], vf[h], "f")):
                sv = np.linalg.svd(rows.astype(D), compute_uv=False)
                gap = sv[7] / sv[0]
                if gap < 1e-3:
                    continue
                e = _align(v, T.svd_null(rows))      # full_matrices: the 8 x 9 system's ninth row of V^T too
                compared[kind] += 1
                if kind == "h":
                    worst_h = max(worst_h, e)
                else:
                    worst_f = max(worst_f, e)
    print(f"null vectors against np.linalg.svd: H {worst_h:.3g} F {worst_f:.3g} over {compared} sets")
    assert min(compared.values()) * 2 >= sampled >= 300      # at least half of the sampled sets say something
    assert worst_h <= TOL_H and worst_f <= TOL_F


def test_svd3_agrees_with_lapack():
    """Q diag(sig) W^T rebuilds M, Q and W are orthogonal, sig equals LAPACK's singular values"""
    rng = np.random.default_rng(3)
    M = rng.normal(size=(200, 3, 3))
    M[::5, :, 2] = M[::5, :, 0] * 0.5 - M[::5, :, 1]          # rank 2, as an essential matrix is
    Q, sig, W, _ = T.svd3(M)
    ref = np.linalg.svd(M, compute_uv=False)
    assert np.abs(sig - ref).max() < 1e-13 * np.abs(ref).max() + 1e-13
    rebuilt = np.einsum("bik,bk,bjk->bij", Q, sig, W)
    assert np.abs(rebuilt - M).max() < 1e-13
    eye = np.eye(3)
    assert np.abs(np.einsum("bki,bkj->bij", Q, Q) - eye).max() < 1e-12
    assert np.abs(np.einsum("bki,bkj->bij", W, W) - eye).max() < 1e-12


@pytest.mark.parametrize("name", ["general", "planar", "mixed", "outliers30", "unmatched"])
def test_pose_agrees_with_the_ground_truth(name):
    p, _, o = T.expected(name)
    assert o["success"] == 1
    eR = np.abs(o["R21"].astype(D) - p["true_R"]).max()
    eT = np.abs(o["t21"].astype(D) - p["true_t"]).max()
    print(f"{name}: |R - R_true| {eR:.3g} |t - t_true| {eT:.3g}")
    assert eR <= TOL_R and eT <= TOL_T
    assert abs(np.linalg.norm(o["t21"].astype(D)) - 1.0) < 1e-6
    good = o["triangulated"]
    assert good.sum() > 50 and (o["p3d"][good][:, 2] > 0).all()


# ---- the Jacobi sweep counts ----

def test_sweep_counts_are_the_measured_need_plus_one():
    """The need: the fewest sweeps after which the fp32 result is the one 20 sweeps give, over every
    set of the scene set with a one-dimensional null space (a doubled set leaves the fundamental
    matrix five null directions: whatever vector the fixed procedure yields is as good as another)."""
    need9 = need3 = 0
    for name in NAMED:
        rh, rf = _systems(name)
        for rows in ((rh, rf) if name in SOUND else (rh,)):
            ref = _bits(T.null_vector(rows, 20))
            need9 = max(need9, next(s for s in range(1, 20) if (_bits(T.null_vector(rows, s)) == ref).all()))
        if name in SOUND:
            Fpre = T.null_vector(rf).astype(F).astype(D).reshape(-1, 3, 3)
            mats = [Fpre]
            o = T.expected(name)[2]
            K = C.scene(name)["K"]
            Km = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], F)
            mats.append(T.mm3(T.mm3(Km.T.copy(), o["F21"]), Km).T.astype(D)[None])
            for M in mats:
                def out(s):
                    Q, sig, W, Cs = T.svd3(M, s)
                    return np.concatenate([_bits(Q).ravel(), _bits(sig).ravel(), _bits(W).ravel(),
                                           _bits(Cs[:, :, 0, None] * W[:, None, :, 0] + Cs[:, :, 1, None] * W[:, None, :, 1]).ravel()])
                ref = out(20)
                need3 = max(need3, next(s for s in range(1, 20) if (out(s) == ref).all()))
    print(f"measured need: 9x9 {need9} sweeps, 3x3 {need3} sweeps")
    assert (need9, need3) == (T.SWEEPS9_NEEDED, T.SWEEPS3_NEEDED)
    assert (T.SWEEPS9, T.SWEEPS3) == (need9 + 1, need3 + 1)


# ---- the score ----

@pytest.mark.parametrize("name", NAMED)
def test_score_is_exact_and_order_free(name):
    """Every term is a multiple of 2^-22 below 6, so the fp64 sum of at most 2 x 8192 of them is
    exact: the same under random permutations, under a pairwise tree and as an integer sum"""
    p, r, _ = T.expected(name)
    pts = r["pts"]
    isg = T.inv_sigma2_of(p["sigma"])
    rng = np.random.default_rng(11)
    for h in range(0, len(p["sets"]), 9):
        H21 = r["H21"][h]
        for terms in (T.homography_terms(H21, T.inv3(H21), pts, isg)[0], T.fundamental_terms(r["F21"][h], pts, isg)[0]):
            t = terms.reshape(-1).astype(D)
            if np.isnan(t).any():
                continue
            assert (t >= 0).all() and (t < 6).all() and (t * 2.0 ** 22 == np.round(t * 2.0 ** 22)).all()
            exact = int(np.round(t * 2.0 ** 22).astype(np.int64).sum())
            want = T.score_of(terms)
            assert want == F(exact / 2.0 ** 22)
            for _ in range(3):
                q = rng.permutation(t)
                seq = 0.0
                for x in q:
                    seq += x
                assert F(seq) == want
                tree = q.copy()
                while len(tree) > 1:
                    if len(tree) % 2:
                        tree = np.append(tree, 0.0)
                    tree = tree[0::2] + tree[1::2]
                assert F(tree[0]) == want


def _gpu_scenes():
    """every problem tests/test_two_view_gpu.py compares with the restatement, by the name it prints
    (the problem of its argument-error test is compared only with its own earlier result)"""
    out = [(n, C.scene(n)) for n in NAMED]
    out += [(f"n={n}", C.sized(n, 12, seed=n)) for n in (8, 9, 63, 64, 65, 128, 129)]
    out += [(f"H={H}", C.sized(70, H, seed=H)) for H in (1, 2, 63, 64, 65, 200)]
    out += [(f"problem {b}", C.batch_problem(b)) for b in range(64)]       # B = 1, 2, 3 are its first problems
    out += list(C.degenerate_problems().items())
    return out


GPU_SCENES = _gpu_scenes()


@pytest.mark.parametrize("what,p", GPU_SCENES, ids=[w for w, _ in GPU_SCENES])
def test_literal_loop_picks_the_same(what, p):
    """upstream's sequential fp32 sum picks the same best hypothesis for H and for F and the same
    side of RH > 0.50 as the order-free score"""
    a, b = T.ransac(p), T.ransac(p, literal=True)
    ha, hb = T.select_first_max(a["scoreH"]), T.select_first_max(b["scoreH"])
    fa, fb = T.select_first_max(a["scoreF"]), T.select_first_max(b["scoreF"])
    assert ha[0] == hb[0] and fa[0] == fb[0], (what, ha, hb, fa, fb)
    with np.errstate(all="ignore"):
        assert (ha[1] / (ha[1] + fa[1]) > F(0.5)) == (hb[1] / (hb[1] + fb[1]) > F(0.5))


# ---- the decisions ----

def _margins(o):
    """(what, value, threshold) of every comparison the result o went through (none after SH + SF ==
    0; no count comparison where no point was counted)"""
    if o["model"] == -1:
        return []
    out = [("RH", float(o["RH"]), 0.5)]
    g = [int(x) for x in o["n_good"]]
    if o["model"] == 1:
        mx = max(g[:4])
        out.append(("maxGood vs nMinGood", mx, max(int(0.9 * o["n_inl"]), 50)))
        out += [(f"nGood{i} vs 0.7 maxGood", g[i], 0.7 * mx) for i in range(4) if mx > 0]
        k = g[:4].index(mx)
        if mx > 0:
            out.append(("parallax", float(o["parallax"][k]), 1.0))
    elif o["model"] == 0:
        d1, d2, d3 = (float(x) for x in o["d"])
        out += [("d1/d2", d1 / d2, 1.00001), ("d2/d3", d2 / d3, 1.00001)]
        if o["n_mot"] and max(g) > 0:
            srt = sorted(g, reverse=True)
            k = g.index(srt[0])
            out += [("secondBest vs 0.75 best", srt[1], 0.75 * srt[0]), ("best vs minTriangulated", srt[0], 50),
                    ("best vs 0.9 N", srt[0], 0.9 * o["n_inl"]), ("parallax", float(o["parallax"][k]), 1.0)]
    return out


# The problems that sit at a threshold, each comparison named. good_le_50: maxGood == nMinGood == 50, a
# comparison of two integers, exact by construction. exit_d_ratio: d1/d2 < 1.00001 needs a ratio
# within 1e-5 of 1, which no scene can hold a relative 1e-3 away from 1.00001; its margin is asserted
# on the scale of the gap instead (test_the_scenes_built_on_a_threshold).
AT_THRESHOLD = {"good_le_50": ("maxGood vs nMinGood",), "exit_d_ratio": ("d1/d2", "d2/d3")}


@pytest.mark.parametrize("what,p", GPU_SCENES, ids=[w for w, _ in GPU_SCENES])
def test_no_decision_sits_on_its_threshold(what, p):
    """every problem the GPU test compares, the size-edge, batch and degenerate ones included"""
    o = T.expected(what)[2] if what in NAMED else T.reconstruct(p)
    for name, v, th in _margins(o):
        if name in AT_THRESHOLD.get(what, ()):
            continue
        assert abs(v - th) > 1e-3 * abs(th), (what, name, v, th)


def test_the_scenes_built_on_a_threshold():
    o = T.expected("good_le_50")[2]
    assert o["n_good"].max() == 50 == max(int(0.9 * o["n_inl"]), 50) and o["n_good"].dtype == np.int32
    d1, d2, _ = T.expected("exit_d_ratio")[2]["d"]
    assert 0.0 <= float(d1) / float(d2) - 1.0 < 1e-6


def test_a_reprojection_error_exactly_at_th2():
    """th2 = 4 fl(sigma sigma) is an input: th2_at carries the sigma that puts it on the fp32 error of
    one match under the accepted hypothesis, bit for bit, where `error > th2` is false and the match
    is counted; th2_above the next sigma below, where it is true. Neither sigma moves a selected
    hypothesis, the model, the chosen motion or the match's error."""
    base, at, above = (T.expected(n)[2] for n in ("unmatched", "th2_at", "th2_above"))
    m, img, i = C.TH2_MATCH["hypothesis"], C.TH2_MATCH["image"], C.TH2_MATCH["match"]
    s_at, s_above = F(C.scene("th2_at")["sigma"]), F(C.scene("th2_above")["sigma"])
    assert s_above == np.nextafter(s_at, F(0))
    for o in (at, above):
        assert all(o[k] == base[k] for k in ("best_h", "best_f", "model", "chosen")) and o["chosen"] == m
    e = base["checks"][m][img][i]
    assert _bits(at["checks"][m][img][i]) == _bits(e) == _bits(above["checks"][m][img][i])
    assert _bits(F(4) * (s_at * s_at)) == _bits(e) and F(4) * (s_above * s_above) < e
    assert at["checks"][m]["good"][i] and not above["checks"][m]["good"][i]
    assert at["n_good"][m] == above["n_good"][m] + 1
    other = "err1" if img == "err2" else "err2"             # the error test alone decides
    assert at["checks"][m][other][i] < F(4) * (s_above * s_above)


def test_every_set_degenerate():
    """Every set drawn from eight coincident matches among distinct ones: all hypotheses come from
    null spaces of several dimensions. The issue expected SH + SF == 0 of it; the Jacobi's finite
    vectors give a homography that maps the one point onto itself (those eight matches are its
    inliers) and the call fails later, in ReconstructH. The literal solver gives the same."""
    p = C.degenerate_problems()["all_sets_degenerate"]
    o, lit = T.reconstruct(p), T.LiteralSolver(p).Reconstruct()[4]
    assert o["success"] == 0 and lit["success"] == 0
    assert (o["best_h"], o["best_f"], o["model"], o["chosen"]) == (lit["best_h"], lit["best_f"], lit["model"], lit["chosen"])
    print("every set degenerate: SH", o["SH"], "SF", o["SF"], "model", o["model"], "n_good", o["n_good"])


def test_scenes_reach_what_they_are_built_for():
    e = {n: T.expected(n)[2] for n in NAMED}
    assert [e[n]["model"] for n in C.PARITY] == [1, 0, 1, 1, 1, 1, 1]
    assert [e[n]["success"] for n in C.PARITY] == [1, 1, 1, 0, 0, 1, 1]
    o = e["exit_d_ratio"]
    assert o["model"] == 0 and o["n_mot"] == 0 and (o["d"][0] / o["d"][1] < F(1.00001) or o["d"][1] / o["d"][2] < F(1.00001))
    o = e["exit_nsimilar"]
    g = o["n_good"][:4]
    assert o["model"] == 1 and (g > 0.7 * g.max()).sum() > 1 and g.max() >= max(int(0.9 * o["n_inl"]), 50)
    o = e["exit_min_good"]
    g = o["n_good"][:4]
    assert o["model"] == 1 and (g > 0.7 * g.max()).sum() == 1 and g.max() < max(int(0.9 * o["n_inl"]), 50)
    o = e["exit_second_best"]
    g = np.sort(o["n_good"])[::-1]
    assert o["model"] == 0 and o["n_mot"] == 8 and g[1] >= 0.75 * g[0] and g[0] > 50 and g[0] > 0.9 * o["n_inl"]
    o = e["exit_min_triangulated"]
    g = np.sort(o["n_good"])[::-1]
    assert o["model"] == 0 and o["n_mot"] == 8 and g[0] <= 50 and g[1] < 0.75 * g[0]
    # rotation and low parallax fail with two equal hypotheses, below the minimum parallax either way
    for n in ("rotation", "low_parallax"):
        assert e[n]["chosen"] == -1 and e[n]["parallax"].max() < 1.0
    # both arms of min(50, size - 1)
    assert e["good_le_50"]["n_good"].max() <= 50 and e["good_51"]["n_good"].max() == 51 and e["good_many"]["n_good"].max() > 51
    assert all(e[n]["success"] == 1 for n in ("good_le_50", "good_51", "good_many"))


def test_check_rt_meets_points_behind_a_camera_on_both_sides_of_the_cosine_limit():
    """Over the motion hypotheses of the scene set CheckRT sees a point with negative depth and a
    cosine below 0.99998 (skipped) and one with a cosine at or above it (kept)"""
    skipped = kept = 0
    for name in ("general", "rotation", "planar"):
        p, r, o = T.expected(name)
        K = np.asarray(p["K"], F)
        mots = T.motions_h(o["H21"], K)[0] if o["model"] == 0 else T.motions_f(o["F21"], K)
        inl = o["inl_h"] if o["model"] == 0 else o["inl_f"]
        for R, t in mots:
            c = T.check_rt(R, t, r["pts"], inl, K, F(4))
            z1 = c["p3d"][:, 2]
            z2 = T.mv3(R, c["p3d"])[:, 2] + t[2]
            behind = inl & np.isfinite(z1) & ((z1 <= 0) | (z2 <= 0))
            skipped += int((behind & (c["cos"] < T.COS_LIMIT)).sum())
            kept += int((behind & ~(c["cos"] < T.COS_LIMIT) & c["good"]).sum())
    assert skipped > 0 and kept > 0


def test_kth_smallest_needs_no_order():
    rng = np.random.default_rng(2)
    c = rng.integers(0, 30, 200).astype(F) / F(32)       # many ties
    for k in (0, 1, 50, 199):
        assert T.kth_smallest(c, k) == np.sort(c)[k] == T.kth_smallest(rng.permutation(c), k)


# ---- draw_sets and the Python class ----

def test_draw_sets_restates_upstream():
    for N, H, seed in ((8, 5, 1), (9, 40, 2), (300, 200, 3)):
        a, b = np.random.default_rng(seed), np.random.default_rng(seed)
        got = draw_sets(N, H, lambda lo, hi: int(a.integers(lo, hi + 1)))
        want = T.literal_draw_sets(N, H, lambda lo, hi: int(b.integers(lo, hi + 1)))
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert all(len(set(row)) == 8 for row in got.tolist()) and got.min() >= 0 and got.max() < N
    calls = []
    draw_sets(10, 1, lambda lo, hi: calls.append((lo, hi)) or 0)
    assert calls == [(0, 9 - k) for k in range(8)]
    with pytest.raises(ValueError):
        draw_sets(7, 1, lambda lo, hi: 0)


def test_python_class_validates_its_arguments():
    p = synthetic_two_view_scene("general", n=30, seed=1, n_hyp=6, unmatched_frac=0.2)
    K = p["K"]
    for bad in ([0, 500, 320, 240], [500, -1, 320, 240], [np.nan, 500, 320, 240], [500, np.inf, 320, 240], [1, 2, 3]):
        with pytest.raises(ValueError):
            TwoViewReconstruction(bad)
    for sigma in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            TwoViewReconstruction(K, sigma)
    for its in (0, 4097):
        with pytest.raises(ValueError):
            TwoViewReconstruction(K, 1.0, its)
    assert np.array_equal(TwoViewReconstruction(np.array([[500, 0, 320], [0, 510, 240], [0, 0, 1]])).K,
                          np.array([500, 510, 320, 240], F))
    tv = TwoViewReconstruction(K, 1.0, 6)
    k1, k2, m, s = p["kps1"], p["kps2"], p["matches12"], p["sets"]

    def refused(*a):
        with pytest.raises(ValueError):
            tv._problem(*a)          # raised before any device call
    refused(k1, k2, m[:-1], s)
    refused(k1, k2, np.where(m >= 0, len(k2), m), s)
    refused(k1, k2, np.where(m >= 0, -2, m), s)
    few = m.copy()
    few[np.nonzero(few >= 0)[0][7:]] = -1
    refused(k1, k2, few, s)
    refused(k1, k2, m, s[:5])
    for h, k, v in ((0, 0, 30), (2, 3, -1), (4, 7, int(s[4, 0]))):
        t = s.copy()
        t[h, k] = v
        refused(k1, k2, m, t)
    refused(k1[:, :1], k2, m, s)
    assert tv._problem(k1, k2, m, s)[4] == 30
    with pytest.raises(ValueError):
        TwoViewReconstruction.reconstruct_batch([tv], [])
    assert TwoViewReconstruction.reconstruct_batch([], []) == []
