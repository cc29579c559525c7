"""The extraction catalogue (tests/extract_cases.py) on the CPU: every envelope case plans with the
geometry it is listed for, the planner's grid and root counts equal a restatement of the reference's
expressions, every rejected shape is rejected, and the oracle alone reaches the condition each case
is named for. A case that stops reaching its edge fails here, and cannot pass silently in
tests/test_extract_cases_gpu.py, which compares the device with the oracle on the same frames."""
import numpy as np
import pytest

import extract_cases as C


def _oracle_n(oracle, name, kind, seed):
    w, h, nf, sf, L = C.envelope_shape(name)
    img = C.frame(kind, seed, w, h)
    return C.stages(oracle, img, (nf, sf, L, 20, 7))


@pytest.mark.parametrize("name", list(C.ENVELOPE))
def test_envelope_case_plans_with_its_geometry(oracle, name):
    c = C.ENVELOPE[name]
    w, h, nf, sf, L = C.envelope_shape(name)
    p = C.plan(w, h, nf, sf, L)
    assert p is not None, "the planner rejects the shape"
    lv = p["levels"]
    for l, g in c.get("grid", {}).items():
        assert (lv[l]["n_cols"], lv[l]["n_rows"], lv[l]["w_cell"], lv[l]["h_cell"]) == g, (l, lv[l])
    if "n_ini" in c:
        assert [g["n_ini"] for g in lv] == c["n_ini"]
    if "feats" in c:
        assert [g["n_feat"] for g in lv] == c["feats"]
    if "last" in c:
        assert (lv[-1]["w"], lv[-1]["h"]) == c["last"]
    if "cells" in c:
        assert len(p["cells"]) == c["cells"]
    if "window" in c:   # one cell whose window is the whole box plus the 6-px rim, cut at the box: kWinMax
        (_, x0, y0, wc, hc, _), = p["cells"]
        assert (x0, y0, wc, hc) == (16, 16, *c["window"]) and c["window"] == (w - 32, h - 32)
    assert all(g["kp_cap"] == g["n_feat"] + 3 + 4 * g["n_ini"] for g in lv)
    # the planner against the reference's expressions on the oracle's level sizes
    for l, (r, g) in enumerate(zip(C.ref_geometry(oracle, w, h, nf, sf, L), lv)):
        assert {k: g[k] for k in r} == r, (l, r, g)


@pytest.mark.parametrize("name,kind,seed", C.envelope_ids())
def test_envelope_case_is_not_empty_in_the_oracle(oracle, name, kind, seed):
    mono, k, d, cand, kept = _oracle_n(oracle, name, kind, seed)
    assert mono >= 0 and len(k) > 0 and len(d) == len(k) and sum(len(c) for c in kept) == len(k)
    want = C.ENVELOPE[name].get("oracle_n", {}).get(kind)
    assert want is None or len(k) == want


def test_round_step_in_the_root_count(oracle):
    """133x100: box 101 x 68, ratio 1.485 -> one root. 134x100: box 102 x 68, ratio exactly 1.5 ->
    std::round gives two (truncation would give one). On noise both levels hold far more candidates
    than their quota of 100, so the roots decide what is kept: 100 of 594 and 101 of 586."""
    a = C.plan(*C.envelope_shape("133x100"))["levels"][0]
    b = C.plan(*C.envelope_shape("134x100"))["levels"][0]
    assert (a["w"] - 32, a["h"] - 32, b["w"] - 32, b["h"] - 32) == (101, 68, 102, 68)
    assert np.float32(102) / np.float32(68) == np.float32(1.5) and int(np.float32(102) / np.float32(68)) == 1
    assert (a["n_ini"], b["n_ini"]) == (1, 2)
    for name, n_cand, n_kept in (("133x100", 594, 100), ("134x100", 586, 101)):
        _, k, _, cand, kept = _oracle_n(oracle, name, "noise", 5)
        assert (len(cand[0]), len(kept[0])) == (n_cand, n_kept)


def test_strip_lapping_split_inside_the_frame(oracle):
    """2200x100: the oracle keeps exactly 500, and with lap = (0, 1000) the split falls inside the
    frame: monoIndex is neither 0 nor n."""
    mono, k, _, cand, kept = _oracle_n(oracle, "2200x100", "synthetic", 5)
    assert len(k) == 500 and mono == 268 and len(cand[0]) > 500
    assert np.all(k[:mono, 0] > 1000) and np.all(k[mono:, 0] <= 1000)


def test_strip_next_to_the_root_and_box_limits():
    g = C.plan(*C.envelope_shape("4100x99"))["levels"][0]
    assert g["n_ini"] == 61 and 61 <= 64 < 4400 - 32 and g["w"] - 32 == 4068 < 4096
    assert C.plan(*C.rejected_shape("4400x99")) is None   # box 4368 >= 4096, and 65 roots


def test_zero_quota_levels_keep_four_per_root(oracle):
    """nfeatures 1 and 7: levels whose quota is 0 (or 1, 2). DistributeOctTree divides at least once, so
    the oracle keeps 4 keypoints per root whatever the quota: 4 per level at 640x480, 8 at levels 5 to
    7 of 320x240 noise, where nIni is 2. The planner's kp_cap = n_feat + 3 + 4 * nIni holds them."""
    for name in ("nfeat1", "nfeat7"):
        for kind in ("synthetic", "noise"):
            _, k, _, _, kept = _oracle_n(oracle, name, kind, 5)
            assert [len(c) for c in kept] == [4] * 8 and len(k) == 32
    _, _, _, _, kept = _oracle_n(oracle, "nfeat7-320x240", "noise", 5)
    assert [len(c) for c in kept] == [4, 4, 4, 4, 4, 8, 8, 8]
    lv = C.plan(*C.envelope_shape("nfeat7-320x240"))["levels"]
    assert all(len(c) <= g["kp_cap"] for c, g in zip(kept, lv))
    assert [g["kp_cap"] for g in lv] == [9, 8, 8, 8, 8, 12, 12, 11]


def test_n_star_is_the_lds_bound(oracle):
    """N* by bisection: it plans, N* + 1 does not, 5000 does and 20000 does not; at N* the octree's
    LDS is within one node_cap step (64 nodes) of the 160 KB budget. On noise the deepest octree then
    runs at that node_cap: level 0 keeps its whole quota."""
    n = C.n_star()
    w, h, _, sf, L = C.envelope_shape("nstar")
    p = C.plan(w, h, n, sf, L)
    assert 5000 < n < 20000 and p is not None and C.plan(w, h, n + 1, sf, L) is None
    assert p["octree"]["lds"] <= 160 * 1024 and p["octree"]["node_cap"] == -(-max(g["kp_cap"] for g in p["levels"]) // 64) * 64
    _, k, _, cand, kept = _oracle_n(oracle, "nstar", "noise", 5)
    assert len(kept[0]) >= p["levels"][0]["n_feat"] and len(cand[0]) > len(kept[0]) and len(k) > 5000


def test_more_than_eight_levels(oracle):
    for name in ("9levels", "12levels"):
        for kind in ("synthetic", "noise"):
            _, k, _, _, kept = _oracle_n(oracle, name, kind, 5)
            assert all(len(c) > 0 for c in kept) and len(kept) > 8
            assert set(k[:, 5].astype(int)) == set(range(len(kept)))


@pytest.mark.parametrize("name", list(C.REJECTED))
def test_rejected_shape_does_not_plan(name):
    assert C.plan(*C.rejected_shape(name)) is None


def test_every_shape_is_under_the_planner_invariants():
    """tests/cpp/extract_plan_check.cpp's kShapes hold every accepted and rejected shape of the catalogue
    (so its invariant checks and its sanitize target cover them), N* included as kNStar."""
    import os
    import re
    src = open(os.path.join(C.CPP, "extract_plan_check.cpp")).read()
    assert int(re.search(r"constexpr int kNStar = (\d+);", src).group(1)) == C.n_star()
    rows = set()
    for m in re.finditer(r"\{(\d+), (\d+), (\d+), ([0-9.]+)f, (\w+(?: \+ 1)?), (true|false), \d+\}", src):
        nf = {"kNStar": C.n_star(), "kNStar + 1": C.n_star() + 1}.get(m.group(5)) or int(m.group(5))
        rows.add((int(m.group(1)), int(m.group(2)), nf, float(m.group(4)), int(m.group(3)), m.group(6) == "true"))
    for name in C.ENVELOPE:
        assert (*C.envelope_shape(name), True) in rows, name
    for name in C.REJECTED:
        assert (*C.rejected_shape(name), False) in rows, name


@pytest.mark.parametrize("name", list(C.CRAFTED))
def test_crafted_frame_reaches_its_edge(oracle, name):
    make, prm, reach = C.CRAFTED[name]
    reach(oracle, make(), prm)


def test_border_positions_follow_from_the_bounds():
    """cand_span against the closed forms: one 35-px cell spans 3 .. 31, a 208-px box 3 .. 204."""
    assert C.cand_span(67, 67) == ((3, 31), (3, 31))
    assert C.cand_span(240, 240) == ((3, 204), (3, 204))
    assert C.cand_span(320, 240) == ((3, 284), (3, 204))
