"""The extraction catalogue (tests/test_extract_cases*.py): frames at the edges of the planner's
envelope and crafted frames that reach one edge of ORBextractor each, with the condition every
case must reach stated on the oracle (oracle/) or on the planner (tests/cpp/extract_plan_check's
"plan" mode), never on the device.

ENVELOPE maps a name to (w, h, nfeatures, scaleFactor, nlevels), the frame kinds it runs on and
"geom": what the planner must give for it, checked on the CPU both against the planner and against
ref_geometry, a restatement of ComputeKeyPointsOctTree's cell grid and DistributeOctTree's root
count from the oracle's level sizes. REJECTED lists shapes that must return
ORBHIP_ERR_UNSUPPORTED. CRAFTED maps a name to a frame builder, its ORB parameters and "reach":
a function of the oracle's stages that raises unless the frame reaches the edge it is named for.

Coordinates. The oracle's candidates (orc_extract_levels, as vToDistributeKeys in the reference)
are relative to the border box, whose origin is (16, 16) of the level: FAST does not detect in the
3-px rim of a cell window, so x runs from 3 to box_w - 4 and y from 3 to box_h - 4 (cand_span).
Its kept keypoints are in level pixels.
"""
import os
import subprocess
from functools import lru_cache

import numpy as np

from helpers import c_round
from orb_slam3_ros2_amd.synthetic import synthetic_frame

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PLAN_EXE = os.path.join(CPP, "build", "extract_plan_check")
UNSUPPORTED = -5
EDGE = 16          # EDGE_THRESHOLD - 3: the border box starts here and ends EDGE short of the level
CELL = 35          # ComputeKeyPointsOctTree's W
CAND_PRIM = 16     # kCandPrim: a cell's first candidates sit in its primary slots, the rest in its slot range


# ---- the planner, as a program ----

@lru_cache(maxsize=None)
def plan(w, h, nfeatures, scale, nlevels):
    """plan_build_host at the default switches -> None when it returns ORBHIP_ERR_UNSUPPORTED, else
    {"levels": [dict(w, h, n_cols, n_rows, w_cell, h_cell, n_cells, n_ini, n_feat, kp_cap)],
     "cells": [(level, x0, y0, wc, hc, slots)], "octree": dict(node_cap, sort_cap, key_cap, lds)}."""
    if not os.path.exists(PLAN_EXE):
        subprocess.check_call(["make", "-s", "-C", CPP, "build/extract_plan_check"])
    r = subprocess.run([PLAN_EXE, "plan", str(w), str(h), str(nlevels), repr(float(scale)), str(nfeatures)],
                       capture_output=True, text=True, timeout=120)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[0].startswith("plan "), r.stdout[-400:] + r.stderr[-400:]
    rc = int(lines[0].split()[1])
    if rc != 0:
        assert rc == UNSUPPORTED, lines[0]
        return None
    out = {"levels": [], "cells": [], "octree": None}
    keys = ("w", "h", "n_cols", "n_rows", "w_cell", "h_cell", "n_cells", "n_ini", "n_feat", "kp_cap")
    for ln in lines[1:]:
        t = ln.split()
        if t[0] == "level":
            out["levels"].append(dict(zip(keys, map(int, t[2:]))))
        elif t[0] == "cell":
            out["cells"].append(tuple(map(int, t[1:])))
        elif t[0] == "octree":
            out["octree"] = dict(zip(("node_cap", "sort_cap", "key_cap", "lds"), map(int, t[1:])))
    assert len(out["levels"]) == nlevels and out["octree"] is not None
    return out


@lru_cache(maxsize=None)
def n_star(w=320, h=240, scale=1.2, nlevels=8, lo=5000, hi=20000):
    """The largest nfeatures that plans at this size, by bisection over the planner program (it plans
    at lo and not at hi; k_octree's 160 KB of LDS is what bounds it)."""
    assert plan(w, h, lo, scale, nlevels) is not None and plan(w, h, hi, scale, nlevels) is None
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if plan(w, h, mid, scale, nlevels) is not None:
            lo = mid
        else:
            hi = mid
    return lo


def ref_geometry(oracle, w, h, nfeatures, scale, nlevels):
    """ComputeKeyPointsOctTree's grid and DistributeOctTree's nIni per level, restated from the
    reference's expressions on the oracle's level sizes (float32 where the reference has float)."""
    f32 = np.float32
    info = oracle.level_info(w, h, nfeatures, scale, nlevels)
    out = []
    for l in range(nlevels):
        lw, lh = int(info["w"][l]), int(info["h"][l])
        bw, bh = lw - 2 * EDGE, lh - 2 * EDGE
        n_cols, n_rows = int(f32(bw) / f32(CELL)), int(f32(bh) / f32(CELL))
        g = dict(w=lw, h=lh, n_cols=n_cols, n_rows=n_rows, n_feat=int(info["feats"][l]))
        if n_cols > 0 and n_rows > 0:
            g["w_cell"] = int(np.ceil(f32(bw) / f32(n_cols)))
            g["h_cell"] = int(np.ceil(f32(bh) / f32(n_rows)))
            g["n_ini"] = c_round(f32(bw) / f32(bh))
        out.append(g)
    return out


def cand_span(lw, lh):
    """((x_min, x_max), (y_min, y_max)) a candidate of a lw x lh level can have, relative to the border
    box, from ComputeKeyPointsOctTree's bounds: the cells' windows [ini, min(ini + cell + 6, maxBorder))
    cover the box, FAST detects 3 px inside a window, and a column (row) of cells whose origin lies
    within 6 (3) px of the box's end is skipped."""
    def axis(n, skip):
        box = n - 2 * EDGE
        cells = int(np.float32(box) / np.float32(CELL))
        size = int(np.ceil(np.float32(box) / np.float32(cells)))
        hi = None
        for i in range(cells):
            ini = i * size
            if ini >= box - skip:
                continue
            hi = min(ini + size + 6, box) - 3 - 1
        return 3, hi
    return axis(lw, 6), axis(lh, 3)


# ---- frames ----

def noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def frame(kind, seed, w, h):
    return synthetic_frame(seed, w, h) if kind == "synthetic" else noise(seed, w, h)


# name -> (w, h, nfeatures, scaleFactor, nlevels), frames as (kind, seed), and the planner's geometry:
# "grid" = level -> (n_cols, n_rows, w_cell, h_cell), "n_ini" / "feats" / "last" = per-level lists or
# the last level's (w, h); "oracle_n" = kind -> the keypoints the oracle finds (pinned from the oracle)
BOTH = (("synthetic", 5), ("noise", 5))
ENVELOPE = {
    "67x67": dict(shape=(67, 67, 100, 1.2, 1), frames=BOTH, grid={0: (1, 1, 35, 35)}, n_ini=[1], cells=1,
                  oracle_n={"synthetic": 9}),
    "101x101": dict(shape=(101, 101, 200, 1.2, 1), frames=BOTH, grid={0: (1, 1, 69, 69)}, n_ini=[1], cells=1,
                    window=(69, 69)),
    "102x102": dict(shape=(102, 102, 200, 1.2, 1), frames=BOTH, grid={0: (2, 2, 35, 35)}, n_ini=[1], cells=4),
    "136x101": dict(shape=(136, 101, 200, 1.2, 1), frames=BOTH, grid={0: (2, 1, 52, 69)}, n_ini=[2], cells=2),
    "133x100": dict(shape=(133, 100, 100, 1.2, 1), frames=BOTH, grid={0: (2, 1, 51, 68)}, n_ini=[1], cells=2),
    "134x100": dict(shape=(134, 100, 100, 1.2, 1), frames=BOTH, grid={0: (2, 1, 51, 68)}, n_ini=[2], cells=2),
    "240x240": dict(shape=(240, 240, 1000, 1.2, 8), frames=BOTH, grid={0: (5, 5, 42, 42), 7: (1, 1, 35, 35)},
                    n_ini=[1] * 8, last=(67, 67)),
    "1000x100": dict(shape=(1000, 100, 500, 1.2, 2), frames=BOTH, grid={0: (27, 1, 36, 68), 1: (22, 1, 37, 51)},
                     n_ini=[14, 16]),
    "2200x100": dict(shape=(2200, 100, 500, 1.2, 1), frames=BOTH, grid={0: (61, 1, 36, 68)}, n_ini=[32], cells=61),
    "4100x99": dict(shape=(4100, 99, 500, 1.2, 1), frames=BOTH, grid={0: (116, 1, 36, 67)}, n_ini=[61], cells=116),
    "nfeat1": dict(shape=(640, 480, 1, 1.2, 8), frames=BOTH, feats=[0, 0, 0, 0, 0, 0, 0, 1], n_ini=[1] * 8),
    "nfeat7": dict(shape=(640, 480, 7, 1.2, 8), frames=BOTH, feats=[2, 1, 1, 1, 1, 1, 1, 0], n_ini=[1] * 8),
    "nfeat7-320x240": dict(shape=(320, 240, 7, 1.2, 8), frames=(("noise", 5),), feats=[2, 1, 1, 1, 1, 1, 1, 0],
                           n_ini=[1, 1, 1, 1, 1, 2, 2, 2]),
    "nstar": dict(shape=(320, 240, None, 1.2, 8), frames=BOTH, n_ini=[1, 1, 1, 1, 1, 2, 2, 2], last=(89, 67)),
    "9levels": dict(shape=(640, 480, 1000, 1.2, 9), frames=BOTH, last=(149, 112)),
    "12levels": dict(shape=(640, 480, 1000, 1.1, 12), frames=BOTH, last=(224, 168)),
    "1920x1080": dict(shape=(1920, 1080, 2000, 1.2, 8), frames=(("synthetic", 5),), grid={0: (53, 29, 36, 37)},
                      n_ini=[2] * 8),
}
# the multi-level cases of at most 1000 px: also run under each batch pyramid engine
PYRAMID_ENGINE_CASES = ["240x240", "1000x100", "nfeat1", "nfeat7", "nfeat7-320x240", "nstar", "9levels", "12levels"]
# one cell as large as a cell gets: also run under every k_fast_cells variant and the sweep octree
BIG_CELL_CASES = ["101x101", "136x101", "240x240"]

# (w, h, nfeatures, scaleFactor, nlevels) -> ORBHIP_ERR_UNSUPPORTED; None = n_star() + 1
REJECTED = {
    "66x67": (66, 67, 100, 1.2, 1), "67x66": (67, 66, 100, 1.2, 1), "100x1000": (100, 1000, 100, 1.2, 1),
    "4400x99": (4400, 99, 500, 1.2, 1), "nstar+1": (320, 240, None, 1.2, 8), "20000": (320, 240, 20000, 1.2, 8),
    "scale2": (320, 240, 1000, 2.0, 2),
}


def envelope_shape(name):
    w, h, nf, sf, L = ENVELOPE[name]["shape"]
    return w, h, (n_star() if nf is None else nf), sf, L


def rejected_shape(name):
    w, h, nf, sf, L = REJECTED[name]
    return w, h, (n_star() + 1 if nf is None else nf), sf, L


def envelope_ids():
    return [(n, kind, seed) for n, c in ENVELOPE.items() for kind, seed in c["frames"]]


# ---- crafted frames ----

def dots(bg, fg, w=320, h=240):
    """A flat frame with single-pixel dots on a 29 x 23 lattice: each dot is a FAST corner of response
    |fg - bg| - 1 whose 16 circle pixels all differ from it by |fg - bg|, and an exactly symmetric patch."""
    img = np.full((h, w), bg, np.uint8)
    img[8::23, 8::29] = fg
    return img


def dots_halves(bg, left, right, split=160, w=320, h=240):
    """dots with contrast `left` in the columns below `split` and `right` from there on."""
    img = np.full((h, w), bg, np.uint8)
    ys, xs = np.arange(8, h, 23), np.arange(8, w, 29)
    for x in xs:
        img[ys, x] = bg + (left if x < split else right)
    return img


SPLIT_21_20 = 110   # dot columns 37, 66, 95 at contrast 21; 124 ... 298 at contrast 20


DENSE_CELL = (0, 0)   # the cell (column, row) of level 0 the checkerboard fills


def lattice_cell(w=320, h=240):
    """A flat frame whose level-0 cell (0, 0) window (42 x 48 at 320x240) holds single pixels of random
    height 1..255 on every second column and row of a black ground. The 3x3 non-maximum suppression
    admits at most every second pixel of each axis (the cell's slot bound, 378 here); a 2-px
    checkerboard, the obvious candidate, has NO corners (no 9 contiguous circle pixels on one side),
    equal heights on this lattice have none either (the circle's four diagonal pixels are lattice
    points), uniform noise reaches 113 and a 4-px lattice of equal dots 72. This lattice reaches 131
    candidates that only this cell can have produced, 35% of the slot bound and 8 times kCandPrim.
    The rest of the frame carries the dot lattice: with the patch alone, DistributeOctTree's first
    split leaves one non-empty child, the node count does not grow, and it stops at one keypoint."""
    img = dots(128, 255, w, h)
    patch = np.zeros((48, 42), np.uint8)
    patch[::2, ::2] = np.random.default_rng(10).integers(1, 256, patch[::2, ::2].shape)
    img[EDGE:EDGE + 48, EDGE:EDGE + 42] = patch
    return img


def stages(oracle, img, prm):
    """The oracle's stages of one frame: (mono, keypoints [n, 6], descriptors, cand per level, kept per level)."""
    nf, sf, L, ini, mn = prm
    mono, k, d = oracle.extract(img, nf, sf, L, ini, mn, (0, 1000))
    cand, kept = oracle.extract_levels(img, nf, sf, L, ini, mn)
    return mono, k, d, cand, kept


def _one_response(cand0):
    assert len(cand0) > 0 and len(np.unique(cand0[:, 4])) == 1, np.unique(cand0[:, 4])


def reach_ties_all_kept(oracle, img, prm):
    _, k, _, cand, kept = stages(oracle, img, prm)
    _one_response(cand[0])
    assert len(cand[0]) == 90 and len(kept[0]) == 90
    # exactly symmetric patches: fastAtan2(0, 0) = 0 at level 0, and the lattice's images on the
    # scaled levels reach the other three exact angles
    for a in (0.0, 90.0, 180.0, 270.0):
        assert np.count_nonzero(k[:, 3] == np.float32(a)) > 0, a
    assert np.count_nonzero(k[:, 3] == 0.0) >= 90


def reach_ties_quota(oracle, img, prm):
    _, _, _, cand, kept = stages(oracle, img, prm)
    _one_response(cand[0])
    quota = int(oracle.level_info(img.shape[1], img.shape[0], prm[0], prm[1], prm[2])["feats"][0])
    assert quota == 22 and len(cand[0]) == 90 and quota <= len(kept[0]) < len(cand[0])


def reach_saturation(n):
    def f(oracle, img, prm):
        _, k, _, cand, _ = stages(oracle, img, prm)
        _one_response(cand[0])
        assert cand[0][0, 4] == 254.0 and len(k) == n, len(k)
    return f


def _halves(cand0, split):
    """level-0 candidates left / right of frame column `split` (box coordinates + EDGE = frame x): the
    two sets are disjoint by x by construction of the mask."""
    x = cand0[:, 0] + EDGE
    return cand0[x < split], cand0[x >= split]


def reach_strict_ini(oracle, img, prm):
    """The lattice has 10 x 9 dots inside the border box. (20, 7): the 27 dots of contrast 21 pass
    iniThFAST (21 > 20); 54 dots of contrast 20 exist only through the minThFAST fallback of cells
    that hold no contrast-21 dot. The 9 contrast-20 dots of column 124 share their cells with column
    95 (contrast 21): those cells found a corner at 20, take no fallback, and the dots are lost: 81
    keypoints, not 90. (20, 20): the fallback threshold is 20 as well, 20 > 20 fails, 27 are left."""
    nf, sf, L, _, _ = prm
    _, k, _, cand, _ = stages(oracle, img, (nf, sf, L, 20, 7))
    left, right = _halves(cand[0], SPLIT_21_20)
    assert len(k) == 81 and len(left) == 27 and len(right) == 54
    assert set(left[:, 4]) == {20.0} and set(right[:, 4]) == {19.0}
    assert 124 not in set(right[:, 0] + EDGE) and {153.0, 298.0} <= set(right[:, 0] + EDGE)
    _, k20, _, cand20, _ = stages(oracle, img, (nf, sf, L, 20, 20))
    left, right = _halves(cand20[0], SPLIT_21_20)
    assert len(k20) == 27 and len(left) == 27 and len(right) == 0


def reach_strict_min(oracle, img, prm):
    """contrast 8 | 7 under (20, 7): nothing passes 20, the fallback finds contrast 8 > 7 and not 7 > 7;
    every blurred comparison of a descriptor ties, so all 45 descriptors are zero."""
    _, k, d, cand, _ = stages(oracle, img, prm)
    left, right = _halves(cand[0], img.shape[1] // 2)
    assert len(k) == 45 and len(left) == 45 and len(right) == 0 and set(left[:, 4]) == {7.0}
    assert np.all(k[:, 0] < img.shape[1] // 2)
    assert d.shape == (45, 32) and not d.any()


def reach_nothing(oracle, img, prm):
    mono, k, _, cand, kept = stages(oracle, img, prm)
    assert mono == 0 and len(k) == 0 and all(len(c) == 0 for c in cand) and all(len(c) == 0 for c in kept)


def reach_border(oracle, img, prm):
    _, k, _, cand, _ = stages(oracle, img, prm)
    (x0, x1), (y0, y1) = cand_span(img.shape[1], img.shape[0])
    c = cand[0]
    assert (c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max()) == (x0, x1, y0, y1), \
        (c[:, 0].min(), c[:, 0].max(), c[:, 1].min(), c[:, 1].max(), x0, x1, y0, y1)
    assert len(k) > 0


def dense_cell_counts(oracle, img, prm):
    """(candidates of level 0 inside the checkerboard cell's own columns and rows, the cell's slot bound)."""
    w, h = img.shape[1], img.shape[0]
    p = plan(w, h, prm[0], prm[1], prm[2])
    g = p["levels"][0]
    ci = DENSE_CELL[1] * g["n_cols"] + DENSE_CELL[0]
    _, x0, y0, wc, hc, slots = p["cells"][ci]
    assert slots == ((wc - 5) // 2) * ((hc - 5) // 2)
    _, _, _, cand, kept = stages(oracle, img, prm)
    assert len(kept[0]) > 100
    c = cand[0]
    # a cell's own detections: FAST positions 3 .. wc - 4 of its window, in box coordinates
    bx, by = x0 - EDGE, y0 - EDGE
    own = (c[:, 0] >= bx + 3) & (c[:, 0] <= bx + wc - 4) & (c[:, 1] >= by + 3) & (c[:, 1] <= by + hc - 4)
    # the neighbours' windows overlap this one by 6 px; count only what no neighbour can have produced
    excl = own & (c[:, 0] < bx + g["w_cell"] + 3 - 6) & (c[:, 1] < by + g["h_cell"] + 3 - 6)
    return int(np.count_nonzero(excl)), slots


def reach_dense(oracle, img, prm):
    n, slots = dense_cell_counts(oracle, img, prm)
    assert (n, slots) == (131, 378) and n > CAND_PRIM, (n, slots)


ORB8 = (1000, 1.2, 8, 20, 7)
ORB1 = (1000, 1.2, 1, 20, 7)
# name -> (frame builder, (nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST), reach)
CRAFTED = {
    "ties-1000": (lambda: dots(100, 255), ORB8, reach_ties_all_kept),
    "ties-100": (lambda: dots(100, 255), (100, 1.2, 8, 20, 7), reach_ties_quota),
    "saturated-white": (lambda: dots(0, 255), ORB8, reach_saturation(382)),
    "saturated-black": (lambda: dots(255, 0), ORB8, reach_saturation(399)),
    "contrast-21|20": (lambda: dots_halves(100, 21, 20, SPLIT_21_20), ORB1, reach_strict_ini),
    "contrast-21|20-min20": (lambda: dots_halves(100, 21, 20, SPLIT_21_20), (1000, 1.2, 1, 20, 20), reach_strict_ini),
    "contrast-8|7": (lambda: dots_halves(100, 8, 7), ORB1, reach_strict_min),
    "contrast-7": (lambda: dots_halves(100, 7, 7), ORB1, reach_nothing),
    "border-67x67": (lambda: noise(BORDER_SEEDS[67], 67, 67), (100, 1.2, 1, 20, 7), reach_border),
    "border-240x240": (lambda: noise(BORDER_SEEDS[240], 240, 240), ORB8, reach_border),
    "dense-cell": (lattice_cell, ORB1, reach_dense),
}
BORDER_SEEDS = {67: 0, 240: 0}   # noise seeds whose level-0 candidates touch all four sides of the box
SWEEP_CASES = ["ties-100"]       # also run under ORBHIP_OCTREE_SWEEP=1
