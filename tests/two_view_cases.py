"""The scenes of the TwoViewReconstruction tests (tests/test_two_view.py asserts their conditions on
the CPU, tests/test_two_view_gpu.py compares the device with the restatement on them). A scene is a
problem dict: kps1, kps2 (n x 2 float32), matches12, K, sigma, sets."""
import functools

import numpy as np

from orb_slam3_ros2_amd.synthetic import synthetic_two_view_scene

# With upstream's RH > 0.50 a homography wins only when the fundamental-matrix hypotheses are poor
# (synthetic_two_view_scene, "doubled"): the scenes that reach ReconstructH double their matches.
_TILTED = dict(kind="planar", doubled=True, plane=(3.5, -0.6, 0.3), t_mean=(1.5, 0.0, 0.0))

SCENES = {
    # ---- the parity set ----
    "general": dict(kind="general", n=240, seed=5),                        # F wins and succeeds
    "planar": dict(n=240, seed=1, **_TILTED),                              # H wins and succeeds
    "mixed": dict(kind="mixed", n=240, seed=2),                            # half plane, half volume
    "rotation": dict(kind="rotation", n=240, seed=1),                      # no baseline: two equal hypotheses
    "low_parallax": dict(kind="low_parallax", n=240, seed=1),
    "outliers30": dict(kind="general", n=300, seed=4, outlier_frac=0.3),
    "unmatched": dict(kind="general", n=240, seed=3, unmatched_frac=0.4),
    # ---- the exits of the two reconstructions ----
    "exit_d_ratio": dict(kind="rotation", n=240, seed=2, doubled=True, noise_px=0.0),   # A = a rotation: d1 = d2 = d3
    "exit_nsimilar": dict(kind="rotation", n=240, seed=2),                 # ReconstructF: nsimilar > 1
    "exit_min_good": dict(kind="general", n=240, seed=1, unmatched_frac=0.4),   # maxGood < nMinGood
    "exit_second_best": dict(kind="planar", n=240, seed=1, doubled=True),  # secondBest >= 0.75 best
    "exit_min_triangulated": dict(n=48, seed=1, **_TILTED),                # best <= minTriangulated
    # ---- min(50, size - 1): at most 50 good points, exactly 51, more ----
    "good_51": dict(kind="general", n=52, seed=2, outlier_frac=0.0),
    "good_many": dict(kind="general", n=120, seed=2, outlier_frac=0.0),
    # ---- a reprojection error exactly at th2 = 4 fl(sigma sigma): "unmatched" with the sigma that puts
    # th2 on the fp32 error of match 28 in image 2 under the accepted hypothesis (TH2_MATCH), where
    # `error > th2` is false, and with the next sigma below, where it is true ----
    "th2_at": dict(kind="general", n=240, seed=3, unmatched_frac=0.4, sigma=1.0392229557037354),
    "th2_above": dict(kind="general", n=240, seed=3, unmatched_frac=0.4, sigma=1.0392228364944458),
}
TH2 = ("th2_at", "th2_above")
TH2_MATCH = dict(hypothesis=1, image="err2", match=28)
PARITY = ("general", "planar", "mixed", "rotation", "low_parallax", "outliers30", "unmatched")
EXITS = ("exit_d_ratio", "exit_nsimilar", "exit_min_good", "exit_second_best", "exit_min_triangulated")


@functools.lru_cache(maxsize=None)
def scene(name):
    """Scene `name` (built once, shared; treat as read-only)"""
    if name == "good_le_50":
        return _good_le_50()
    return synthetic_two_view_scene(**SCENES[name])


def _good_le_50():
    """good_many cut down to 51 of the matches its accepted hypothesis counts, with sets of its own:
    CheckRT's list then holds 50 cosines or fewer (the CPU test asserts the counts of the three
    good_* scenes)."""
    import two_view_numpy as T
    p = dict(scene("good_many"))
    o = T.reconstruct(p)
    first = o["first"]
    counted = np.nonzero(np.any(o["p3d"][first] != 0, 1))[0]
    keep = counted[:51]
    m = np.full_like(p["matches12"], -1)
    m[first[keep]] = p["matches12"][first[keep]]
    draw = np.random.default_rng(5)
    from orb_slam3_ros2_amd.two_view import draw_sets
    p["matches12"] = m
    p["sets"] = draw_sets(51, 200, lambda lo, hi: int(draw.integers(lo, hi + 1)))
    return p


def sized(n, n_hyp, seed=0, **kw):
    """A general scene of n matches and n_hyp sets for the size edges"""
    return synthetic_two_view_scene("general", n=n, seed=100 + seed, n_hyp=n_hyp, outlier_frac=0.1 if n >= 20 else 0.0, **kw)


def batch_problem(b):
    """Problem b of the batch-edge calls: a match count, set count, camera and unmatched share of
    its own"""
    cam = dict(fx=500.0 + 3 * b, fy=510.0 - b, cx=320.0 + b, cy=240.5)
    return sized(8 + (7 * b) % 90, 1 + (5 * b) % 17, seed=500 + b, cam=cam, unmatched_frac=0.1 * (b % 4))


def coincident(n=12, n_hyp=5):
    """Every match at one place: Normalize divides by a mean deviation of 0, every matrix is NaN,
    no hypothesis ever wins: SH + SF == 0"""
    p = dict(sized(n, n_hyp))
    p["kps1"] = np.tile(np.array([[100.0, 80.0]], np.float32), (len(p["kps1"]), 1))
    p["kps2"] = np.tile(np.array([[120.5, 90.25]], np.float32), (len(p["kps2"]), 1))
    return p


def with_twin_points(name="general", h=3):
    """Scene `name` with eight of its outlier matches moved onto one place in both frames, and set h
    drawn from them (eight copies of one point), set h + 1 = set 0 (two identical sets)"""
    p = dict(scene(name))
    first = np.nonzero(p["matches12"] >= 0)[0]
    idx = np.nonzero(p["outlier"])[0][:8]
    assert len(idx) == 8
    k1, k2 = p["kps1"].copy(), p["kps2"].copy()
    k1[first[idx]] = k1[first[idx[0]]]
    k2[p["matches12"][first[idx]]] = k2[p["matches12"][first[idx[0]]]]
    sets = p["sets"].copy()
    sets[h] = idx
    sets[h + 1] = sets[0]
    p.update(kps1=k1, kps2=k2, sets=sets, twin_h=h)
    return p


def all_sets_degenerate(name="outliers30", n_hyp=6):
    """with_twin_points with every set drawn from the eight coincident matches (the other matches
    stay distinct): all 2 n_hyp hypotheses come from null spaces of several dimensions"""
    p = with_twin_points(name)
    idx = p["sets"][p["twin_h"]]
    p["sets"] = np.stack([np.roll(idx, k) for k in range(n_hyp)]).astype(np.int32)
    return p


@functools.lru_cache(maxsize=None)
def degenerate_problems():
    """name -> problem of the degenerate-set comparisons (`identical` needs the winner of `twins`)"""
    import two_view_numpy as T
    twins = with_twin_points("outliers30")
    best_f = T.reconstruct(twins)["best_f"]
    return dict(twins=twins, identical=dict(twins, sets=np.tile(twins["sets"][best_f], (4, 1))),
                coincident=coincident(), all_sets_degenerate=all_sets_degenerate())
