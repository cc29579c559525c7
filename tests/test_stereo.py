"""The restatement of Frame::ComputeStereoMatches (tests/stereo_numpy.py) pinned on the CPU: a
definitional known-answer test, its SAD and its median cut against plain loops, the branches its
scene set reaches (tests/test_stereo_gpu.py runs the library on exactly these scenes) and a golden
fixture. Inputs come from the oracle extractor with vLappingArea (0, 0) and the oracle pyramid."""
import os

import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import synthetic_frame, synthetic_stereo_pair

import stereo_numpy as S
from stereo_cases import upstream_median_loop

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_320x240_s5.npz")


def test_library_exports_the_stereo_entry_points():
    from orb_slam3_ros2_amd import _lib
    L = _lib.lib()
    for name in ("orbhip_extract_stereo", "orbhip_extract_stereo_device", "orbhip_test_stereo_match"):
        assert hasattr(L, name), name
    assert "orbhip_extract_stereo" in _lib.EXPORTED and "orbhip_extract_stereo_device" in _lib.EXPORTED
    assert "orbhip_test_stereo_match" not in _lib.EXPORTED   # a hook: not declared in the header


def test_std_round_is_not_numpy_round():
    assert [S.std_round(f32(v)) for v in (0.5, 1.5, 2.5, -0.5, -2.5, 2.4999, 3.0)] == [1, 2, 3, -1, -3, 2, 3]
    assert np.round(f32(2.5)) == 2   # why the restatement does not use it


def test_synthetic_stereo_pair_is_seeded_and_shifted():
    l0, r0 = synthetic_stereo_pair(3, 320, 240)
    l1, r1 = synthetic_stereo_pair(3, 320, 240)
    assert np.array_equal(l0, l1) and np.array_equal(r0, r1) and l0.shape == (240, 320) and l0.dtype == np.uint8
    assert not np.array_equal(l0, r0)
    l2, _ = synthetic_stereo_pair(4, 320, 240)
    assert not np.array_equal(l0, l2)
    # noise-free: zero disparity gives the same image twice; quarter-pixel disparities give the
    # right image blended edge values that the left image does not hold
    l, r = synthetic_stereo_pair(0, 64, 32, n_rect=5, noise_sigma=0.0, max_disparity=0.0)
    assert np.array_equal(l, r)
    l, r = synthetic_stereo_pair(0, 64, 32, n_rect=5, noise_sigma=0.0, max_disparity=8.0)
    assert set(np.unique(r).tolist()) - set(np.unique(l).tolist())


def test_definitional_kat(oracle):
    """right[y, x] = left[y, min(x + d, w - 1)], d = 7, no fresh noise: every accepted octave-0
    keypoint has best SAD 0 and |(uL - uRight) - d| <= 0.5 (deltaR = (d1 - d3) / (2 (d1 + d3)) with
    d2 = 0 lies in [-0.5, 0.5]) + 1e-3."""
    d, w, h = 7, 320, 240
    left = synthetic_frame(41, w, h)
    right = left[:, np.minimum(np.arange(w) + d, w - 1)].copy()
    kl, dl, kr, dr, pl, pr = S.extract_pair(oracle, left, right)
    sc, inv = S.scale_tables(oracle, w, h)
    for cp in (0, 1):
        r = S.compute_stereo_matches(kl, dl, kr, dr, pl, pr, sc, inv, 40.0, 1.0, cp)
        acc0 = np.flatnonzero((r.status == 1) & (kl["octave"] == 0))
        assert len(acc0) > 50, len(acc0)
        assert (r.sad[acc0] == 0).all(), r.sad[acc0][r.sad[acc0] != 0]
        err = np.abs((kl["x"][acc0].astype(np.float64) - r.u_right[acc0]) - d)
        assert err.max() <= 0.5 + 1e-3, err.max()
        assert (r.depth[acc0] > 0).all() and (r.u_right[r.status != 1] == -1).all() and (r.depth[r.status != 1] == -1).all()


@pytest.mark.parametrize("cp", [0, 1])
def test_sad_equals_a_plain_double_loop(oracle, cp):
    """20 random left keypoints at their own levels and scaled positions, against a right centre
    up to 30 level pixels to their left."""
    s = S.parity_scene(oracle, 0)
    rng = np.random.default_rng(7)
    for i in rng.choice(len(s["kps_l"]), size=20, replace=False):
        lev = int(s["kps_l"]["octave"][i])
        lev_l, lev_r = s["pyr_l"][lev], s["pyr_r"][lev]
        sul = S.std_round(s["kps_l"]["x"][i] * s["inv_scale"][lev])
        svl = S.std_round(s["kps_l"]["y"][i] * s["inv_scale"][lev])
        sur0 = max(sul - int(rng.integers(0, 31)), 10)
        got = S.patch_sads(lev_l, lev_r, sul, svl, sur0, cp)
        for inc in range(-5, 6):
            tot = 0
            cl, cr = int(lev_l[svl, sul]), int(lev_r[svl, sur0 + inc])
            for dy in range(-5, 6):
                for dx in range(-5, 6):
                    a, b = int(lev_l[svl + dy, sul + dx]), int(lev_r[svl + dy, sur0 + inc + dx])
                    tot += abs((a - cl) - (b - cr)) if cp else abs(a - b)
            assert got[5 + inc] == tot


def test_median_cut_equals_upstreams_loop():
    """Upstream sorts (SAD, iL), takes sorted[size / 2].first and walks back from the end until the
    first SAD below thDist (stereo_cases.upstream_median_loop, shared with test_stereo_cases.py)."""
    rng = np.random.default_rng(11)
    for n in (1, 2, 3, 10, 101, 500):
        for hi in (3, 40, 60000):
            sads = rng.integers(0, hi, size=n + 5)
            acc = np.sort(rng.choice(n + 5, size=n, replace=False))
            assert sorted(S.median_cut(sads, acc)) == sorted(upstream_median_loop(sads, acc))
    assert S.median_cut(np.zeros(4, int), []) == []
    assert S.median_cut(np.array([7]), [0]) == []          # alone: 7 < 2.1 * 7
    assert S.median_cut(np.array([0]), [0]) == [0]         # alone with SAD 0: 0 >= 0


def test_delta_gate():
    """The gate itself (a NaN passes). With integer SADs it cannot fire: d2 is the strict first
    minimum of the eleven and not at an end, so d1 > d2 and d3 >= d2, the denominator
    2 (d1 + d3 - 2 d2) is positive and |d1 - d3| <= d1 + d3 - 2 d2, i.e. |deltaR| <= 0.5."""
    assert S.delta_gate(S.parabola(0, 5, 10)) and S.delta_gate(S.parabola(10, 5, 0))
    assert not S.delta_gate(S.parabola(9, 5, 9)) and not S.delta_gate(S.parabola(5, 5, 5))   # 0, NaN
    assert np.isnan(S.parabola(5, 5, 5))
    rng = np.random.default_rng(3)
    for _ in range(2000):
        d2 = int(rng.integers(0, 61711))
        d1, d3 = d2 + 1 + int(rng.integers(0, 1000)), d2 + int(rng.integers(0, 1000))
        assert abs(S.parabola(d1, d2, d3)) <= f32(0.5)


def test_scene_set_reaches_every_branch(oracle):
    """Every status occurs in at least one scene, and so do a Hamming tie between two right
    keypoints, an equal-SAD tie and the disparity <= 0 substitution. Status 6 is the exception: no
    input reaches it (test_delta_gate), which the scenes confirm by |deltaR| <= 0.5 throughout."""
    seen, ev = set(), dict(hamming_tie=0, sad_tie=0, disparity_sub=0)
    sizes = set()
    for k in range(len(S.PARITY_SCENES)):
        s = S.parity_scene(oracle, k)
        sizes.add(s["left"].shape)
        for cp in (0, 1):
            r = S.restate(s, cp)
            assert r.status.min() >= 1 and r.status.max() <= 9
            seen |= set(r.status.tolist())
            for name in ev:
                ev[name] += r.events[name]
            assert r.events["max_abs_delta"] <= 0.5
            assert r.n_stereo == (r.status == 1).sum() and (r.u_right[r.status == 1] >= 0).all()
        if "planted" in s:
            p, r = s["planted"], S.restate(s, 0)
            assert (r.status[p["guard"]] == 9).all() and r.status[p["ini_end"]] == 4 and r.status[p["flat"]] == 5
            assert (r.status[p["no_row"]] == 2).all() and r.status[p["bad_right"]] in (2, 3)
            twins = np.flatnonzero((s["desc_r"] == s["desc_l"][p["ham_tie"]]).all(axis=1))
            assert len(twins) == 2 and r.best_r[p["ham_tie"]] == twins.min()   # the lower iR wins the tie
            i = p["zero_disp"]   # the substitution: disparity 0.01, uRight = (float)((double)uL - 0.01)
            assert r.status[i] == 1 and r.depth[i] == f32(s["bf"]) / f32(0.01)
            assert r.u_right[i] == f32(np.float64(s["kps_l"]["x"][i]) - 0.01)
    assert seen == {1, 2, 3, 4, 5, 7, 8, 9}, seen
    assert all(v > 0 for v in ev.values()), ev
    assert sizes == {(240, 320), (480, 640)}


def test_golden_fixture(oracle):
    g = np.load(GOLDEN)
    assert (int(g["seed"]), int(g["width"]), int(g["height"])) == S.PARITY_SCENES[0][1:4]
    s = S.parity_scene(oracle, 0)
    assert (float(g["bf"]), float(g["b"])) == (s["bf"], s["b"])
    r = S.restate(s, int(g["center_patch"]))
    assert np.array_equal(r.status, g["status"])
    assert np.array_equal(r.u_right.view(np.uint32), g["u_right"].view(np.uint32))
    assert np.array_equal(r.depth.view(np.uint32), g["depth"].view(np.uint32))
