"""The projection searches' route table (orbhip_test_proj_route, host code only) and the
preconditions of the crafted scenes of tests/proj_cases.py, on the CPU with the oracle and numpy
alone: a scene that does not reach the edge it was built for fails here, and cannot pass quietly
on the GPU (tests/test_proj_routes_gpu.py)."""
import ctypes

import numpy as np
import pytest

import proj_cases as pc
from helpers import proj_route
from orb_slam3_ros2_amd.matcher import ProjFrame
from orb_slam3_ros2_amd.synthetic import synthetic_projection_scene


def frame_of(s, **kw):
    return ProjFrame(s["kps"], s["desc"], s["pose_q"], s["pose_t"], s["fx"], s["fy"], s["cx"], s["cy"],
                     claimed=s["claimed"], **kw)


def oracle_last(oracle, s, f, ori=False, th=None):
    return oracle.search_by_projection_last(f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"],
                                            s.get("th_last", 15.0) if th is None else th, ori)


def oracle_local(oracle, s, f, th=None, nnratio=None):
    return oracle.search_local_points(f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"],
                                      s["skip"], th=s.get("th_local", 1.0) if th is None else th,
                                      nnratio=s.get("nnratio", 0.8) if nnratio is None else nnratio)


def natural_entries():
    """2000 x 2000 searched with th 25: far more list entries than the resolve holds in LDS, no
    list above 128 (both asserted below)."""
    s = synthetic_projection_scene(n_kp=2000, n_mp=2000, seed=70)
    s["th_last"] = 25.0
    return s


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in ("ORBHIP_PROJ_ROUNDS", "ORBHIP_PROJ_TWO", "ORBHIP_PROJ_CAP", "ORBHIP_PROJ_DMA"):
        monkeypatch.delenv(k, raising=False)


# ---- the route table ----

def test_route_size_gates():
    assert proj_route(8192, 64)["lists"] and not proj_route(8193, 64)["lists"]
    assert proj_route(300, 8192)["lists"] and not proj_route(300, 8193)["lists"]
    r = proj_route(8192, 6911)
    assert r["lists"] and r["ent_cap"] == 0
    assert not proj_route(8192, 6912)["lists"]          # the resolve's head alone exceeds its LDS
    assert proj_route(1000, 900, 15)["lists"] and not proj_route(1000, 900, 16)["lists"]
    r = proj_route(1000, 900)
    assert r == {"lists": True, "ent_cap": pc.ent_cap_of(1000, 900), "cap": 128, "fused": True}
    assert 16000 < r["ent_cap"] < 17500
    for n, nq in [(0, 1), (1, 1), (2000, 2000), (8192, 6911), (8192, 6000), (pc.ENTRIES_N, pc.ENTRIES_NQ)]:
        assert proj_route(n, nq)["ent_cap"] == pc.ent_cap_of(n, nq), (n, nq)


def test_route_switches(monkeypatch):
    monkeypatch.setenv("ORBHIP_PROJ_ROUNDS", "1")
    assert not proj_route(1000, 900)["lists"]
    monkeypatch.setenv("ORBHIP_PROJ_ROUNDS", "0")
    assert proj_route(1000, 900)["lists"]
    monkeypatch.delenv("ORBHIP_PROJ_ROUNDS")
    monkeypatch.setenv("ORBHIP_PROJ_TWO", "1")
    r = proj_route(1000, 900)
    assert r["lists"] and not r["fused"]
    monkeypatch.delenv("ORBHIP_PROJ_TWO")
    for v, want in [("2", 2), ("1", 1), ("0", 1), ("-5", 1), ("128", 128), ("129", 128), ("100000", 128), ("64", 64)]:
        monkeypatch.setenv("ORBHIP_PROJ_CAP", v)
        assert proj_route(1000, 900)["cap"] == want, v
    monkeypatch.delenv("ORBHIP_PROJ_CAP")
    assert proj_route(1000, 900)["cap"] == 128


def test_route_rejects_bad_arguments():
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 4)()
    f = lib().orbhip_test_proj_route
    assert f(10, 10, 0, None) == -1
    assert f(-1, 10, 0, out) == -1 and f(10, -1, 0, out) == -1 and f(10, 10, -1, out) == -1
    assert f(65536, 10, 0, out) == -1 and f(65535, 10, 0, out) == 0 and out[0] == 0


# ---- the crafted scenes reach what they were built for ----

@pytest.mark.parametrize("K", [3, 70, 102])
def test_chain_last_precondition(oracle, K):
    s = pc.chain(K)
    f = frame_of(s)
    n, m = oracle_last(oracle, s, f)
    assert np.array_equal(m, s["expect"]) and n == min(K, 101)
    if K == 102:
        assert m[100] == 100 and m[101] == -1      # TH_HIGH itself matches, 101 does not
    rect, cand = pc.counts_last(s, f)
    assert (cand == K).all() and (rect == K).all()


def test_chain_last_rotation_outliers_are_dropped(oracle):
    s = pc.chain(70, rot_outliers=(5, 33, 60))
    n, m = oracle_last(oracle, s, frame_of(s), ori=True)
    want = s["expect"].copy()
    want[[5, 33, 60]] = -1
    assert n == 67 and np.array_equal(m, want)


def test_chain_local_preconditions(oracle):
    s = pc.chain(70, "local")
    n, m, iv, lvl = oracle_local(oracle, s, frame_of(s))
    assert n == 70 and np.array_equal(m, s["expect"]) and iv.all() and (lvl == pc.LEVEL).all()
    s = pc.chain(12, "ratio")
    n, m, iv, lvl = oracle_local(oracle, s, frame_of(s))
    assert np.array_equal(m, s["expect"]) and iv.all() and (lvl == pc.LEVEL).all()
    assert n == 5 and (m[:5] >= 0).all() and (m[5:] == -1).all()      # matches, then in-view rejections
    # without the ratio test (best and second on different levels) every query of the same scene matches
    s["kps"]["octave"][1::2] = pc.LEVEL - 1
    assert oracle_local(oracle, s, frame_of(s))[0] == 12


def test_ties_precondition(oracle):
    s = pc.ties()
    f = frame_of(s)
    n, m = oracle_last(oracle, s, f)
    assert n == 40 and np.array_equal(m, s["expect"]) and not np.array_equal(m, np.arange(40))
    cells = np.round(s["kps"]["x"] / 10).astype(int) * 48 + np.round(s["kps"]["y"] / 10).astype(int)
    assert len(set(cells.tolist())) == 40 and (np.diff(cells) < 0).all()
    assert (pc.counts_last(s, f)[1] == 40).all()


@pytest.mark.parametrize("R", [512, 513])
def test_dense_rect_precondition(oracle, R):
    s = pc.dense_rect(R)
    f = frame_of(s)
    rect, cand = pc.counts_last(s, f)
    assert (rect == R).all() and (cand == 40).all() and len(s["kps"]) % 256 != 0
    n, m = oracle_last(oracle, s, f)
    assert n == 40 and np.array_equal(m, s["expect"])


@pytest.mark.parametrize("C,claim,listed", [(128, False, 128), (129, False, 129), (129, True, 128)])
def test_list_count_precondition(oracle, C, claim, listed):
    s = pc.list_count(C, claim)
    f = frame_of(s)
    rect, cand = pc.counts_last(s, f)
    big = s["big_query"]
    assert cand[big] == listed and rect[big] == C and (np.delete(cand, big) == 1).all()
    n, m = oracle_last(oracle, s, f)
    assert n == 41 and np.array_equal(m, s["expect"])


@pytest.mark.parametrize("extra", [0, 1])
def test_entries_precondition(oracle, extra):
    s = pc.entries(extra)
    f = frame_of(s)
    assert (len(s["kps"]), len(s["points"])) == (pc.ENTRIES_N, pc.ENTRIES_NQ)
    r = proj_route(pc.ENTRIES_N, pc.ENTRIES_NQ)
    assert r["lists"] and r["ent_cap"] == s["ent_cap"] > 0
    rect, cand = pc.counts_last(s, f)
    assert cand.sum() == s["total"] == r["ent_cap"] + extra and cand.max() <= 10
    assert oracle_last(oracle, s, f)[0] > 90


def test_natural_entries_precondition(oracle):
    s = natural_entries()
    f = frame_of(s)
    rect, cand = pc.counts_last(s, f)
    r = proj_route(2000, 2000)
    assert r["lists"] and cand.sum() > 2 * r["ent_cap"] and 64 < cand.max() <= 128, (cand.sum(), cand.max())
    assert oracle_last(oracle, s, f, ori=True)[0] > 500


def test_dist256_precondition(oracle):
    s = pc.dist256()
    f = frame_of(s)
    n, m = oracle_last(oracle, s, f)
    assert n == 5 and np.array_equal(m, s["expect"])
    assert (pc.counts_last(s, f)[1] == 1).all()
    n, m, iv, lvl = oracle_local(oracle, s, f)
    assert n == 5 and np.array_equal(m, s["expect"]) and iv.all()
    win = pc.windows_local(f, s["points"], s["normals"], s["th_local"], iv, lvl)
    assert (pc.window_counts(f, win)[1] == 1).all()
    from oracle.pyoracle import lib
    assert lib().orc_descriptor_distance(s["mp_desc"][2], s["desc"][2]) == 256


def test_scale_steps_straddle_every_step(oracle):
    s = pc.scale_steps()
    f = frame_of(s, n_levels=pc.STEP_LEVELS)
    n, m, iv, lvl = oracle_local(oracle, s, f)
    assert iv.all()
    for k in range(8):
        got = set(lvl[s["k"] == k].tolist())
        assert got == {k, k + 1}, (k, got)
    assert n > 0


@pytest.mark.parametrize("sf,n_levels", [(1.2, 8), (2.0, 8), (1.2, 10), (1.1, 16)])
def test_level_thresholds_reproduce_the_host_level(oracle, sf, n_levels):
    """The steps the device compares a ratio against (orbhip_test_level_thresholds, host code only):
    counting the steps at or below a ratio gives the oracle's level for every float in [0.5, 8) at
    1.2 / 8 levels, and 65536 floats either side of every step otherwise. This is also the check
    that the level is monotone in the ratio, which the bisection behind the steps relies on."""
    from orb_slam3_ros2_amd._lib import lib
    log_sf = float(np.log(np.float32(sf)).astype(np.float32))
    thr = np.zeros(n_levels, np.float32)
    assert lib().orbhip_test_level_thresholds(log_sf, n_levels, thr.ctypes.data) == 0
    assert (np.diff(thr[1:]) > 0).all() and thr[1] > 1.0
    bits = lambda x: int(np.float32(x).view(np.uint32))
    if (sf, n_levels) == (1.2, 8):
        ranges = [(bits(0.5), bits(8.0) - 1)]
    else:
        ranges = [(bits(t) - 65536, bits(t) + 65536) for t in thr[1:]]
    for lo, hi in ranges:
        for a in range(lo, hi + 1, 1 << 24):
            b = min(a + (1 << 24) - 1, hi)
            ratio = np.arange(a, b + 1, dtype=np.uint32).view(np.float32)
            got = np.searchsorted(thr[1:], ratio, side="right").astype(np.int8)
            assert np.array_equal(got, oracle.predict_scale_range(a, b, log_sf, n_levels)), (sf, n_levels, a)
    assert lib().orbhip_test_level_thresholds(log_sf, 0, thr.ctypes.data) == -1
    assert lib().orbhip_test_level_thresholds(log_sf, 8, None) == -1


def test_predict_scale_range_is_the_search_s_level(oracle):
    """orc_predict_scale_range restates the level of orc_search_local_points: the levels of the
    step scene, recomputed from the ratios the search forms."""
    s = pc.scale_steps()
    f = frame_of(s, n_levels=pc.STEP_LEVELS)
    lvl = oracle_local(oracle, s, f)[3]
    P, Ow = s["points"], -s["pose_t"]
    PO = [P[:, i] - Ow[i] for i in range(3)]
    ratio = s["max_dist"] / np.sqrt(PO[0] * PO[0] + PO[1] * PO[1] + PO[2] * PO[2])
    assert ratio.dtype == np.float32
    for r, want in zip(ratio, lvl):
        b = int(r.view(np.uint32))
        assert oracle.predict_scale_range(b, b, f.log_scale_factor, pc.STEP_LEVELS)[0] == want
    lo, hi = int(np.float32(0.5).view(np.uint32)), int(np.float32(8.0).view(np.uint32)) - 1
    a = oracle.predict_scale_range(lo, lo + 99999, f.log_scale_factor, 8)
    b = oracle.predict_scale_range(hi - 99999, hi, f.log_scale_factor, 8)
    assert (np.diff(a) >= 0).all() and a[0] == 0 and b[-1] == 7 and (np.diff(b) >= 0).all()
