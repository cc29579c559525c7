"""The brute-force matcher's dispatch table and the planted-match generator, on the CPU: the
route function is host code (the library loads without a device), the generator is checked
against the oracle alone. The GPU tests in test_match_routes_gpu.py assert their route through
the same hook, so a moved constant fails here and there instead of silently testing another row."""
import numpy as np
import pytest

from tests.helpers import MATCH_HIST_IDS as HIST_IDS, MATCH_HISTOGRAMS as HISTOGRAMS, match_route, planted_match_set


@pytest.fixture
def clean_env(monkeypatch):
    for k in ("ORBHIP_MATCH_UNFUSED", "ORBHIP_MATCH_TC", "ORBHIP_MATCH_XCD"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def test_route_table(clean_env):
    """Every row of run_match's dispatch: k_match_fused (<= 4 pairs), k_match_top2<64> (the "small"
    rule), <256> with and without the xcd_runs remap, <512> / <1024> (ORBHIP_MATCH_TC),
    ORBHIP_MATCH_XCD=0, and the 4-byte / 8-byte partial formats at the 14-bit edge."""
    env = clean_env
    assert match_route(1, 1000, 2000)["kernel"] == "fused"
    assert match_route(4, 1024, 1024)["kernel"] == "fused"
    assert match_route(5, 1024, 1024)["kernel"] != "fused"
    assert match_route(1, 1000, 2000, fused_allowed=False) == {"kernel": "tc64", "nch": 32, "xrun": 0, "pk": 1}
    env.setenv("ORBHIP_MATCH_UNFUSED", "1")
    assert match_route(1, 1000, 2000) == {"kernel": "tc64", "nch": 32, "xrun": 0, "pk": 1}
    # 32 query blocks x 16 chunks = 512: not "small"
    assert match_route(1, 2048, 4096) == {"kernel": "tc256", "nch": 16, "xrun": 0, "pk": 1}
    assert match_route(1, 2048 - 64, 4096)["kernel"] == "tc64"
    env.setenv("ORBHIP_MATCH_UNFUSED", "0")
    assert match_route(1, 1000, 2000)["kernel"] == "fused"
    env.delenv("ORBHIP_MATCH_UNFUSED")
    assert match_route(5, 1536, 1536) == {"kernel": "tc256", "nch": 6, "xrun": 0, "pk": 1}
    assert match_route(7, 1024, 1024)["xrun"] == 0 and match_route(8, 1024, 1024)["xrun"] == 64
    assert match_route(9, 1024, 1024) == {"kernel": "tc256", "nch": 4, "xrun": 64, "pk": 1}
    env.setenv("ORBHIP_MATCH_XCD", "0")
    assert match_route(9, 1024, 1024) == {"kernel": "tc256", "nch": 4, "xrun": 0, "pk": 1}
    env.delenv("ORBHIP_MATCH_XCD")
    env.setenv("ORBHIP_MATCH_TC", "512")
    assert match_route(9, 1024, 1024) == {"kernel": "tc512", "nch": 2, "xrun": 32, "pk": 1}
    assert match_route(1, 1000, 2000, fused_allowed=False)["kernel"] == "tc64"   # "small" ignores the switch
    env.setenv("ORBHIP_MATCH_TC", "1024")
    assert match_route(9, 1024, 1024) == {"kernel": "tc1024", "nch": 1, "xrun": 16, "pk": 1}
    env.setenv("ORBHIP_MATCH_TC", "300")      # anything else: 256
    assert match_route(9, 1024, 1024)["kernel"] == "tc256"
    env.delenv("ORBHIP_MATCH_TC")
    assert match_route(1, 130, 16383, False) == {"kernel": "tc64", "nch": 256, "xrun": 0, "pk": 1}
    assert match_route(1, 130, 16384, False) == {"kernel": "tc64", "nch": 256, "xrun": 0, "pk": 0}
    assert match_route(9, 1024, 16383)["pk"] == 1 and match_route(9, 1024, 16384)["pk"] == 0


def test_route_hook_rejects_bad_arguments():
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 4)()
    assert lib().orbhip_test_match_route(1, 10, 10, 1, None) == -1
    assert lib().orbhip_test_match_route(0, 10, 10, 1, out) == -1
    assert lib().orbhip_test_match_route(1, -1, 10, 1, out) == -1


@pytest.mark.parametrize("hist,keep,kept", HISTOGRAMS, ids=HIST_IDS)
def test_planted_sets_are_what_the_oracle_accepts(oracle, hist, keep, kept):
    """The construction the GPU tests stand on: with flips 0..40, TH_LOW 50 and ratio 0.9 the
    oracle accepts exactly the planted queries, each at its train with best == its flips, and the
    rotation filter keeps exactly the bins (and the count) ComputeThreeMaxima's rules give."""
    ds = planted_match_set(300, 700, hist, (0, 40), seed=31)
    assert int(ds.planted.sum()) == sum(hist.values())
    n, m, b, s = oracle.match_bf(ds.q, ds.qa, ds.t, ds.ta, 50, 0.9, False)
    assert n == sum(hist.values()) and np.array_equal(m, ds.train)
    assert np.array_equal(b[ds.planted], ds.flips[ds.planted]) and b[~ds.planted].min() > 50
    n, m, _, _ = oracle.match_bf(ds.q, ds.qa, ds.t, ds.ta, 50, 0.9, True)
    assert n == kept and np.array_equal(m, np.where(np.isin(ds.bin, keep), ds.train, -1))


def test_planted_bins_stay_below_13():
    """rot in [0, 360) times 1/30 rounds to 0..12 only: `bin == 30` never happens and bins 13..29
    stay empty; the generator's rotations 30 b and 350 land in bins b and 12."""
    rot = np.arange(360, dtype=np.float32)
    x = rot * np.float32(1.0 / 30)                            # the float product the kernels and the oracle form
    bins = np.floor(x.astype(np.float64) + 0.5).astype(int)   # roundf: halves away from zero
    assert bins.min() == 0 and bins.max() == 12
    assert all(bins[30 * b] == b for b in range(12)) and bins[350] == 12


def test_planted_explicit_distances(oracle):
    ds = planted_match_set(8, 100, None, seed=5, plants=[(0, 10, 7), (0, 20, 7), (1, 30, 9), (1, 5, 8), (2, 99, 0)])
    assert np.array_equal(ds.t[10], ds.t[20]) and list(ds.train[:3]) == [10, 5, 99]
    n, m, b, s = oracle.match_bf(ds.q, ds.qa, ds.t, ds.ta, 50, 1.01, True)
    assert list(m[:3]) == [10, 5, 99] and list(b[:3]) == [7, 8, 0] and list(s[:2]) == [7, 9] and n == 3
