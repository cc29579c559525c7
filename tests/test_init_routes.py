"""SearchForInitialization at the limits of its routes, on the CPU: every crafted scene of
tests/init_cases.py reaches the edge it was built for. The model there restates the device
formulation (ranks, lists, the per-lane top-4 and its `lost` rule, `need`, the fixed-point rounds
and their claimants, the chain); here its matches equal the oracle's on every scene, and the need
counts, whole-list scans, rounds and claimants it finds equal the figures each scene plants by
construction. A scene that drifts off its edge fails here; tests/test_init_routes_gpu.py then
demands the same figures and the oracle's result from the device. Also the envelope arithmetic
(init_search's own function through orbhip_test_init_route, host only)."""
import numpy as np
import pytest

import init_cases as ic
from helpers import init_route

ERR_ARG, ERR_UNSUPPORTED = -1, -5


def oracle_init(oracle, s, ratio=None, ori=True):
    return oracle.search_for_initialization(s["k1"], s["d1"], s["k2"], s["d2"], s["prev"], s["window"],
                                            s["ratio"] if ratio is None else ratio, ori, bounds=s["bounds"])


def assert_model_is_oracle(oracle, s, ratio=None, ori=True):
    m = ic.model(s, ratio, ori)
    on, om, op = oracle_init(oracle, s, ratio, ori)
    assert m["n"] == on and np.array_equal(m["m12"], om) and np.array_equal(m["prev"], op)
    if m["form"] == 0:      # the converged rounds and the chain are one result
        assert np.array_equal(m["rounds_m12"], om)
    return m, om


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("name", list(ic.CRAFTED))
def test_scene_reaches_its_edge(oracle, name, ori):
    s = ic.crafted(name)
    m, om = assert_model_is_oracle(oracle, s, ori=ori)
    for key, want in s["plant"].items():
        assert m[key] == want, (key, m[key], want)
    for i1, i2 in s["expect"].items():
        assert om[i1] == i2, (i1, om[i1], i2)
    if "Q" in s:
        q = m["nq0"] - 1                            # Q is the last query
        assert m["need"][q] == (2 if name.startswith("lost") else 1)
        assert m["lens"][q] == len(s["k2"]) > ic.K16
    if "q_slot" in s:
        assert (m["nq0"] - 1) % 4 == s["q_slot"]


def test_lost_scene_off_its_lane_is_noticed(oracle):
    """The check above is not vacuous: with the lane's third to sixth entries spread over three other
    lanes no lane pops four, nothing is lost, and the planted need2 no longer holds. (Moving the
    fifth alone would not do: a lane that pops its four kept entries while it saw more is `lost`
    whether or not the fifth was among the 16.)"""
    s = dict(ic.lost(7, 0))
    d2 = s["d2"].copy()
    d2[[135, 136, 199, 201, 263, 266, 327, 329]] = d2[[136, 135, 201, 199, 266, 263, 329, 327]]
    s["d2"] = d2
    m = ic.model(s)
    assert m["need2"] == 0 and m["need1"] == 5
    assert m["m12"][s["Q"]] == 266          # the same keypoint: now the 16 smallest hold it


@pytest.mark.parametrize("N", ic.CHAIN_N)
def test_chain_rounds(oracle, N):
    """Round r of the fixed point sets query r right: N queries end in round N, which the cap of
    min(64, N + 2) rounds allows for N <= 63 only."""
    m, om = assert_model_is_oracle(oracle, ic.crafted(f"chain-{N}"))
    assert (om[:N] == np.arange(1, N + 1)).all()
    assert (m["form"], m["rounds"]) == ((0, N) if N <= 63 else (2, None))


@pytest.mark.parametrize("ratio", ic.GATE_RATIOS)
def test_gates_sit_on_their_side(oracle, ratio):
    s = ic.crafted("gates")
    m, om = assert_model_is_oracle(oracle, s, ratio=ratio, ori=False)
    want = ic.gate_expect(ratio)
    assert [bool(v >= 0) for v in om] == want
    # the sides the issue names: 50 in, 51 out, every product on an integer out, a lone candidate in
    by = dict(zip(ic.GATES, want))
    assert by[(50, None)] and not by[(51, None)] and not by[(12, "=")]
    if ratio == 0.9:
        assert not any(by[g] for g in [(9, 10), (18, 20), (45, 50), (27, 30)]) and by[(7, 10)]
    if ratio == 0.7:
        assert not any(by[g] for g in [(7, 10), (14, 20), (35, 50)]) and by[(6, 10)]
    if ratio == 0.6:
        assert not by[(6, 10)]


def test_size_edges_model_is_oracle(oracle):
    """Every (nq0, nr0) of the size edges: the model equals the oracle; the set reaches need == 1,
    queries without candidates, picks that move after round 0 and a few claim-slot overflows (the whole-list scans
    are the crafted scenes' business)."""
    seen = dict(need1=0, scans=0, empty=0, rounds=0, matches=0, overflows=0)
    for nq0 in ic.SIZES_Q:
        for nr0 in ic.SIZES_R:
            s = ic.sized(nq0, nr0)
            m, om = assert_model_is_oracle(oracle, s)
            assert (m["nq0"], m["nr0"]) == (nq0, nr0) and len(s["k1"]) > nq0 and len(s["k2"]) > nr0 + 2
            assert m["form"] in (0, 1)      # (many queries on few keypoints overflow the claim slots)
            seen["need1"] += m["need1"]; seen["scans"] += m["full_scans"]; seen["matches"] += m["n"]
            seen["empty"] += sum(1 for n in m["lens"] if n == 0)
            seen["rounds"] = max(seen["rounds"], m["rounds"] or 0)
            seen["overflows"] += m["form"] == 1
    print(f"INIT_SIZE_EDGES {seen}")
    assert seen["need1"] > 50 and seen["empty"] > 100 and seen["rounds"] >= 2, seen
    assert seen["matches"] > 200 and 0 < seen["overflows"] < 30, seen


def test_envelope_arithmetic():
    """init_search's envelope from a call's sizes: 4 * (nr0 + nq0) + 16 bytes of LDS up to 150 KiB,
    nq0 * list_cap up to 2^28, at most 65535 keypoints a frame."""
    ok = init_route(4, 38392, 4, 38392)
    assert ok == {"rc": 0, "lds": 150 * 1024, "list_cap": 38400, "cap": 6}
    assert init_route(5, 38392, 5, 38392)["rc"] == ERR_UNSUPPORTED
    assert init_route(4, 38393, 4, 38393)["rc"] == ERR_UNSUPPORTED
    r = init_route(19000, 19000, 19000, 19000)      # LDS 152016 bytes fits; 19000 * 19008 > 2^28
    assert r["lds"] <= 150 * 1024 and r["list_cap"] == 19008 and 19000 * r["list_cap"] > 2 ** 28
    assert r["rc"] == ERR_UNSUPPORTED
    assert init_route(14122, 19008, 14122, 19008)["rc"] == 0 and 14122 * 19008 <= 2 ** 28 < 14123 * 19008
    assert init_route(14123, 19008, 14123, 19008)["rc"] == ERR_UNSUPPORTED
    assert init_route(65535, 65535, 0, 0)["rc"] == 0
    assert init_route(65536, 10, 5, 5)["rc"] == ERR_ARG and init_route(10, 65536, 5, 5)["rc"] == ERR_ARG
    assert init_route(10, 10, 0, 0) == {"rc": 0, "lds": 16, "list_cap": 64, "cap": 2}
    assert init_route(100, 100, 62, 65)["cap"] == 64 and init_route(100, 100, 61, 64)["cap"] == 63
    assert init_route(100, 100, 61, 64)["list_cap"] == 64 and init_route(100, 100, 62, 65)["list_cap"] == 128
