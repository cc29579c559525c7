"""SearchForInitialization on the device at the limits of its routes: the crafted scenes of
tests/init_cases.py (their preconditions are asserted on the CPU in tests/test_init_routes.py) in
both forms (the parallel rounds, and the chain by ORBHIP_INIT_CHAIN), the size edges, the gates, one
context through short and long searches in turn, and the envelope. Every comparison is with the
oracle and exact (matches12, nmatches, the updated vbPrevMatched); every test asserts the route it
ran on through orbhip_test_init_stats against the model of tests/init_cases.py."""
import functools

import numpy as np
import pytest

import init_cases as ic
from helpers import init_stats
from orb_slam3_ros2_amd._lib import KP_DTYPE, Context, OrbHipError
from orb_slam3_ros2_amd.matcher import ORBmatcher
from test_init_routes import ERR_ARG, ERR_UNSUPPORTED, oracle_init

pytestmark = pytest.mark.gpu


@pytest.fixture(params=["rounds", "chain"])
def form(request, monkeypatch):
    monkeypatch.delenv("ORBHIP_INIT_CHAIN", raising=False)
    if request.param == "chain":
        monkeypatch.setenv("ORBHIP_INIT_CHAIN", "1")
    return request.param


@pytest.fixture
def default_form(monkeypatch):
    monkeypatch.delenv("ORBHIP_INIT_CHAIN", raising=False)


@pytest.fixture(scope="module")
def ctx():
    c = Context()
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def crafted_model(name, ratio, ori):
    return ic.model(ic.crafted(name), ratio, ori)


@functools.lru_cache(maxsize=None)
def sized_case(nq0, nr0):
    s = ic.sized(nq0, nr0)
    return s, ic.model(s)


def run(ctx, oracle, s, ratio=None, ori=True):
    """The device call, equal to the oracle; returns (n, matches12, prev) and the call's stats."""
    ratio = s["ratio"] if ratio is None else ratio
    got = ORBmatcher(ratio, ori, ctx=ctx).SearchForInitialization(s["k1"], s["d1"], s["k2"], s["d2"], s["prev"],
                                                                  s["window"], bounds2=s["bounds"])
    want = oracle_init(oracle, s, ratio, ori)
    assert got[0] == want[0], (got[0], want[0])
    assert np.array_equal(got[1], want[1]), np.nonzero(got[1] != want[1])[0][:10]
    assert got[2].tobytes() == want[2].tobytes()
    return got, init_stats(ctx)


def assert_route(st, m, form):
    """The hook's figures against the model's: the sizes and need counts in both forms; the form,
    and the round that changed nothing (the cap where none did), in the default form."""
    assert (st["nq0"], st["nr0"], st["need1"], st["need2"]) == (m["nq0"], m["host_nr0"], m["need1"], m["need2"]), (st, m["form"])
    if form == "chain":
        assert (st["form"], st["round"]) == (3, 0), st
        return
    assert st["form"] == m["form"], (st, m["form"], m["rounds"])
    if m["form"] == 0:
        assert st["round"] == m["rounds"], (st, m["rounds"])
    elif m["form"] == 2:
        assert st["round"] == m["cap"], (st, m["cap"])
    else:
        assert m["overflow_round"] < st["round"] <= m["cap"], (st, m["overflow_round"])


@pytest.mark.parametrize("ori", [True, False])
@pytest.mark.parametrize("name", list(ic.CRAFTED))
def test_crafted_scene(ctx, oracle, form, name, ori):
    """Lost entries (need == 2), fewer than two eligible among the 16 (need == 1), the dependency
    chain to the round cap and past it, 7 / 8 / 9 / 16 claimants of one rank, the window and grid
    boundaries: equal to the oracle, on the route the model predicts."""
    s = ic.crafted(name)
    (n, m12, _), st = run(ctx, oracle, s, ori=ori)
    for i1, i2 in s["expect"].items():
        assert m12[i1] == i2, (i1, m12[i1], i2)
    assert_route(st, crafted_model(name, s["ratio"], ori), form)


@pytest.mark.parametrize("ratio", ic.GATE_RATIOS)
def test_gates(ctx, oracle, form, ratio):
    """d1 <= 50 from both sides; (float)d1 < (float)d2 * nnratio at products on an integer."""
    s = ic.crafted("gates")
    (n, m12, _), st = run(ctx, oracle, s, ratio=ratio, ori=False)
    assert [bool(v >= 0) for v in m12] == ic.gate_expect(ratio)
    assert_route(st, crafted_model("gates", ratio, False), form)


@pytest.mark.parametrize("nq0", ic.SIZES_Q)
def test_size_edges(ctx, oracle, form, nq0):
    """Blocks of 4 queries (the chain), 4 per wave and 16 per work-group (the rounds), ranks in
    strides of 64: every size around them, with octaves interleaved and keypoints off the grid."""
    for nr0 in ic.SIZES_R:
        s, m = sized_case(nq0, nr0)
        _, st = run(ctx, oracle, s)
        assert_route(st, m, form)


def test_history_independence(oracle, default_form):
    """Long and short searches in turn on ONE context (init_ahead adapts to the last call, the three
    claim tables and the flags are laid out anew in a reused block): each result equals the oracle's
    and, bit for bit, the same call on a fresh context; init_ahead follows the host's rule."""
    steps = [("chain-63", None), (None, (17, 65)), ("chain-5", None), ("chain-64", None), ("lost-lane7-pad1", None),
             ("chain-63", None)]
    shared = Context()
    try:
        assert init_stats(shared) == {"form": -1, "round": 0, "init_ahead": 6, "nq0": 0, "nr0": 0, "need1": -1,
                                      "need2": -1}
        ahead = 6
        for i, (name, size) in enumerate(steps):
            s, m = (ic.crafted(name), crafted_model(name, 0.9, True)) if name else sized_case(*size)
            got, st = run(shared, oracle, s)
            assert_route(st, m, "rounds")
            ahead = ic.ahead_after(ahead, m)
            assert st["init_ahead"] == ahead, (i, st, ahead)
            fresh = Context()
            try:
                alone, st2 = run(fresh, oracle, s)
            finally:
                fresh.close()
            assert got[0] == alone[0] and got[1].tobytes() == alone[1].tobytes() and got[2].tobytes() == alone[2].tobytes(), i
            assert st2["init_ahead"] == ic.ahead_after(6, m), (i, st2)
            assert {k: v for k, v in st.items() if k != "init_ahead"} == {k: v for k, v in st2.items() if k != "init_ahead"}
    finally:
        shared.close()


# ---- the envelope ----

def _frame(n, rng, octave0):
    k = np.zeros(n, KP_DTYPE)
    k["x"], k["y"] = rng.uniform(1.0, 638.0, n).astype(np.float32), rng.uniform(1.0, 478.0, n).astype(np.float32)
    k["angle"] = rng.uniform(0, 360, n).astype(np.float32)
    k["size"], k["response"] = 31.0, 50.0
    k["octave"] = 1
    k["octave"][:octave0] = 0
    return k


@functools.lru_cache(maxsize=None)
def _envelope_scene():
    """4 queries against 38392 ranked keypoints at random places: 4 * (38392 + 4) + 16 = 150 KiB."""
    rng = np.random.default_rng(38392)
    k2 = _frame(38392, rng, 38392)
    d2 = rng.integers(0, 256, (38392, 32), dtype=np.uint8)
    src = [5, 20000, 38391, 777]
    k1 = k2[src].copy()
    k1["x"] += 2.0
    d1 = np.stack([ic.flip_low_bits(d2[j], 3 * i) for i, j in enumerate(src)])
    return ic.scene(k1, d1, k2, d2, np.stack([k1["x"], k1["y"]], 1), 100)


def test_envelope_largest_call(ctx, oracle, form):
    s = _envelope_scene()
    (n, m12, _), st = run(ctx, oracle, s)
    assert n == 4 and (st["nq0"], st["nr0"]) == (4, 38392) and st["form"] == (0 if form == "rounds" else 3), st


def test_envelope_refusals(ctx, oracle, default_form):
    """One query too many for the LDS, 19000 x 19000 (the 2^28 list entries), 65536 keypoints on
    either side: refused with the code the envelope names, and the context serves the next call."""
    small = ic.crafted("chain-5")
    big = _envelope_scene()
    rng = np.random.default_rng(5)
    k5 = np.concatenate([big["k1"], big["k1"][:1]])
    d5 = np.concatenate([big["d1"], big["d1"][:1]])

    def call(k1, d1, k2, d2):
        return ORBmatcher(0.9, True, ctx=ctx).SearchForInitialization(k1, d1, k2, d2, np.stack([k1["x"], k1["y"]], 1), 100)
    k19, d19 = _frame(19000, rng, 19000), rng.integers(0, 256, (19000, 32), dtype=np.uint8)
    k64, d64 = _frame(65536, rng, 10), rng.integers(0, 256, (65536, 32), dtype=np.uint8)
    for args, code in [((k5, d5, big["k2"], big["d2"]), ERR_UNSUPPORTED), ((k19, d19, k19, d19), ERR_UNSUPPORTED),
                       ((k64, d64, k19, d19), ERR_ARG), ((k19[:100], d19[:100], k64, d64), ERR_ARG)]:
        with pytest.raises(OrbHipError) as e:
            call(*args)
        assert e.value.code == code
        assert init_stats(ctx)["form"] == -1
        _, st = run(ctx, oracle, small)
        assert (st["form"], st["round"]) == (0, 5), st
