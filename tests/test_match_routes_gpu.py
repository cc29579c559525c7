"""GPU parity of the Hamming brute-force matcher on every dispatch route and size edge, against
the oracle and exact (match, best, second and the count; no tolerances). Data sets carry their
matches by construction (tests/helpers.planted_match_set). Every test asserts the route its shape
takes (tests/helpers.match_route, the function run_match itself follows), and every checked call
follows a call on DIFFERENT data of the same shape and route: the chunk partials live in context
scratch that persists between calls, so a skipped work-group would otherwise leave the right
answer behind.

Routes reached here (run_match, csrc/match_kernels.hip):
  k_match_fused (<= 4 pairs)                        every test on the "fused" path
  k_match_top2<64> + k_match_finish ("small")       the host-call tests on the "two-kernel" path
  k_match_top2<256>, xrun 0 (5-7 pairs, one big pair)  test_ties (batch), test_large_sides[2048x4096],
                                                    test_batches[5 pairs]
  k_match_top2<256>, xrun > 0 (>= 8 pairs)          test_batches[9 pairs] (xcd_runs tail), [16 pairs]
  k_match_top2<512> / <1024> (ORBHIP_MATCH_TC)      test_ties, test_batches[9 pairs-tc512 / -tc1024]
  ORBHIP_MATCH_XCD=0                                test_batches[9 pairs-xcd0]
  8-byte partials (pk 0) and the 14-bit edge        test_large_sides[130x16383 / 130x16384]
  k_match_finish nq > kFinQ, nt > kFinQ             test_large_sides[6214x320 / 200x6200]
  orbhip_match_frames_device                        test_frames_device
  nq = 0, nt = 1, bad arguments on the host call    test_size_edges, test_host_call_edges
  nq = 0 / nt = 0 / nt = 1 for one pair of a batch  test_batches[9 pairs]"""
import ctypes
import functools

import numpy as np
import pytest

from tests.helpers import MATCH_HIST_IDS as HIST_IDS, MATCH_HISTOGRAMS as HISTOGRAMS, match_route, planted_match_set

pytestmark = pytest.mark.gpu
_SWITCHES = ("ORBHIP_MATCH_UNFUSED", "ORBHIP_MATCH_TC", "ORBHIP_MATCH_XCD", "ORBHIP_GRAPH")


@pytest.fixture(params=["fused", "two-kernel"])
def match_path(request, monkeypatch):
    """The one-launch k_match_fused (the default up to 4 pairs) or k_match_top2 + k_match_finish
    (ORBHIP_MATCH_UNFUSED=1). The other switches are cleared: a captured graph (ORBHIP_GRAPH) would
    pin the first route."""
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    if request.param == "two-kernel":
        monkeypatch.setenv("ORBHIP_MATCH_UNFUSED", "1")
    return request.param


@pytest.fixture
def env(monkeypatch):
    for k in _SWITCHES:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.fixture(scope="module")
def matcher():
    from orb_slam3_ros2_amd import ORBmatcher
    return ORBmatcher(0.9, True)


def _expect_route(path, npairs, max_q, max_t, kernel, **more):
    r = match_route(npairs, max_q, max_t)
    if path == "fused":
        assert r["kernel"] == "fused", r
    else:
        assert r["kernel"] == kernel and all(r[k] == v for k, v in more.items()), r
    return r


def _check(matcher, oracle, ds, th=50, ratio=0.9, ori=True):
    """One host call against the oracle; returns (n, match, best, second)."""
    matcher.mfNNratio, matcher.mbCheckOrientation = ratio, ori
    n, m, b, s = matcher.match_bf(ds.q, ds.qa, ds.t, ds.ta, th)
    on, om, ob, os_ = oracle.match_bf(ds.q, ds.qa, ds.t, ds.ta, th, ratio, ori)
    assert np.array_equal(b, ob) and np.array_equal(s, os_)
    assert np.array_equal(m, om) and n == on
    return n, m, b, s


def _run(matcher, ds, th=50, ratio=0.9, ori=True):
    matcher.mfNNratio, matcher.mbCheckOrientation = ratio, ori
    return matcher.match_bf(ds.q, ds.qa, ds.t, ds.ta, th)


def _spread(n, bins=(2, 5, 9, 12)):
    """n planted queries over four bins of falling weight, so the rotation filter drops the last."""
    c = [n - n // 4 - n // 5 - n // 10, n // 4, n // 5, n // 10]
    return {b: k for b, k in zip(bins, c) if k > 0}


# ---- a. size edges, host call ----

# every nq in {1, 15, 16, 17, 63, 64, 65, 1025} and every nt in {1, 2, 15, 16, 17, 63, 64, 65, 255,
# 256, 257, 1023, 1024, 1025, 2049}: the strides of the kernels are 16 (fused queries per
# work-group, tc64 trains per wave), 64 (fused slices, queries per top2 block, tc64 chunk), 256
# (tc256 chunk), 1024 (fused LDS chunk and work-group; the finish kernel's threads)
SIZE_EDGES = [(1, 1), (15, 2), (16, 15), (17, 16), (63, 17), (64, 63), (65, 64), (1025, 65), (1, 255), (15, 256),
              (16, 257), (17, 1023), (63, 1024), (64, 1025), (65, 2049), (1025, 1025)]


@pytest.mark.parametrize("nq,nt", SIZE_EDGES, ids=[f"{a}x{b}" for a, b in SIZE_EDGES])
def test_size_edges(matcher, oracle, match_path, nq, nt):
    """k_match_fused and k_match_top2<64> + finish at and around their strides; about half of the
    queries planted with 0..60 flips (both sides of TH_LOW), rotation filter on and off. nt = 1:
    second stays 256."""
    _expect_route(match_path, 1, nq, nt, "tc64", nch=(nt + 63) // 64, xrun=0, pk=1)
    a = planted_match_set(nq, nt, _spread((nq + 1) // 2), (0, 60), seed=1000 + nq + nt)
    b = planted_match_set(nq, nt, _spread((nq + 1) // 2), (0, 60), seed=2000 + nq + nt)
    for ori in (True, False):
        _run(matcher, a, ori=ori)
        n, m, best, second = _check(matcher, oracle, b, ori=ori)
        assert (best[b.planted] == b.flips[b.planted]).all()
        if nt == 1:
            assert (second == 256).all()
        _check(matcher, oracle, a, ori=ori)


def test_host_call_edges(matcher, oracle, match_path):
    """orbhip_match_bf: nq = 0 returns 0 and touches nothing; negative counts and null pointers are
    ORBHIP_ERR_ARG; nt = 0 leaves best = second = 256 and no match (the oracle's answer too)."""
    from orb_slam3_ros2_amd._lib import lib, ptr
    L, h = lib(), matcher.ctx.handle
    ds = planted_match_set(5, 9, {0: 3}, seed=3)
    m = np.full(5, 77, np.int32); b = np.full(5, 78, np.int32); s = np.full(5, 79, np.int32)

    def call(q=ds.q, qa=ds.qa, nq=5, t=ds.t, ta=ds.ta, nt=9, ctx=h, mm=m, bb=b, ss=s):
        return L.orbhip_match_bf(ctx, ptr(q), ptr(qa), nq, ptr(t), ptr(ta), nt, 50, ctypes.c_float(0.9), 1, ptr(mm),
                                 ptr(bb), ptr(ss))
    assert call(nq=0) == 0
    assert (m == 77).all() and (b == 78).all() and (s == 79).all()
    assert call(nq=0, q=None, qa=None, mm=None, bb=None, ss=None) == 0
    for bad in (dict(nq=-1), dict(nt=-1), dict(ctx=None), dict(q=None), dict(qa=None), dict(t=None), dict(ta=None),
                dict(mm=None), dict(bb=None), dict(ss=None)):
        assert call(**bad) == -1, bad          # ORBHIP_ERR_ARG
    assert (m == 77).all() and (b == 78).all() and (s == 79).all()
    assert call() == 3 and np.array_equal(m, ds.train)
    assert call(nt=0, t=None, ta=None) == 0
    on, om, ob, os_ = oracle.match_bf(ds.q, ds.qa, ds.t[:0], ds.ta[:0], 50, 0.9, True)
    assert on == 0 and np.array_equal(m, om) and np.array_equal(b, ob) and np.array_equal(s, os_)
    assert (b == 256).all() and (s == 256).all() and (m == -1).all()


# ---- b. ties and merge order ----

# (a, b) straddle: fused slices (0, 1), fused waves (3, 4), tc64 wave quarters (15, 16), tc64 chunks /
# tc256 quarters / the 64 fused slices (63, 64), one fused slice twice (5, 69), tc512 quarters (127, 128),
# tc256 chunks / tc1024 quarters (255, 256), tc512 chunks (511, 512), tc1024 and fused LDS chunks
# (1023, 1024), (2047, 2048), first and last train (0, 2099)
TIE_PAIRS = [(0, 1), (3, 4), (15, 16), (63, 64), (5, 69), (127, 128), (255, 256), (511, 512), (1023, 1024),
             (2047, 2048), (0, 2099)]
TIE_NT, TIE_NQ = 2100, 48


@functools.lru_cache(maxsize=None)
def _tie_sets():
    """Kind 1: the same descriptor at trains a and b (expect a, second == best). Kind 2: distance
    d + 1 at a and d at b (expect b, second == d + 1). A train index can serve one query only, so
    the cases are dealt into data sets with disjoint indices, all over the same 2100 random trains
    with the same query count. Returns [(set, [(query, expected match, best, second)])]."""
    cases = [(a, b, kind) for kind in (1, 2) for (a, b) in TIE_PAIRS]
    groups = []
    for c in cases:
        for g in groups:
            if not any({c[0], c[1]} & {o[0], o[1]} for o in g):
                g.append(c)
                break
        else:
            groups.append([c])
    rng = np.random.default_rng(77)
    base = (rng.integers(0, 256, (TIE_NT, 32), dtype=np.uint8), rng.integers(0, 360, TIE_NT).astype(np.float32))
    out = []
    for gi, g in enumerate(groups):
        plants, expect = [], []
        for qi, (a, b, kind) in enumerate(g):
            d = 3 + (qi * 7 + gi) % 40        # 3 .. 42 flips: best > 0 and below TH_LOW
            q = 2 * qi + 1                    # odd query slots; the others stay random
            if kind == 1:
                plants += [(q, a, d), (q, b, d)]
                expect.append((q, a, d, d))
            else:
                plants += [(q, a, d + 1), (q, b, d)]
                expect.append((q, b, d, d + 1))
        out.append((planted_match_set(TIE_NQ, TIE_NT, None, seed=500 + gi, plants=plants, trains=base), expect))
    assert sum(len(e) for _, e in out) == 2 * len(TIE_PAIRS)
    return out


def _assert_ties(expect, m, b, s):
    for q, em, eb, es in expect:
        assert (m[q], b[q], s[q]) == (em, eb, es), (q, em, eb, es, m[q], b[q], s[q])


def test_ties_host(matcher, oracle, match_path):
    """First index wins and `second` is the multiset second across every merge of k_match_fused
    and of k_match_top2<64> + finish (ratio 1.01, so a tie best == second is accepted)."""
    _expect_route(match_path, 1, TIE_NQ, TIE_NT, "tc64", nch=33)
    sets = _tie_sets()
    _run(matcher, sets[-1][0], ratio=1.01)
    for ds, expect in sets:             # each call follows one on another set of the same shape
        n, m, b, s = _check(matcher, oracle, ds, ratio=1.01)
        _assert_ties(expect, m, b, s)
        assert n == len(expect)


def _to_dev(frames, cap, pad_from_prev=True):
    """[(desc (n, 32), angle (n,))] -> kps (B, cap, 6), desc (B, cap, 32), n (B,) device tensors.
    The rows past a frame's count are NOT blank: descriptors copy the previous frame's (the
    queries that frame is a train set for), so a kernel that read past nt would find distance 0."""
    import torch
    B = len(frames)
    rng = np.random.default_rng(9)
    kps = rng.uniform(0, 360, (B, cap, 6)).astype(np.float32)
    desc = rng.integers(0, 256, (B, cap, 32), dtype=np.uint8)
    n = np.zeros(B, np.int32)
    for f, (d, a) in enumerate(frames):
        n[f] = len(d)
        if pad_from_prev and f > 0 and len(frames[f - 1][0]):
            pd, pa = frames[f - 1]
            idx = np.arange(cap - n[f]) % len(pd)
            desc[f, n[f]:] = pd[idx]
            kps[f, n[f]:, 3] = pa[idx]
        desc[f, :n[f]] = d
        kps[f, :n[f], 3] = a
    dev = torch.device("cuda:0")
    return torch.from_numpy(kps).to(dev), torch.from_numpy(desc).to(dev), torch.from_numpy(n).to(dev)


def _garbage_out(npairs, cap):
    """Stale outputs that would read as results: bin-0 tentative indices, plausible distances."""
    import torch
    dev = torch.device("cuda:0")
    mm = torch.arange(cap, dtype=torch.int32, device=dev).repeat(npairs, 1)
    return mm, torch.full_like(mm, 7), torch.full_like(mm, 3), torch.full((npairs,), 12345, dtype=torch.int32,
                                                                          device=dev)


def _check_pairs(oracle_refs, frames, out):
    mm, bb, ss, nm = (x.cpu().numpy() for x in out)
    for p, (on, om, ob, os_) in enumerate(oracle_refs):
        nq = len(frames[p][0])
        assert nm[p] == on, p
        assert np.array_equal(mm[p, :nq], om), p
        assert np.array_equal(bb[p, :nq], ob) and np.array_equal(ss[p, :nq], os_), p


def _oracle_pairs(oracle, frames, th, ratio, ori):
    return [oracle.match_bf(frames[p][0], frames[p][1], frames[p + 1][0], frames[p + 1][1], th, ratio, ori)
            for p in range(len(frames) - 1)]


@functools.lru_cache(maxsize=None)
def _tie_batch():
    from oracle import pyoracle
    sets = _tie_sets()
    frames = [x for ds, _ in sets for x in ((ds.q, ds.qa), (ds.t, ds.ta))]
    warm = frames[2:] + frames[:2]            # the same shapes, every pair another data set
    return sets, frames, warm, _oracle_pairs(pyoracle, frames, 50, 1.01, True)


@pytest.mark.parametrize("tc", [256, 512, 1024])
def test_ties_batch(oracle, env, tc):
    """The tie sets as one batch [Q0, T0, Q1, T1, ...] on k_match_top2<256> (5-7 pairs, xrun 0)
    and, through ORBHIP_MATCH_TC, <512> and <1024>: every pair (the T -> Q ones too) against the
    oracle, and the Q -> T ones against what they were built to give."""
    import torch
    from orb_slam3_ros2_amd import ORBmatcher
    sets, frames, warm, refs = _tie_batch()
    npairs = len(frames) - 1
    assert 5 <= npairs <= 7
    if tc != 256:
        env.setenv("ORBHIP_MATCH_TC", str(tc))
    r = match_route(npairs, TIE_NT, TIE_NT)
    assert r == {"kernel": f"tc{tc}", "nch": -(-TIE_NT // tc), "xrun": 0, "pk": 1}, r
    mt = ORBmatcher(1.01, True)
    out = _garbage_out(npairs, TIE_NT)
    mt.match_pairs_device(*_to_dev(warm, TIE_NT), *out)
    torch.cuda.synchronize()
    out = _garbage_out(npairs, TIE_NT)
    mt.match_pairs_device(*_to_dev(frames, TIE_NT), *out)
    torch.cuda.synchronize()
    _check_pairs(refs, frames, out)
    mm, bb, ss, nm = (x.cpu().numpy() for x in out)
    for i, (ds, expect) in enumerate(sets):
        _assert_ties(expect, mm[2 * i], bb[2 * i], ss[2 * i])
        assert nm[2 * i] == len(expect)


# ---- c. acceptance boundaries and ComputeThreeMaxima ----

def test_acceptance_boundaries(matcher, oracle, match_path):
    """best <= th_low (50 in, 51 out) and (float)best < ratio * (float)second: with a second of 50
    and ratio 0.9f the product is 45.0f, so best 44 is in and 45 is out."""
    _expect_route(match_path, 1, 64, 700, "tc64", nch=11)
    plants = [(0, 10, 50), (1, 20, 51), (2, 30, 44), (2, 31, 50), (3, 40, 45), (3, 41, 50)]
    ds = planted_match_set(64, 700, {0: 20}, (0, 40), seed=8, plants=plants)
    other = planted_match_set(64, 700, {0: 20}, (0, 40), seed=9, plants=plants)
    assert np.float32(0.9) * np.float32(50) == np.float32(45)
    _run(matcher, other)
    n, m, b, s = _check(matcher, oracle, ds)
    assert list(m[:4]) == [10, -1, 30, -1] and list(b[:4]) == [50, 51, 44, 45] and list(s[2:4]) == [50, 50]
    expect = ds.train.copy()
    expect[[1, 3]] = -1
    assert n == 22 and np.array_equal(m, expect)


@pytest.mark.parametrize("hist,keep,kept", HISTOGRAMS, ids=HIST_IDS)
def test_three_maxima(matcher, oracle, match_path, hist, keep, kept):
    """ComputeThreeMaxima on the device (three_maxima_wave, both kernels): tie order, the 10 % rule
    at its float boundary, fewer than three occupied bins, and bin 12, the last one rot * (1/30)
    can reach. The kept count and the exact match array are the construction's, not only the
    oracle's."""
    _expect_route(match_path, 1, 300, 700, "tc64", nch=11)
    ds = planted_match_set(300, 700, hist, (0, 40), seed=31)
    _run(matcher, planted_match_set(300, 700, {1: 60, 6: 50, 10: 40, 12: 30}, (0, 40), seed=32))
    n, m, b, s = _check(matcher, oracle, ds)
    assert n == kept and np.array_equal(m, np.where(np.isin(ds.bin, keep), ds.train, -1))
    n, m, b, s = _check(matcher, oracle, ds, ori=False)
    assert n == sum(hist.values()) and np.array_equal(m, ds.train)


def test_histograms_back_to_back(oracle, match_path):
    """Two different histograms and then a call without the rotation filter on one fresh context:
    the fused kernel's sync words (done counter, histogram, count) are reset by every launch."""
    from orb_slam3_ros2_amd import ORBmatcher
    mt = ORBmatcher(0.9, True)
    _expect_route(match_path, 1, 300, 700, "tc64")
    a = planted_match_set(300, 700, HISTOGRAMS[0][0], (0, 40), seed=41)
    b = planted_match_set(300, 700, HISTOGRAMS[5][0], (0, 40), seed=42)
    for rep in range(2):
        assert _check(mt, oracle, a)[0] == HISTOGRAMS[0][2]
        assert _check(mt, oracle, b)[0] == HISTOGRAMS[5][2]
        assert _check(mt, oracle, b, ori=False)[0] == 130
        assert _check(mt, oracle, a, ori=False)[0] == 160


# ---- d. large-side branches ----

def _large(nq, nt, seed):
    top = nt - 1
    plants = [(1, 0, 4), (3, top, 5), (5, top - 1, 6), (7, 1, 9), (7, top - 2, 9)]   # query 7: a tie (second == best: the ratio rejects it)
    if nt > 6144 + 40:
        plants += [(9 + 2 * i, 6145 + 3 * i, 10 + i) for i in range(12)]
    # the explicit plants sit in bin 0: the heaviest bin here, so the rotation filter keeps them
    return planted_match_set(nq, nt, _spread(nq // 2, (0, 5, 9, 12)), (0, 60), seed=seed, plants=plants)


LARGE = [(6214, 320, "tc64", 5, 1), (200, 6200, "tc64", 97, 1), (130, 16383, "tc64", 256, 1),
         (130, 16384, "tc64", 256, 0), (2048, 4096, "tc256", 16, 1)]


@pytest.mark.parametrize("nq,nt,kernel,nch,pk", LARGE, ids=[f"{c[0]}x{c[1]}" for c in LARGE])
def test_large_sides(matcher, oracle, match_path, nq, nt, kernel, nch, pk):
    """k_match_finish past its LDS capacity kFinQ = 6144 (nq = 6214: matches re-read through
    global match[]; nt = 6200: train angles from global, and more than 16 chunks per query); the
    4-byte partial format at its last index (nt = 16383: index 16382 next to the sentinel 0x3FFF)
    and the 8-byte format (nt = 16384, best at 16383); one pair large enough for k_match_top2<256>.
    Bests are planted at trains 0, 1, nt - 3, nt - 2 and nt - 1."""
    _expect_route(match_path, 1, nq, nt, kernel, nch=nch, xrun=0, pk=pk)
    ds, other = _large(nq, nt, 600), _large(nq, nt, 601)
    if nq > 6144:
        assert (ds.planted[:6144]).any() and (ds.planted[6144:]).sum() > 10
    if nt > 6144:
        assert (ds.train > 6144).sum() > 10
    _run(matcher, other)
    n, m, b, s = _check(matcher, oracle, ds)
    assert list(m[[1, 3, 5, 7]]) == [0, nt - 1, nt - 2, -1]
    assert list(b[[1, 3, 5, 7]]) == [4, 5, 6, 9] and s[7] == 9
    assert n > nq // 8
    _check(matcher, oracle, other, ori=False)


# ---- e. batches on device tensors ----

def _chain(counts, seed):
    """Frames of the given keypoint counts, frame f planted from frame f + 1 (its train set in pair
    f): about half of its queries, 0..60 flips."""
    frames = [None] * len(counts)
    nxt = None
    for f in range(len(counts) - 1, -1, -1):
        n = counts[f]
        if nxt is None or len(nxt[0]) == 0:
            rng = np.random.default_rng(seed + f)
            frames[f] = (rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 360, n).astype(np.float32))
        else:
            ds = planted_match_set(n, len(nxt[0]), _spread(n // 2), (0, 60), seed=seed + f, trains=nxt)
            frames[f] = (ds.q, ds.qa)
        nxt = frames[f]
    return frames


BATCHES = {
    # 9 pairs of 16 x 4 work-groups = 576: one full xcd_runs round of 512 and a tail of 64; pairs with
    # nt = 0 (0), nq = 0 and nt = 1 (1), nq = 1 (2), counts on and around the block sizes
    "9 pairs": (1024, [1024, 0, 1, 63, 64, 65, 1000, 1024, 257, 513]),
    "16 pairs": (1024, [1024, 1000, 900, 1024, 777, 1024, 1023, 1, 1024, 512, 1024, 640, 1024, 999, 1024, 65, 1024]),
    "5 pairs": (1536, [1536, 1300, 1025, 1536, 17, 1536]),
}
# (a data seed of its own for every case: a fresh context may be handed the scratch a previous test
# freed, and partials left there by the same data in the same layout would be right ones)
BATCH_CASES = [("9 pairs", 1, {}, "tc256", 4, 64), ("9 pairs", 2, {"ORBHIP_MATCH_XCD": "0"}, "tc256", 4, 0),
               ("9 pairs", 3, {"ORBHIP_MATCH_TC": "512"}, "tc512", 2, 32),
               ("9 pairs", 4, {"ORBHIP_MATCH_TC": "1024"}, "tc1024", 1, 16),
               ("16 pairs", 5, {}, "tc256", 4, 64), ("5 pairs", 6, {}, "tc256", 6, 0)]


@functools.lru_cache(maxsize=None)
def _batch(name, seed):
    from oracle import pyoracle
    cap, counts = BATCHES[name]
    frames, warm = _chain(counts, 7000 + 100 * seed), _chain(counts, 8000 + 100 * seed)
    return cap, frames, warm, _oracle_pairs(pyoracle, frames, 50, 0.9, True)


@pytest.mark.parametrize("name,seed,switches,kernel,nch,xrun", BATCH_CASES,
                         ids=["9 pairs", "9 pairs-xcd0", "9 pairs-tc512", "9 pairs-tc1024", "16 pairs", "5 pairs"])
def test_batches(oracle, env, name, seed, switches, kernel, nch, xrun):
    """match_pairs_device on synthetic tensors: k_match_top2<256> with the xcd_runs remap (with a
    tail and without), in dispatch order (ORBHIP_MATCH_XCD=0, and 5 pairs), <512> and <1024>; per
    pair match[:nq], best[:nq], second[:nq] and nmatch against the oracle (rows past nq are
    unspecified)."""
    import torch
    from orb_slam3_ros2_amd import ORBmatcher
    for k, v in switches.items():
        env.setenv(k, v)
    cap, frames, warm, refs = _batch(name, seed)
    npairs = len(frames) - 1
    assert match_route(npairs, cap, cap) == {"kernel": kernel, "nch": nch, "xrun": xrun, "pk": 1}
    mt = ORBmatcher(0.9, True)
    out = _garbage_out(npairs, cap)
    mt.match_pairs_device(*_to_dev(warm, cap), *out)
    torch.cuda.synchronize()
    out = _garbage_out(npairs, cap)
    mt.match_pairs_device(*_to_dev(frames, cap), *out)
    torch.cuda.synchronize()
    _check_pairs(refs, frames, out)
    assert sum(r[0] for r in refs) > 100 * (npairs - 3)


# ---- f. two frames in separate allocations ----

FRAME_CASES = [(1000, 1000, 1024), (17, 1025, 1536), (0, 500, 1024), (500, 0, 1024)]


@pytest.mark.parametrize("nq,nt,cap", FRAME_CASES, ids=[f"{a}x{b}" for a, b, _ in FRAME_CASES])
def test_frames_device(oracle, match_path, nq, nt, cap):
    """orbhip_match_frames_device (the front-end's call): out_stride 0, query and train buffers in
    separate allocations, nq and nt device scalars; fused and two-kernel, garbage-prefilled
    outputs, an empty query set and an empty train set."""
    import torch
    from orb_slam3_ros2_amd import ORBmatcher
    _expect_route(match_path, 1, cap, cap, "tc64", nch=cap // 64, xrun=0, pk=1)
    mt = ORBmatcher(0.9, True)
    chains = [_chain([nq, nt], 9000 + nq), _chain([nq, nt], 9500 + nq)]
    on, om, ob, os_ = oracle.match_bf(*chains[1][0], *chains[1][1], 50, 0.9, True)
    for frames in chains:
        qk, qd, qn = _to_dev(frames[:1], cap)
        tk, td, tn = _to_dev([frames[0], frames[1]], cap)      # the train rows past nt copy the queries
        tk, td, tn = tk[1].clone(), td[1].clone(), tn[1:2].clone()
        mm, bb, ss, nm = _garbage_out(1, cap)
        mt.match_frames_device(qk[0], qd[0], qn, tk, td, tn, mm[0], bb[0], ss[0], nm)
        torch.cuda.synchronize()
    assert int(nm[0]) == on
    assert np.array_equal(mm[0, :nq].cpu().numpy(), om)
    assert np.array_equal(bb[0, :nq].cpu().numpy(), ob) and np.array_equal(ss[0, :nq].cpu().numpy(), os_)
    if nq and nt:
        assert on > nq // 8
    if nq == 0:      # nothing to write: the outputs keep their contents
        assert np.array_equal(mm[0].cpu().numpy(), np.arange(cap))
