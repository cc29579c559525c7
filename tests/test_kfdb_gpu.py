"""KeyFrameDatabase queries on the device (csrc/kfdb_kernels.hip) against the oracle, past 1024
slots and at every edge: U:src/KeyFrameDatabase.cc DetectRelocalizationCandidates and
DetectNBestCandidates with DBoW2 L1 scoring.

After every query the candidate lists AND the persistent KeyFrame members (mnRelocQuery /
mnRelocWords / mRelocScore and the mnPlaceRecognition* ones) are compared with the oracle's:
  query  equal on every slot;
  score  bit-equal on every slot (the same terms in the same order, summed in fp64, no multiply
         to contract, halved, cast to float);
  words  equal on the slots the query just claimed (query == its id). The oracle also resets the
         word count of connected KeyFrames without claiming them, which no later query can see.

  large   2603 slots (k_kfdb_select's 1024-wide loops take several trips, the ranks exceed 1024),
          KeyFrames added in a scrambled order, bursts of queries between adds and erases,
          "corridor" queries that score > 2048 KeyFrames and return lists of hundreds.
  edges   BowVector lengths around the lane tail (64) and the summation chunk (512), KeyFrames
          longer than the query, query lengths 0, 1, kQMax = 3072 and 3073.
  ties    identical BowVectors: first-encounter order is insertion order, not slot order; a
          re-added slot moves to the end; exact accScore ties keep entry order (stable sort).
  errors  every ORBHIP_ERR_ARG of the entry points leaves the members and later results alone.
"""
import numpy as np
import pytest

from orb_slam3_ros2_amd.synthetic import synthetic_kfdb_scene, synthetic_query_bow

pytestmark = pytest.mark.gpu

ERR_ARG = -1
KQMAX = 3072


def _l1(a, b):
    """DBoW2 L1Scoring::score restated: common words ascending, fp64, summed in order."""
    wa, va = a
    wb, vb = b
    _, ia, ib = np.intersect1d(wa, wb, return_indices=True)
    s = 0.0
    for x, y in zip(va[ia].tolist(), vb[ib].tolist()):
        s += abs(x - y) - abs(x) - abs(y)
    return -s / 2.0


def _norm_bow(rng, words):
    w = np.unique(np.asarray(words)).astype(np.int32)
    v = rng.gamma(2.0, 1.0, w.shape[0])
    return w, v / max(v.sum(), 1e-300)


def _check_members(dev, ref, mode, qid, tag):
    dq, dw, ds = dev._members(mode)
    rq, rw, rs = ref._members(mode)
    assert np.array_equal(dq, rq), (tag, "query", np.flatnonzero(dq != rq)[:8])
    bad = np.flatnonzero(ds.view(np.uint32) != rs.view(np.uint32))
    assert bad.size == 0, (tag, "score", bad[:8], ds[bad[:8]], rs[bad[:8]])
    m = rq == qid
    assert np.array_equal(dw[m], rw[m]), (tag, "words", np.flatnonzero(m & (dw != rw))[:8])
    return dq, dw, ds


class _Pair:
    """The device database and the oracle's, fed the same calls; every query is compared."""

    def __init__(self, oracle, max_kf, n_words):
        from orb_slam3_ros2_amd import KeyFrameDatabase
        self.dev = KeyFrameDatabase(max_kf)
        self.ref = oracle.KeyFrameDatabase(max_kf, n_words)
        self.qid = 100

    def add(self, kf, bow):
        self.dev.add(kf, bow); self.ref.add(kf, bow)

    def erase(self, kf):
        self.dev.erase(kf); self.ref.erase(kf)

    def reloc(self, bow, covis, kf_map=None, query_map=0, tag=None):
        self.qid += 1
        a = self.dev.DetectRelocalizationCandidates(self.qid, bow, covis, kf_map, query_map)
        b = self.ref.DetectRelocalizationCandidates(self.qid, bow, covis, kf_map, query_map)
        assert np.array_equal(a, b), (tag, "reloc", a[:16], b[:16], len(a), len(b))
        _check_members(self.dev, self.ref, 0, self.qid, tag)
        return b

    def nbest(self, bow, covis, connected=None, n=3, kf_map=None, query_map=0, flags=None, tag=None):
        self.qid += 1
        a = self.dev.DetectNBestCandidates(self.qid, bow, covis, connected, n, kf_map, query_map, flags)
        b = self.ref.DetectNBestCandidates(self.qid, bow, covis, connected, n, kf_map, query_map, flags)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (tag, "nbest", a, b)
        _check_members(self.dev, self.ref, 1, self.qid, tag)
        return b

    def members(self):
        return [x.copy() for mode in (0, 1) for x in self.dev._members(mode)]


def _same(ma, mb):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(ma, mb))


# ---------------------------------------------------------------------------
# a. large database
# ---------------------------------------------------------------------------
N_LARGE, MAX_LARGE = 2600, 2603   # 2603: not a multiple of 4, the last three slots are never added


@pytest.fixture(scope="module")
def large_scene():
    sc = synthetic_kfdb_scene(n_kf=N_LARGE, words_per_place=20, seed=5, common_pool=600, common_frac=0.6)
    covis = np.full((MAX_LARGE, 10), -1, np.int32); covis[:N_LARGE] = sc["covis"]
    kf_map = np.zeros(MAX_LARGE, np.int32); kf_map[:N_LARGE] = sc["kf_map"]
    # the repetitive-texture pool: the words more than 20 % of the KeyFrames see
    seen = np.bincount(np.concatenate([w for w, _ in sc["bows"]]), minlength=20000)
    pool = np.flatnonzero(seen > 0.2 * N_LARGE)
    return dict(sc, covis=covis, kf_map=kf_map, pool=pool)


def _corridor_bow(rng, pool):
    """A frame in a corridor of repetitive texture: about half of the pool words, plus 40 random words."""
    return _norm_bow(rng, np.concatenate([pool[rng.random(pool.shape[0]) < 0.5], rng.choice(20000, 40, replace=False)]))


def _above_cut(bows, slots, qw):
    """KeyFrames above the common-word cut (0.8f * max common words) of a query, from numpy alone."""
    common = np.array([np.isin(bows[s][0], qw, assume_unique=True).sum() for s in slots])
    cut = int(np.float32(common.max()) * np.float32(0.8))
    return int((common > cut).sum())


def test_large_database_matches_oracle(oracle, large_scene):
    sc = large_scene
    p = _Pair(oracle, MAX_LARGE, 20000)
    order = np.random.default_rng(1).permutation(N_LARGE)
    rng = np.random.default_rng(3)
    crng = np.random.default_rng(2)   # the corridor queries
    assert 550 <= sc["pool"].shape[0] <= 600
    # (kind: near k KeyFrames | 0 = corridor, kf_map?, N-best n, connected?)
    bursts = {900: [(1, True, 3, True), (3, False, 0, False), (0, True, 32, True), (0, False, 3, False)],
              1700: [(2, False, 32, False), (1, True, 3, True), (0, False, 0, True), (0, True, 32, False)],
              2600: [(3, True, 32, True), (0, True, 32, False), (0, False, 3, True), (0, True, 0, False),
                     (2, False, 3, False)]}
    added = []
    seen = dict(scored=[], reloc=[], loop=[], merge=[])
    for i, s in enumerate(order.tolist()):
        p.add(s, sc["bows"][s]); added.append(s)
        if i + 1 not in bursts:
            continue
        for t, (near, use_map, n, use_con) in enumerate(bursts[i + 1]):
            tag = (i + 1, t)
            k = int(rng.choice(added))
            if near:
                ks = [k] + [int(x) for x in rng.choice(added, near - 1, replace=False)]
                bow = synthetic_query_bow(sc, ks, seed=1000 + 10 * i + t, keep=0.5)
            else:
                bow = _corridor_bow(crng, sc["pool"])
            km, qm = (sc["kf_map"] if use_map else None), int(sc["kf_map"][k])
            rl = p.reloc(bow, sc["covis"], km, qm, tag)
            con = None
            if use_con:
                con = np.zeros(MAX_LARGE, np.uint8)
                con[sc["covis"][k][sc["covis"][k] >= 0]] = 1
                con[rng.choice(added, 30, replace=False)] = 1
            flags = ((rng.random(MAX_LARGE) < 0.05) | ((rng.random(MAX_LARGE) < 0.05) << 1)).astype(np.uint8)
            lo, me = p.nbest(bow, sc["covis"], con, n, km, qm, flags, tag)
            assert len(lo) <= n and len(me) <= n
            if not near and i + 1 == N_LARGE:   # the corridor queries on the full database
                seen["scored"].append(_above_cut(sc["bows"], added, bow[0]))
                seen["reloc"].append(len(rl)); seen["loop"].append(len(lo)); seen["merge"].append(len(me))
        if i + 1 < N_LARGE:   # KeyFrame culling; the last burst sees the erased slots
            for k in rng.choice(added, 3, replace=False).tolist():
                p.erase(k); added.remove(k)
    print("large: corridor query on the full database:", seen)
    # what this test is for, from numpy and the oracle alone: every 1024-wide loop of the select
    # kernel takes a third trip, the ranks of both sorts pass 2048, the lists are long
    assert any(s > 2048 and r > 100 and lp == 32 and mg == 32
               for s, r, lp, mg in zip(seen["scored"], seen["reloc"], seen["loop"], seen["merge"])), seen


# ---------------------------------------------------------------------------
# b. BowVector length edges
# ---------------------------------------------------------------------------
EDGE_LENS = [0, 1, 63, 64, 65, 511, 512, 513, 1024, 1025, 1537, 3072, 3500]
EDGE_WORDS = 40000


@pytest.fixture(scope="module")
def edge_db(oracle):
    """Isolated KeyFrames (no covisibility) of disjoint word sets, one per length; `pad` holds
    the words no KeyFrame owns. 13 slots: the last work-group of k_kfdb_share has one wave of work."""
    rng = np.random.default_rng(7)
    words = rng.permutation(EDGE_WORDS)
    bows, o = [], 0
    for ln in EDGE_LENS:
        bows.append(_norm_bow(rng, words[o:o + ln])); o += ln
    pad = np.sort(words[o:])
    p = _Pair(oracle, len(EDGE_LENS), EDGE_WORDS)
    for s in rng.permutation(len(EDGE_LENS)).tolist():
        p.add(s, bows[s])
    return p, bows, pad, np.full((len(EDGE_LENS), 10), -1, np.int32)


def _edge_queries(rng, bow, pad):
    """Queries holding the KeyFrame's words (its first 3072) plus padding words, of the KeyFrame's
    length (>= 1), + 64 and kQMax; and one of every second word (a KeyFrame longer than the query)."""
    own = bow[0][:KQMAX]
    sizes = sorted({max(own.shape[0], 1), min(own.shape[0] + 64, KQMAX), KQMAX})
    qs = [_norm_bow(rng, np.concatenate([own, rng.choice(pad, nq - own.shape[0], replace=False)])) for nq in sizes]
    if own.shape[0] >= 2:
        qs.append(_norm_bow(rng, own[::2]))
    return qs


@pytest.mark.parametrize("slot", range(len(EDGE_LENS)), ids=[f"len{n}" for n in EDGE_LENS])
def test_bowvector_length_edges(edge_db, slot):
    p, bows, pad, covis = edge_db
    rng = np.random.default_rng(100 + slot)
    ln = EDGE_LENS[slot]
    for q in _edge_queries(rng, bows[slot], pad):
        tag = (ln, q[0].shape[0])
        assert q[0].shape[0] <= KQMAX
        before = p.members()
        rl = p.reloc(q, covis, tag=tag)
        lo, me = p.nbest(q, covis, None, 3, tag=tag)
        after = p.members()
        expect = [slot] if ln else []
        assert rl.tolist() == expect and lo.tolist() == expect and me.tolist() == [], (tag, rl, lo, me)
        # only that slot's members change
        for x, y in zip(before, after):
            bits = np.uint32 if x.itemsize == 4 else np.uint64
            assert np.flatnonzero(x.view(bits) != y.view(bits)).tolist() in ([], expect), tag
        if ln:
            want = _l1(q, bows[slot])
            n_common = np.isin(bows[slot][0], q[0]).sum()
            for qy, wd, sc in (after[0:3], after[3:6]):
                assert wd[slot] == n_common and qy[slot] in (p.qid - 1, p.qid)
                # bit-equal to the oracle (checked in reloc / nbest), and the oracle to the definition
                assert abs(float(sc[slot]) - float(np.float32(want))) <= 1e-12 * abs(want), (tag, sc[slot], want)


def test_query_size_edges(edge_db):
    from orb_slam3_ros2_amd._lib import OrbHipError
    p, bows, pad, covis = edge_db
    rng = np.random.default_rng(11)
    before = p.members()
    empty = (np.zeros(0, np.int32), np.zeros(0, np.float64))
    assert p.reloc(empty, covis, tag="nq0").size == 0
    lo, me = p.nbest(empty, covis, None, 3, tag="nq0")
    assert lo.size == 0 and me.size == 0
    assert _same(before, p.members())
    # kQMax + 1 words, half of them the 3072-word KeyFrame's
    big = _norm_bow(rng, np.concatenate([bows[EDGE_LENS.index(3072)][0][:1500], pad[:KQMAX + 1 - 1500]]))
    assert big[0].shape[0] == KQMAX + 1
    for call in (lambda: p.dev.DetectRelocalizationCandidates(7, big, covis),
                 lambda: p.dev.DetectNBestCandidates(8, big, covis, None, 3)):
        with pytest.raises(OrbHipError) as e:
            call()
        assert e.value.code == ERR_ARG
    assert _same(before, p.members())


# ---------------------------------------------------------------------------
# c. ties and insertion order
# ---------------------------------------------------------------------------
N_TIE = 40


def test_ties_follow_insertion_order(oracle):
    """40 identical BowVectors: every score and accScore ties, so the lists are the first-encounter
    order = insertion order (never slot order), and the N-best sort must be stable."""
    rng = np.random.default_rng(21)
    bow = _norm_bow(rng, rng.choice(20000, 300, replace=False))
    order = rng.permutation(N_TIE).tolist()
    assert order != sorted(order)
    covis = np.full((N_TIE, 10), -1, np.int32)
    kf_map = (np.arange(N_TIE) % 2).astype(np.int32)
    p = _Pair(oracle, N_TIE, 20000)
    for s in order:
        p.add(s, bow)
    assert p.reloc(bow, covis, tag="ties").tolist() == order
    lo, me = p.nbest(bow, covis, None, 32, kf_map, 0, tag="ties")
    assert lo.tolist() == [s for s in order if s % 2 == 0] and len(lo) == 20
    assert me.tolist() == [s for s in order if s % 2 == 1] and len(me) == 20
    # a re-added KeyFrame is the newest entry of every inverted list
    first = order[0]
    p.erase(first)
    assert p.reloc(bow, covis, tag="erased").tolist() == order[1:]
    p.add(first, bow)
    order = order[1:] + [first]
    assert p.reloc(bow, covis, tag="readded").tolist() == order
    lo, me = p.nbest(bow, covis, None, 32, kf_map, 0, tag="readded")
    assert lo.tolist() == [s for s in order if s % 2 == 0]
    assert me.tolist() == [s for s in order if s % 2 == 1]
    _, _, sc = p.dev._members(0)
    assert (sc.view(np.uint32) == np.float32(1.0).view(np.uint32)).all()


def test_ties_with_covisibility(oracle):
    """accScores that tie across groups and differ between them. Slots s % 4 == 0 hold the query's
    BowVector (score 1), the others the same words with other values (score w < 1, all equal).
      s % 4 == 0  covisible s + 1        acc 1 + w   pBestKF s
      s % 4 == 1  covisible s - 1        acc w + 1   pBestKF s - 1 (the better score)
      s % 4 == 2  covisible s - 1, s + 1 acc 3 w     pBestKF s (equal scores never replace it)
      s % 4 == 3  none                   acc w       pBestKF s
    N-best walks the 3w entries, then the 1 + w ones, then the w ones, each group in insertion
    order, a pBestKF only once; relocalisation keeps accScore > 0.75 * 3w in entry order."""
    rng = np.random.default_rng(22)
    words = rng.choice(20000, 300, replace=False)
    strong = _norm_bow(rng, words)
    weak = _norm_bow(rng, words)
    w = np.float32(_l1(strong, weak))
    one = np.float32(_l1(strong, strong))
    acc = {0: one + w, 1: w + one, 2: (w + w) + w, 3: w}
    assert acc[0] == acc[1] and acc[2] > acc[0] > acc[3] and acc[0] > np.float32(0.75) * acc[2] > acc[3]
    order = rng.permutation(N_TIE).tolist()
    covis = np.full((N_TIE, 10), -1, np.int32)
    for s in range(N_TIE):
        covis[s, :2] = {0: [s + 1, -1], 1: [s - 1, -1], 2: [s - 1, s + 1], 3: [-1, -1]}[s % 4]
    kf_map = (np.arange(N_TIE) // 2 % 2).astype(np.int32)
    p = _Pair(oracle, N_TIE, 20000)
    for s in order:
        p.add(s, strong if s % 4 == 0 else weak)
    best = {s: s - 1 if s % 4 == 1 else s for s in order}

    def first_occurrences(entries):
        out = []
        for s in entries:
            if best[s] not in out:
                out.append(best[s])
        return out

    rl = p.reloc(strong, covis, tag="covis ties")
    assert rl.tolist() == first_occurrences([s for s in order if s % 4 != 3])
    lo, me = p.nbest(strong, covis, None, 32, kf_map, 0, tag="covis ties")
    walk = first_occurrences([s for s in order if s % 4 == 2] + [s for s in order if s % 4 in (0, 1)] +
                             [s for s in order if s % 4 == 3])
    assert len(walk) == 30
    assert lo.tolist() == [s for s in walk if kf_map[s] == 0]
    assert me.tolist() == [s for s in walk if kf_map[s] == 1]
    # with fewer places than candidates the walk stops early, still in that order
    lo, me = p.nbest(strong, covis, None, 3, kf_map, 0, tag="covis ties n3")
    assert lo.tolist() == [s for s in walk if kf_map[s] == 0][:3]
    assert me.tolist() == [s for s in walk if kf_map[s] == 1][:3]


# ---------------------------------------------------------------------------
# d. argument errors
# ---------------------------------------------------------------------------
N_ERR = 30


@pytest.fixture(scope="module")
def err_db(oracle):
    sc = synthetic_kfdb_scene(n_kf=N_ERR, seed=4)
    p = _Pair(oracle, N_ERR, 20000)
    for s in range(N_ERR - 4):   # the last four slots stay free
        p.add(s, sc["bows"][s])
    q = synthetic_query_bow(sc, [7, 8], seed=1)
    p.reloc(q, sc["covis"], sc["kf_map"], 0, tag="warm")
    p.nbest(q, sc["covis"], None, 3, sc["kf_map"], 0, tag="warm")
    return p, sc, q


def _bad_covis(sc, row, col, value):
    cv = sc["covis"].copy()
    cv[row, col] = value
    return cv


ERR_CALLS = {
    "add_active": lambda d, sc, q: d.add(3, sc["bows"][3]),
    "add_descending": lambda d, sc, q: d.add(N_ERR - 1, (sc["bows"][5][0][::-1].copy(), sc["bows"][5][1])),
    "add_repeated": lambda d, sc, q: d.add(N_ERR - 1, (np.array([4, 9, 9, 12], np.int32), np.full(4, 0.25))),
    "add_slot_high": lambda d, sc, q: d.add(N_ERR, sc["bows"][5]),
    "add_slot_negative": lambda d, sc, q: d.add(-1, sc["bows"][5]),
    "erase_high": lambda d, sc, q: d.erase(N_ERR),
    "erase_negative": lambda d, sc, q: d.erase(-1),
    "reloc_unsorted": lambda d, sc, q: d.DetectRelocalizationCandidates(9001, (q[0][::-1].copy(), q[1]), sc["covis"]),
    "nbest_unsorted": lambda d, sc, q: d.DetectNBestCandidates(9002, (q[0][::-1].copy(), q[1]), sc["covis"]),
    "reloc_repeated_word": lambda d, sc, q: d.DetectRelocalizationCandidates(
        9003, (np.concatenate([q[0][:1], q[0]]), np.concatenate([q[1][:1], q[1]])), sc["covis"]),
    "nbest_n33": lambda d, sc, q: d.DetectNBestCandidates(9004, q, sc["covis"], None, 33),
    "nbest_n_negative": lambda d, sc, q: d.DetectNBestCandidates(9005, q, sc["covis"], None, -1),
    "reloc_covis_n_slots": lambda d, sc, q: d.DetectRelocalizationCandidates(9006, q, _bad_covis(sc, 7, 0, N_ERR)),
    "nbest_covis_n_slots": lambda d, sc, q: d.DetectNBestCandidates(9007, q, _bad_covis(sc, 8, 9, N_ERR)),
    "reloc_covis_huge": lambda d, sc, q: d.DetectRelocalizationCandidates(9008, q, _bad_covis(sc, 0, 3, 2**31 - 1)),
    "nbest_covis_last_row": lambda d, sc, q: d.DetectNBestCandidates(9009, q, _bad_covis(sc, N_ERR - 1, 9, N_ERR + 5)),
}


@pytest.mark.parametrize("name", sorted(ERR_CALLS))
def test_argument_errors_leave_the_database_alone(err_db, name):
    """The invalid covis rows only ever reach a library that validates them on the host, before
    its first copy or launch (run_query)."""
    from orb_slam3_ros2_amd._lib import OrbHipError
    p, sc, q = err_db
    before = p.members()
    with pytest.raises(OrbHipError) as e:
        ERR_CALLS[name](p.dev, sc, q)
    assert e.value.code == ERR_ARG
    assert _same(before, p.members())
    # and the database still answers as the oracle's, which never saw the call
    p.reloc(q, sc["covis"], sc["kf_map"], 1, tag=name)
    p.nbest(q, sc["covis"], None, 3, sc["kf_map"], 1, tag=name)
    if name.startswith("add"):
        p.add(N_ERR - 1, sc["bows"][N_ERR - 1])   # the slot a failed add named is still free
        p.reloc(sc["bows"][N_ERR - 1], sc["covis"], tag=name)
        p.erase(N_ERR - 1)


def test_negative_covis_ends_the_row(err_db):
    """Negative entries keep their meaning: the first one ends the row, whatever follows it (< n_slots)."""
    p, sc, q = err_db
    cv = sc["covis"].copy()
    cv[7, 2] = -5
    cv[8, 0] = -2**31
    p.reloc(q, cv, tag="negative covis")
    p.nbest(q, cv, None, 3, tag="negative covis")


def test_create_rejects_empty_database():
    from orb_slam3_ros2_amd import KeyFrameDatabase
    from orb_slam3_ros2_amd._lib import OrbHipError
    for n in (0, -1):
        with pytest.raises(OrbHipError) as e:
            KeyFrameDatabase(n)
        assert e.value.code == ERR_ARG
