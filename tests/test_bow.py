"""Bag of words: DBoW2 transform + BowVector / FeatureVector and
ORBmatcher::SearchByBoW. CPU: known-answer tests of the oracle restatement on hand-built
vocabularies, the ORBvoc.txt text round trip. GPU: bit-exact word / node / weight per descriptor
and identical SearchByBoW matches vs the oracle (the happy paths; tests/test_bow_gpu.py sweeps the
edges, and the last part of this file checks its scenes on the CPU first). Parity unpinned by the reference (DBoW2 and
ORBvoc.txt are absent): the vocabularies are synthetic (orb_slam3_ros2_amd.vocabulary)."""
import numpy as np
import pytest

import bow_numpy as B
from orb_slam3_ros2_amd.vocabulary import Vocabulary, bow_vector, feature_vector


def _tiny_vocab():
    """k=2, L=2: root -> {1, 2}; 1 -> {3, 4}; 2 -> {5, 6}. Node 2's descriptor equals node 1's
    (ties: the first child wins); leaves 3..6 are words 0..3 (leaf order); node 6 has weight 0."""
    desc = np.zeros((7, 32), np.uint8)
    desc[1] = 0x00; desc[2] = 0x00
    desc[3, :4] = 0x0F; desc[4, :4] = 0xF0
    desc[5] = 0xFF; desc[6] = 0xAA
    parent = np.array([-1, 0, 0, 1, 1, 2, 2], np.int32)
    leaf = np.array([0, 0, 0, 1, 1, 1, 1], np.uint8)
    weight = np.array([0, 0, 0, 1.5, 2.0, 3.0, 0.0])
    return Vocabulary(2, 2, 0, 0, parent, leaf, desc, weight)


def test_oracle_transform_known_answers(oracle):
    v = _tiny_vocab()
    f = np.zeros((3, 32), np.uint8)
    f[0, :4] = 0x0F              # -> node 1 (tie with 2, first wins) -> leaf 3 (word 0)
    f[1, :4] = 0xF0              # -> node 1 -> leaf 4 (word 1)
    f[2] = 0xAA                  # node 1 and 2 tie (both 0x00) -> 1 -> 3 vs 4 tie -> 3
    w, nd, wt = oracle.bow_transform(v, f, levelsup=1)   # FeatureVector level L - 1 = 1
    assert w.tolist() == [0, 1, 0] and nd.tolist() == [1, 1, 1]
    assert wt.tolist() == [1.5, 2.0, 1.5]
    w2, nd2, _ = oracle.bow_transform(v, f, levelsup=4)  # level <= 0 -> root
    assert nd2.tolist() == [0, 0, 0]
    words, vals = oracle.bow_vector(w, wt)
    assert words.tolist() == [0, 1] and np.allclose(vals, [3.0 / 5.0, 2.0 / 5.0])
    ww, vv = bow_vector(w, wt)
    assert ww.tolist() == words.tolist() and np.allclose(vv, vals)
    assert feature_vector(nd, wt) == {1: [0, 1, 2]}


def test_zero_weight_words_leave_both_vectors(oracle):
    v = _tiny_vocab()
    v.desc[1] = 0xFF             # node 1 = 0xFF, node 2 = 0x00
    f = np.zeros((2, 32), np.uint8)
    f[0, :] = 0xAA               # d = 128 to both -> node 1 (first) -> a weighted leaf
    f[1] = 0x00                  # node 2 -> leaf 6 (0xAA, d 128 < 256): weight 0, in neither vector
    w, nd, wt = oracle.bow_transform(v, f, levelsup=1)
    keep = wt > 0
    words, _ = oracle.bow_vector(w, wt)
    assert set(words.tolist()) == set(w[keep].tolist())
    assert sum(len(x) for x in feature_vector(nd, wt).values()) == int(keep.sum())


def test_vocabulary_text_round_trip(tmp_path):
    v = Vocabulary.synthetic(k=4, L=3, seed=2)
    p = str(tmp_path / "voc.txt")
    v.save_text(p)
    u = Vocabulary.load_text(p)
    assert (u.k, u.L) == (4, 3) and np.array_equal(u.parent, v.parent) and np.array_equal(u.desc, v.desc)
    assert np.array_equal(u.is_leaf, v.is_leaf) and np.allclose(u.weight, v.weight, rtol=0, atol=0)
    first, nch, children, word = v.csr()
    assert nch[0] == 4 and word.max() == 4 ** 3 - 1


def test_oracle_search_bow_greedy_and_ratio(oracle):
    """Two KF features in one node compete for the same frame feature: the first (index order)
    takes it, the second falls back to the remaining one; ratio rejects an ambiguous pair."""
    kd = np.zeros((3, 32), np.uint8)
    kd[1] = kd[0]; kd[1, 0] ^= 0x01            # near-duplicate of KF 0
    kd[2] = 0x55
    fd = np.zeros((3, 32), np.uint8)
    fd[1] = fd[0]; fd[1, 0] ^= 0x03            # 2 bits from frame 0
    fd[2] = 0x55; fd[2, 0] ^= 0x01
    ka = np.zeros(3, np.float32); fa = np.zeros(3, np.float32)
    n, m = oracle.search_bow(kd, ka, np.array([5, 5, 9]), np.array([1, 1, 1], np.uint8), fd, fa,
                             np.array([5, 5, 9]), ratio=0.9, check_orientation=False)
    # KF0 -> frame 0 (d 0 vs 2: accepted); KF1 -> frame 1 (frame 0 taken; d=1, second 256);
    # KF2 -> frame 2 (only candidate, d = 1)
    assert m.tolist() == [0, 1, 2] and n == 3
    n2, m2 = oracle.search_bow(kd, ka, np.array([5, 5, 9]), np.array([0, 1, 1], np.uint8), fd, fa,
                               np.array([5, 5, 9]), ratio=0.6, check_orientation=False)
    # KF0 has no map point; KF1: d(f0)=1, d(f1)=1 -> best 1, second 1: 1 < 0.6 fails
    assert m2.tolist() == [-1, -1, 2] and n2 == 1


# ------------------------------------------------------------------------------- GPU
def _frames():
    from orb_slam3_ros2_amd import ORBextractor
    from orb_slam3_ros2_amd.synthetic import shifted_frame, synthetic_frame
    ext = ORBextractor(1000)
    a = synthetic_frame(41)
    b = shifted_frame(a, 3, 2, 42)
    _, ka, da = ext(a)
    _, kb, db = ext(b)
    return ka, da, kb, db


@pytest.mark.gpu
@pytest.mark.parametrize("k,L,levelsup", [(10, 6, 4), (10, 4, 2), (6, 5, 3)])
def test_gpu_transform_bit_exact(oracle, k, L, levelsup):
    from orb_slam3_ros2_amd import ORBVocabulary
    v = Vocabulary.synthetic(k, L, seed=7)
    ka, da, kb, db = _frames()
    rng = np.random.default_rng(3)
    feats = np.concatenate([da, db, rng.integers(0, 256, (500, 32), dtype=np.uint8)])
    voc = ORBVocabulary(v)
    w, nd, wt = voc.transform_features(feats, levelsup)
    ow, on, ov = oracle.bow_transform(v, feats, levelsup)
    assert np.array_equal(w, ow) and np.array_equal(nd, on) and np.array_equal(wt, ov)
    (gw, gv), gfv = voc.transform(feats, levelsup)
    rw, rv = oracle.bow_vector(ow, ov)
    assert np.array_equal(gw, rw) and np.array_equal(gv, rv)


@pytest.mark.gpu
def test_gpu_vocab_load_text(tmp_path, oracle):
    from orb_slam3_ros2_amd import ORBVocabulary
    v = Vocabulary.synthetic(8, 4, seed=9)
    p = str(tmp_path / "voc.txt")
    v.save_text(p)
    voc = ORBVocabulary(p)
    assert (voc.k, voc.L, voc.n_nodes, voc.n_words) == (8, 4, v.n_nodes, 8 ** 4)
    rng = np.random.default_rng(5)
    f = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    w, nd, wt = voc.transform_features(f, 2)
    ow, on, ov = oracle.bow_transform(v, f, 2)
    assert np.array_equal(w, ow) and np.array_equal(nd, on) and np.array_equal(wt, ov)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio,ori,levelsup", [(0.7, True, 4), (0.9, False, 4), (0.75, True, 3)])
def test_gpu_search_bow_matches_oracle(oracle, ratio, ori, levelsup):
    from orb_slam3_ros2_amd import ORBmatcher, ORBVocabulary
    v = Vocabulary.synthetic(10, 6, seed=11)
    voc = ORBVocabulary(v)
    ka, da, kb, db = _frames()
    kw_, kn, kwt = voc.transform_features(da, levelsup)
    fw_, fn, fwt = voc.transform_features(db, levelsup)
    valid = (np.random.default_rng(6).random(len(da)) < 0.8).astype(np.uint8)
    mt = ORBmatcher(ratio, ori, ctx=voc.ctx)
    n, m = mt.SearchByBoW(da, ka["angle"], kn, kwt, valid, db, kb["angle"], fn, fwt)
    # the oracle takes FeatureVector membership from node >= 0: gate by weight on both sides
    on2, om2 = oracle.search_bow(da, ka["angle"], np.where(kwt > 0, kn, -1), valid, db, kb["angle"],
                                 np.where(fwt > 0, fn, -1), ratio=ratio, check_orientation=ori)
    assert n == on2 and np.array_equal(m, om2)
    assert n > 50


# ------------------------------------------- the scenes of tests/test_bow_gpu.py, on the CPU
# Before the device is compared with the oracle on a scene, the oracle and an independent plain
# restatement (tests/bow_numpy.py) must agree on it, and the scene must reach what it is there for.
def _oracle_search(oracle, sc, ratio, ori, th_low=50):
    gk, gf = B.gated(sc)
    return oracle.search_bow(sc["kd"], sc["ka"], gk, sc["kv"], sc["fd"], sc["fa"], gf, ratio=ratio,
                             check_orientation=ori, th_low=th_low)


def _numpy_search(sc, ratio, ori, th_low=50):
    gk, gf = B.gated(sc)
    st = {}
    n, m = B.search_bow_numpy(sc["kd"], sc["ka"], gk, sc["kv"], sc["fd"], sc["fa"], gf, ratio, ori, th_low, stats=st)
    return n, m, st


@pytest.mark.parametrize("name", list(B.SCENES))
def test_scene_oracle_equals_restatement_and_is_not_trivial(oracle, name):
    sc = B.scene(name)
    gk, gf = B.gated(sc)
    pos = B.position_in_node(gf)
    for ratio, ori in B.SEARCH_PARAMS:
        n, m = _oracle_search(oracle, sc, ratio, ori)
        rn, rm, st = _numpy_search(sc, ratio, ori)
        assert n == rn and np.array_equal(m, rm)
        assert n == int((m >= 0).sum()) and n > 0.25 * min(len(gk), len(gf))
        # both sides carry zero-weight features, invalid KF features and one-sided nodes
        assert (sc["kw"] == 0).any() and (sc["fw"] == 0).any() and (sc["kv"] == 0).any() and sc["kv"].any()
        assert set(gk[gk >= 0]) - set(gf[gf >= 0]) and set(gf[gf >= 0]) - set(gk[gk >= 0])
        # a KF feature within th_low that only the ratio rule rejects, with best == second
        assert st["ratio_ties"] >= 1
        if name in B.CROWDED:
            # more than two 64-lane chunks in one node, and a match found past the first chunk
            assert np.bincount(gf[gf >= 0]).max() > 128
            assert pos[m >= 0].max() >= 64
    if name in B.ROTATION_BINS:
        # the rotation filter drops matches, and keeps exactly the bins the mixture is built for
        n0, m0 = _oracle_search(oracle, sc, 0.9, False)
        n1, m1 = _oracle_search(oracle, sc, 0.9, True)
        assert n1 < n0 and np.array_equal(m1[m1 >= 0], m0[m1 >= 0])
        bins = [B.rotation_bin(sc["ka"][m0[f]], sc["fa"][f]) for f in np.nonzero(m0 >= 0)[0]]
        keep = [k for k in B.three_maxima(np.bincount(bins, minlength=30)) if k >= 0]
        assert len(keep) == B.ROTATION_BINS[name]
        assert n1 == sum(b in keep for b in bins)


def test_scene_th_low_30(oracle):
    sc = B.scene("flip45")
    n, m = _oracle_search(oracle, sc, 0.9, True, th_low=30)
    rn, rm, st = _numpy_search(sc, 0.9, True, th_low=30)
    assert n == rn and np.array_equal(m, rm)
    assert 0 < n < _oracle_search(oracle, sc, 0.9, True)[0]      # the tighter bound rejects matches


@pytest.mark.parametrize("name", B.DEGENERATE)
def test_degenerate_scenes_give_no_match(oracle, name):
    sc = B.degenerate(name)
    for ratio, ori in B.SEARCH_PARAMS:
        n, m = _oracle_search(oracle, sc, ratio, ori)
        rn, rm, _ = _numpy_search(sc, ratio, ori)
        assert n == rn == 0 and (m == -1).all() and (rm == -1).all()


@pytest.mark.parametrize("seed", [1, 2])
def test_ragged_vocabulary_oracle_equals_numpy_descent(oracle, seed):
    v = B.ragged_vocabulary(5, 5, seed)
    first, nch, children, word = v.csr()
    dep = B.depths(v)
    assert (v.parent[1:] < np.arange(1, v.n_nodes)).all() and dep.max() == v.L
    assert (nch == 1).any() and 1 < nch.max() <= v.k
    assert ((v.is_leaf > 0) & (dep < v.L)).any()                         # leaves above depth L
    assert ((v.is_leaf > 0) & (v.weight == 0)).any() and (v.weight[v.is_leaf == 0] == 0).all()
    twins = [i for i in range(2, v.n_nodes)
             if v.parent[i] == v.parent[i - 1] and np.array_equal(v.desc[i], v.desc[i - 1])]
    assert twins                                                         # identical siblings
    f = B.transform_feats(v, 257, seed)
    for levelsup in (0, v.L - 1, v.L, v.L + 2):
        ow, on, ov = oracle.bow_transform(v, f, levelsup)
        rw, rn, rv = B.bow_transform_numpy(v, f, levelsup)
        assert np.array_equal(ow, rw) and np.array_equal(on, rn) and np.array_equal(ov, rv)
        if levelsup >= v.L:
            assert (on == 0).all()                                       # the root
    ow, on, ov = oracle.bow_transform(v, f, 0)
    early = dep[np.nonzero(v.is_leaf)[0][ow]] < v.L
    assert early.any() and (on[early] == 0).all() and (on[~early] > 0).all()   # level L never reached: node 0
    assert (ov == 0).any()
    path_nodes = oracle.bow_transform(v, f, v.L - 1)[1]                  # the level-1 node of each path
    assert set(np.nonzero(nch == 1)[0]) & set(path_nodes)                # a single-child node is descended
    assert not set(twins) & set(np.nonzero(v.is_leaf)[0][ow])            # the first of two equal siblings wins


@pytest.mark.parametrize("levelsup,n_nodes", [(5, 10), (6, 1)])
def test_vocabulary_scene_oracle_equals_restatement(oracle, levelsup, n_nodes):
    sc = _vocabulary_scene(oracle.bow_transform, levelsup)
    assert len(set(sc["kn"]) | set(sc["fn"])) == n_nodes
    for ratio, ori in B.SEARCH_PARAMS:
        n, m = _oracle_search(oracle, sc, ratio, ori)
        rn, rm, _ = _numpy_search(sc, ratio, ori)
        assert n == rn and np.array_equal(m, rm) and n > 100


_SYNTH = {}


def _synthetic_10_6():
    if not _SYNTH:
        _SYNTH["v"] = Vocabulary.synthetic(10, 6, seed=11)
    return _SYNTH["v"]


def _vocabulary_scene(transform, levelsup):
    """A 600 x 600 scene whose nodes and weights come from `transform(vocabulary, desc, levelsup)`."""
    sc = dict(B.bow_scene(600, 600, [0], seed=600))
    v = _synthetic_10_6()
    _, sc["kn"], sc["kw"] = transform(v, sc["kd"], levelsup)
    _, sc["fn"], sc["fw"] = transform(v, sc["fd"], levelsup)
    return sc
