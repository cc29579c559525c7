"""Test infrastructure for the bag-of-words path: a plain restatement of
U:src/ORBmatcher.cc::SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) and of DBoW2's per-feature
transform, written from the reference's text with Python containers (dict of node -> indices, a
sequential greedy loop), plus the scene and vocabulary builders the tests share. Not used by the
product.

The restatement keeps every float operation the reference performs as one np.float32 operation:
(float)bestDist1 < mfNNratio * (float)bestDist2, rot = kf angle - frame angle (+ 360 when negative),
bin = round(rot * (1.0f / HISTO_LENGTH)) with C round (halves away from zero) and bin 30 -> 0."""
import numpy as np

from helpers import HISTO_LENGTH, c_round, rotation_bin, three_maxima  # noqa: F401 (the tests use them as B.*)
from orb_slam3_ros2_amd.vocabulary import L1_NORM, TF_IDF, Vocabulary

f32 = np.float32
TH_LOW = 50
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def hamming(a, b) -> int:
    return int(_POP[np.bitwise_xor(a, b)].sum())


def search_bow_numpy(kf_desc, kf_angle, kf_node, kf_valid, f_desc, f_angle, f_node, ratio=0.7,
                     check_orientation=True, th_low=TH_LOW, stats=None):
    """(nmatches, match[nf]): match[f] = the KF feature matched to frame feature f, or -1. A node
    < 0 marks a feature outside its FeatureVector. `stats`, a dict, receives what the run did:
    accepted (before the rotation filter), ratio_ties (KF features within th_low that only the ratio
    rule rejected, with best == second), th_low_rejected, kept_bins, max_accept_pos (the largest
    position, inside its node's frame list, of an accepted frame feature)."""
    kd = np.asarray(kf_desc, np.uint8).reshape(-1, 32)
    fd = np.asarray(f_desc, np.uint8).reshape(-1, 32)
    nf = len(f_node)
    fvk, fvf = {}, {}
    for i, nd in enumerate(kf_node):
        if nd >= 0:
            fvk.setdefault(int(nd), []).append(i)
    for i, nd in enumerate(f_node):
        if nd >= 0:
            fvf.setdefault(int(nd), []).append(i)
    match = np.full(nf, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    st = dict(accepted=0, ratio_ties=0, th_low_rejected=0, kept_bins=0, max_accept_pos=-1)
    ratio = f32(ratio)
    for nd in sorted(set(fvk) & set(fvf)):
        cand = np.array(fvf[nd])
        for ik in fvk[nd]:
            if not kf_valid[ik]:
                continue
            # one sequential scan of the node's frame features, skipping matched ones, keeping
            # (best, second) with strict <: the first minimum and the multiset's second smallest
            d = np.where(match[cand] >= 0, 256, _POP[np.bitwise_xor(fd[cand], kd[ik])].sum(axis=1))
            best_pos = int(np.argmin(d))                     # argmin returns the first minimum
            best1 = int(d[best_pos])
            d[best_pos] = 256
            best2 = int(d.min())
            if best1 > th_low:
                st["th_low_rejected"] += 1
                continue
            if f32(best1) < ratio * f32(best2):
                jf = int(cand[best_pos])
                match[jf] = ik
                st["accepted"] += 1
                st["max_accept_pos"] = max(st["max_accept_pos"], best_pos)
                if check_orientation:
                    hist[rotation_bin(kf_angle[ik], f_angle[jf])].append(jf)
            elif best1 == best2:
                st["ratio_ties"] += 1
    n = st["accepted"]
    if check_orientation:
        keep = three_maxima([len(h) for h in hist])
        st["kept_bins"] = sum(k >= 0 for k in keep)
        for i, h in enumerate(hist):
            if i not in keep:
                for jf in h:
                    match[jf] = -1
                    n -= 1
    if stats is not None:
        stats.update(st)
    return n, match


def bow_scene(nk, nf, node_ids, seed, rots=(12.0,), rot_probs=(1.0,), dup_frac=0.2, distractor_frac=0.15,
              absent_frac=0.05, zero_weight_frac=0.05, valid_frac=0.8, max_flip=30, angle_noise=2.5):
    """A KeyFrame / Frame pair as SearchByBoW sees it, without a vocabulary: node ids are given.
    KF descriptors are random, spread over `node_ids`. A frame feature is a KF source with 0..max_flip
    flipped bits in the source's node; a share (dup_frac) repeat another frame feature's source, half
    of them with the very same descriptor (best == second), a share are random distractors, a share
    sit in nodes the KF does not have; a few KF features sit in a node the frame does not have. A
    share of each side has weight 0; kf_valid is ~80 % ones. Frame angle = KF angle - a rotation
    drawn from (rots, rot_probs) + noise, in [0, 360). Returns a dict of arrays."""
    rng = np.random.Generator(np.random.PCG64(seed))
    node_ids = np.asarray(node_ids, np.int32)
    top = int(node_ids.max()) + 1
    kd = rng.integers(0, 256, (nk, 32), dtype=np.uint8)
    ka = rng.uniform(0.0, 360.0, nk).astype(np.float32)
    kn = node_ids[rng.integers(0, len(node_ids), nk)] if nk else np.zeros(0, np.int32)
    kn = kn.astype(np.int32)
    kw = rng.uniform(0.5, 8.0, nk)
    kw[rng.random(nk) < zero_weight_frac] = 0.0
    kv = (rng.random(nk) < valid_frac).astype(np.uint8)
    fd = rng.integers(0, 256, (nf, 32), dtype=np.uint8)      # distractors keep these
    fa = rng.uniform(0.0, 360.0, nf).astype(np.float32)
    fn = node_ids[rng.integers(0, len(node_ids), nf)].astype(np.int32) if nf else np.zeros(0, np.int32)
    fw = rng.uniform(0.5, 8.0, nf)
    fw[rng.random(nf) < zero_weight_frac] = 0.0
    if nk and nf:
        src = rng.integers(0, nk, nf)
        src[:min(nk, nf)] = rng.permutation(nk)[:min(nk, nf)]
        kind = rng.random(nf)
        rot = rng.choice(np.asarray(rots, np.float64), size=nf, p=np.asarray(rot_probs, np.float64))
        noise = rng.uniform(-angle_noise, angle_noise, nf)
        nflip = rng.integers(0, max_flip + 1, nf)
        for i in range(nf):
            if kind[i] < distractor_frac:
                continue
            twin = -1
            if kind[i] < distractor_frac + dup_frac and i > 0:
                twin = int(rng.integers(0, i))
                src[i] = src[twin]
            s = int(src[i])
            d = kd[s].copy()
            bits = rng.choice(256, size=int(nflip[i]), replace=False)
            np.bitwise_xor.at(d, bits >> 3, (1 << (bits & 7)).astype(np.uint8))
            fd[i] = d
            fn[i] = kn[s]
            if twin >= 0 and kind[i] < distractor_frac + dup_frac / 2:
                fd[i], fn[i] = fd[twin], fn[twin]            # identical twin: a best == second tie
            fa[i] = np.float32((float(ka[s]) - rot[i] + noise[i]) % 360.0)
        fa[fa >= np.float32(360.0)] = 0.0
        fn[rng.random(nf) < absent_frac] = top + 3           # a node the KF never has
    kn[rng.random(nk) < 0.02] = top + 7                      # a node the frame never has
    return dict(kd=kd, ka=ka, kn=kn, kw=kw, kv=kv, fd=fd, fa=fa, fn=fn, fw=fw)


def gated(sc):
    """The scene's node arrays as the oracle and the restatement take them: -1 where the weight is 0."""
    return (np.where(sc["kw"] > 0, sc["kn"], -1).astype(np.int32),
            np.where(sc["fw"] > 0, sc["fn"], -1).astype(np.int32))


def ragged_vocabulary(k, L, seed) -> Vocabulary:
    """A vocabulary no full k-ary tree gives: child counts drawn from 1..k (the first level-1 node
    has exactly one child), leaves above depth L, sibling pairs with identical descriptors, leaves
    of weight 0. Nodes are numbered breadth first, so parent[i] < i."""
    rng = np.random.Generator(np.random.PCG64(seed))
    parent, depth, desc, leaf = [-1], [0], [np.zeros(32, np.uint8)], [0]
    frontier = [0]
    forced_single = False
    while frontier:
        nxt = []
        for p in frontier:
            nc = int(rng.integers(1, k + 1))
            if p == 0:
                nc = max(nc, 3)
            elif not forced_single:
                nc, forced_single = 1, True
            for c in range(nc):
                if depth[p] == 0:
                    d = rng.integers(0, 256, 32, dtype=np.uint8)
                else:
                    m = rng.integers(0, 256, 32, dtype=np.uint8) & rng.integers(0, 256, 32, dtype=np.uint8)
                    d = desc[p] ^ (m & rng.integers(0, 256, 32, dtype=np.uint8))
                if c > 0 and rng.random() < 0.2:
                    d = desc[-1].copy()                      # identical to the previous sibling
                i = len(parent)
                parent.append(p); depth.append(depth[p] + 1); desc.append(d)
                # the single child stays internal while it can, so the one-child descent is taken
                early = depth[i] < L and nc > 1 and rng.random() < 0.2
                is_leaf = depth[i] == L or early
                leaf.append(int(is_leaf))
                if not is_leaf:
                    nxt.append(i)
        frontier = nxt
    N = len(parent)
    leaf = np.array(leaf, np.uint8)
    weight = np.zeros(N, np.float64)
    nl = int(leaf.sum())
    w = rng.uniform(0.5, 8.0, nl)
    w[rng.random(nl) < 0.1] = 0.0
    weight[leaf > 0] = w
    return Vocabulary(k, L, L1_NORM, TF_IDF, np.array(parent, np.int32), leaf, np.stack(desc).astype(np.uint8),
                      weight)


def bow_transform_numpy(vocab: Vocabulary, feats, levelsup):
    """DBoW2 transform(feature, word, weight, nid, levelsup) per feature: the first child at the
    smallest distance, the node at level L - levelsup (0 if that level is never reached)."""
    kids = {}
    for i in range(1, vocab.n_nodes):
        kids.setdefault(int(vocab.parent[i]), []).append(i)
    word_of = {int(n): w for w, n in enumerate(np.nonzero(vocab.is_leaf)[0])}
    out = []
    for f in np.asarray(feats, np.uint8).reshape(-1, 32):
        cur, level, nid = 0, 0, 0
        while cur in kids:
            level += 1
            cur = min(kids[cur], key=lambda c: hamming(f, vocab.desc[c]))   # min keeps the first
            if level == vocab.L - levelsup:
                nid = cur
        out.append((word_of[cur], nid, float(vocab.weight[cur])))
    w, nd, wt = zip(*out) if out else ((), (), ())
    return np.array(w, np.int32), np.array(nd, np.int32), np.array(wt, np.float64)


# ------------------------------------------------------------------ the scenes the tests share
ROTS = (12.0, 100.0, 200.0, 300.0)
# name -> bow_scene arguments. Crowded scenes hold more than 128 frame features in one node (a wave
# scans 64 per chunk); the rotation scenes keep one, two and three histogram bins.
SCENES = {
    "one64": dict(nk=64, nf=64, node_ids=[5], seed=64),
    "one65": dict(nk=65, nf=65, node_ids=[5], seed=65),
    "one128": dict(nk=128, nf=128, node_ids=[5], seed=128),
    "one129": dict(nk=129, nf=129, node_ids=[5], seed=129),
    "one1000": dict(nk=1000, nf=1000, node_ids=[5], seed=1000),
    "cap_one": dict(nk=2048, nf=2048, node_ids=[5], seed=2048),
    "cap_40": dict(nk=2048, nf=2048, node_ids=list(range(100, 140)), seed=2049),
    "three1025": dict(nk=1025, nf=1025, node_ids=[3, 9, 11], seed=1025),
    "three1500": dict(nk=1500, nf=1300, node_ids=[3, 9, 11], seed=1500),
    "two129": dict(nk=129, nf=200, node_ids=[4, 8], seed=329),
    # up to 45 flipped bits: th_low = 30 rejects what the default 50 accepts
    "flip45": dict(nk=600, nf=600, node_ids=[3, 9, 11], seed=645, max_flip=45),
    "rot1": dict(nk=400, nf=400, node_ids=[3, 9, 11], seed=401, rots=ROTS, rot_probs=(0.94, 0.02, 0.02, 0.02)),
    "rot2": dict(nk=400, nf=400, node_ids=[3, 9, 11], seed=402, rots=ROTS, rot_probs=(0.6, 0.36, 0.02, 0.02)),
    "rot3": dict(nk=400, nf=400, node_ids=[3, 9, 11], seed=403, rots=ROTS, rot_probs=(0.4, 0.3, 0.25, 0.05)),
}
CROWDED = ("one1000", "cap_one", "three1025", "three1500")
ROTATION_BINS = {"rot1": 1, "rot2": 2, "rot3": 3}
SEARCH_PARAMS = [(0.7, True), (0.9, False), (1.0, True)]
_BUILT = {}


def scene(name):
    """A named scene, built once per process and never modified."""
    if name not in _BUILT:
        _BUILT[name] = bow_scene(**SCENES[name])
    return _BUILT[name]


def degenerate(name):
    """Scenes that must give 0 matches, derived from "two129": no valid KF feature; disjoint node
    sets; every frame weight 0; every KF weight 0."""
    sc = dict(scene("two129"))
    if name == "no_valid":
        sc["kv"] = np.zeros_like(sc["kv"])
    elif name == "disjoint":
        sc["fn"] = sc["fn"] + 1000
    elif name == "frame_weight0":
        sc["fw"] = np.zeros_like(sc["fw"])
    elif name == "kf_weight0":
        sc["kw"] = np.zeros_like(sc["kw"])
    else:
        raise KeyError(name)
    return sc


DEGENERATE = ("no_valid", "disjoint", "frame_weight0", "kf_weight0")


def position_in_node(f_node):
    """Per frame feature: its position among the features of its node, in index order (-1 outside)."""
    pos = np.full(len(f_node), -1, np.int64)
    seen = {}
    for i, nd in enumerate(f_node):
        if nd >= 0:
            pos[i] = seen.get(int(nd), 0)
            seen[int(nd)] = pos[i] + 1
    return pos


def transform_feats(vocab, n, seed):
    """n descriptors for a transform test: two thirds are node descriptors of the vocabulary with a
    few flipped bits (they descend towards every kind of node), the rest random."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    near = np.nonzero(rng.random(n) < 0.67)[0]
    f[near] = vocab.desc[rng.integers(1, vocab.n_nodes, len(near))]
    bits = rng.integers(0, 256, (len(near), 3))
    for r, i in enumerate(near):
        for b in bits[r]:
            f[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return f


def depths(vocab):
    d = np.zeros(vocab.n_nodes, np.int64)
    for i in range(1, vocab.n_nodes):
        d[i] = d[vocab.parent[i]] + 1
    return d
