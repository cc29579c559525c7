"""The bag-of-words kernels at every route and size edge against the oracle (tests/test_bow.py holds
the happy paths and, on the CPU, the proof that the oracle and a plain restatement agree on every
scene used here and that each scene reaches what it is there for):
  k_search_bow     nodes of more than 64 frame features (the chunk merge), more than 1024 features
                   a side (the compaction passes), the 2048 cap and the refusal past it, rotation
                   mixtures that keep one, two and three histogram bins, th_low, empty and
                   one-sided inputs;
  k_bow_transform  ragged vocabularies (single children, early leaves, equal siblings), levelsup
                   from 0 to past L, n around the 256-thread block, and the batched device entry
                   point with per-frame counts.
Indices, node ids, weights and counts are compared bit for bit."""
import ctypes

import numpy as np
import pytest

import bow_numpy as B
from orb_slam3_ros2_amd.vocabulary import Vocabulary

pytestmark = pytest.mark.gpu

_CTX = {}


def _matcher(ratio, ori):
    from orb_slam3_ros2_amd import ORBmatcher
    from orb_slam3_ros2_amd._lib import Context
    if "ctx" not in _CTX:
        _CTX["ctx"] = Context()
    return ORBmatcher(ratio, ori, ctx=_CTX["ctx"])


def _device(sc, ratio, ori, th_low=None):
    return _matcher(ratio, ori).SearchByBoW(sc["kd"], sc["ka"], sc["kn"], sc["kw"], sc["kv"], sc["fd"], sc["fa"],
                                            sc["fn"], sc["fw"], th_low=th_low)


_REF = {}


def _oracle(oracle, name, sc, ratio, ori, th_low=50):
    """The oracle's (n, match) for a named scene: computed once, never modified."""
    key = (name, ratio, ori, th_low)
    if key not in _REF:
        gk, gf = B.gated(sc)
        n, m = oracle.search_bow(sc["kd"], sc["ka"], gk, sc["kv"], sc["fd"], sc["fa"], gf, ratio=ratio,
                                 check_orientation=ori, th_low=th_low)
        m.setflags(write=False)
        _REF[key] = (n, m)
    return _REF[key]


# ---------------------------------------------------------------------------- SearchByBoW
@pytest.mark.parametrize("ratio,ori", B.SEARCH_PARAMS)
@pytest.mark.parametrize("name", list(B.SCENES))
def test_search_bow_scene_matches_oracle(oracle, name, ratio, ori):
    sc = B.scene(name)
    n, m = _device(sc, ratio, ori)
    on, om = _oracle(oracle, name, sc, ratio, ori)
    assert n == on and np.array_equal(m, om)
    if ori and name.startswith("rot"):   # k_search_bow's rotation filter removes matches in these scenes
        assert on < _oracle(oracle, name, sc, ratio, False)[0]
    assert n > 0


@pytest.mark.parametrize("hist", ["12-1", "ties"])
def test_rotation_filter_rules(oracle, hist):
    """ComputeThreeMaxima's two rules in k_search_bow: one node, every KF feature with its twin in
    the frame (the same descriptor, every other one random), so each matches it and the angles alone
    decide. A single match beside twelve is dropped (1 < 0.1f * 12); of four equal bins the three
    of lower index stay."""
    from helpers import rot_edge_bins
    bins, kept = rot_edge_bins(hist)
    n = len(bins)
    d = np.random.default_rng(100 + n).integers(0, 256, (n, 32), dtype=np.uint8)
    node, w = np.zeros(n, np.int32), np.ones(n)
    sc = dict(kd=d, ka=(30.0 * bins).astype(np.float32), kn=node, kw=w, kv=np.ones(n, np.uint8), fd=d,
              fa=np.zeros(n, np.float32), fn=node, fw=w)
    on, om = _oracle(oracle, "rules-" + hist, sc, 0.7, True)
    assert _oracle(oracle, "rules-" + hist, sc, 0.7, False)[0] == n > on == kept
    gn, gm = _device(sc, 0.7, True)
    assert gn == on and np.array_equal(gm, om)


def test_search_bow_th_low_30(oracle):
    sc = B.scene("flip45")
    n, m = _device(sc, 0.9, True, th_low=30)
    on, om = _oracle(oracle, "flip45", sc, 0.9, True, th_low=30)
    assert n == on and np.array_equal(m, om)
    assert n < _oracle(oracle, "flip45", sc, 0.9, True)[0]


@pytest.mark.parametrize("name", B.DEGENERATE)
def test_search_bow_degenerate_scene_gives_no_match(oracle, name):
    sc = B.degenerate(name)
    for ratio, ori in B.SEARCH_PARAMS:
        n, m = _device(sc, ratio, ori)
        assert n == 0 and m.shape == sc["fn"].shape and (m == -1).all()


def _cut(sc, nk, nf):
    out = {k: v[:nk] for k, v in sc.items() if k[0] == "k"}
    out.update({k: v[:nf] for k, v in sc.items() if k[0] == "f"})
    return out


def test_search_bow_empty_sides():
    sc = B.scene("two129")
    n, m = _device(_cut(sc, 0, 200), 0.9, True)
    assert n == 0 and m.shape == (200,) and (m == -1).all()
    n, m = _device(_cut(sc, 129, 0), 0.9, True)
    assert n == 0 and m.shape == (0,)
    n, m = _device(_cut(sc, 0, 0), 0.9, True)
    assert n == 0 and m.shape == (0,)


@pytest.mark.parametrize("nk,nf", [(2049, 64), (64, 2049)])
def test_search_bow_past_the_cap_is_refused(nk, nf):
    from orb_slam3_ros2_amd._lib import OrbHipError
    sc = B.bow_scene(nk, nf, [5], seed=7)
    with pytest.raises(OrbHipError) as ei:
        _device(sc, 0.9, True)
    assert ei.value.code == -5 and "ORBHIP_ERR_UNSUPPORTED" in str(ei.value)


# ------------------------------------------------------------------------------ transform
_VOCS = {}


def _vocab(name):
    """(Vocabulary, ORBVocabulary on the device), built once."""
    from orb_slam3_ros2_amd import ORBVocabulary
    if name not in _VOCS:
        v = {"ragged1": lambda: B.ragged_vocabulary(5, 5, 1), "ragged2": lambda: B.ragged_vocabulary(5, 5, 2),
             "full_6_3": lambda: Vocabulary.synthetic(6, 3, seed=5),
             "full_10_6": lambda: Vocabulary.synthetic(10, 6, seed=11)}[name]()
        _VOCS[name] = (v, ORBVocabulary(v))
    return _VOCS[name]


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("name", ["ragged1", "ragged2", "full_6_3"])
def test_transform_every_level_bit_exact(oracle, name, n):
    v, voc = _vocab(name)
    f = B.transform_feats(v, n, seed=n + 1)
    for levelsup in (0, v.L - 1, v.L, v.L + 2):
        w, nd, wt = voc.transform_features(f, levelsup)
        assert (w.dtype, nd.dtype, wt.dtype) == (np.int32, np.int32, np.float64)
        assert w.shape == nd.shape == wt.shape == (n,)
        if n == 0:
            continue
        ow, on, ov = oracle.bow_transform(v, f, levelsup)
        assert np.array_equal(w, ow) and np.array_equal(nd, on) and np.array_equal(wt, ov)


@pytest.mark.parametrize("name,levelsup", [("ragged1", 0), ("ragged2", 3), ("full_6_3", 1)])
def test_transform_device_entry_point_ragged_batch(oracle, name, levelsup):
    """orbhip_bow_transform_device on torch tensors: B = 3 frames of capacity 300 holding 300, 0 and
    37 descriptors (counts read on the device); rows from n[f] on are not written."""
    import torch
    from orb_slam3_ros2_amd._lib import check, lib, ptr, torch_stream
    v, voc = _vocab(name)
    nB, cap, counts = 3, 300, [300, 0, 37]
    feats = B.transform_feats(v, nB * cap, seed=31).reshape(nB, cap, 32)
    dev = torch.device("cuda")
    d_desc = torch.from_numpy(feats).to(dev)
    d_n = torch.tensor(counts, dtype=torch.int32, device=dev)
    d_word = torch.full((nB, cap), -7, dtype=torch.int32, device=dev)
    d_node = torch.full((nB, cap), -7, dtype=torch.int32, device=dev)
    d_weight = torch.full((nB, cap), -7.0, dtype=torch.float64, device=dev)
    check(lib().orbhip_bow_transform_device(voc.ctx.handle, voc.handle, ptr(d_desc), ptr(d_n), nB, cap, levelsup,
                                            ptr(d_word), ptr(d_node), ptr(d_weight), torch_stream()),
          "orbhip_bow_transform_device")
    torch.cuda.current_stream().synchronize()
    word, node, weight = d_word.cpu().numpy(), d_node.cpu().numpy(), d_weight.cpu().numpy()
    for f, n in enumerate(counts):
        ow, on, ov = oracle.bow_transform(v, feats[f, :n], levelsup)
        assert np.array_equal(word[f, :n], ow) and np.array_equal(node[f, :n], on)
        assert np.array_equal(weight[f, :n], ov)
        assert (word[f, n:] == -7).all() and (node[f, n:] == -7).all() and (weight[f, n:] == -7.0).all()


def test_transform_device_entry_point_rejects_bad_arguments():
    from orb_slam3_ros2_amd._lib import lib
    _, voc = _vocab("full_6_3")
    one = ctypes.c_void_p(256)          # never dereferenced: the call returns before any launch
    L = lib()
    assert L.orbhip_bow_transform_device(voc.ctx.handle, voc.handle, one, one, 0, 300, 1, one, one, one, None) == -1
    assert L.orbhip_bow_transform_device(voc.ctx.handle, voc.handle, one, one, 3, 0, 1, one, one, one, None) == -1
    assert L.orbhip_bow_transform_device(voc.ctx.handle, voc.handle, one, None, 3, 300, 1, one, one, one, None) == -1


# --------------------------------------------------------------- end to end through a vocabulary
@pytest.mark.parametrize("levelsup,n_nodes", [(5, 10), (6, 1)])
def test_transform_then_search_matches_oracle(oracle, levelsup, n_nodes):
    """ComputeBoW then SearchByBoW as Tracking runs them: nodes and weights from the device
    transform. levelsup 5 gives the 10 level-1 nodes (~60 features each), levelsup 6 the root."""
    v, voc = _vocab("full_10_6")
    sc = dict(B.bow_scene(600, 600, [0], seed=600))
    for side in "kf":
        w, nd, wt = voc.transform_features(sc[side + "d"], levelsup)
        ow, on, ov = oracle.bow_transform(v, sc[side + "d"], levelsup)
        assert np.array_equal(w, ow) and np.array_equal(nd, on) and np.array_equal(wt, ov)
        sc[side + "n"], sc[side + "w"] = nd, wt
    assert len(set(sc["kn"]) | set(sc["fn"])) == n_nodes
    for ratio, ori in B.SEARCH_PARAMS:
        n, m = _matcher(ratio, ori).SearchByBoW(sc["kd"], sc["ka"], sc["kn"], sc["kw"], sc["kv"], sc["fd"],
                                                sc["fa"], sc["fn"], sc["fw"])
        on, om = _oracle(oracle, f"voc{levelsup}", sc, ratio, ori)
        assert n == on and np.array_equal(m, om) and n > 100
