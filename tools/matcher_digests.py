"""SHA-256 digests of every output of a fixed, seeded list of matcher calls, one per device route of
the matcher family (projection searches in every form, SearchForInitialization, SearchByBoW,
SearchForTriangulation, the brute-force match through both finishing kernels): for proving that a
change of those kernels or their host drivers changes no result bit. After each projection search
the route it took (orbhip_test_proj_stats: form, rounds, list entries) is recorded too, so the same
result by another route shows. Reads nothing but the package next to this file and the scene
builders of tests/.

  python tools/matcher_digests.py --out new.json            run the cases, write their digests
  python tools/matcher_digests.py --compare a.json b.json   list the cases whose digests differ (exit 1 if any)
  python tools/matcher_digests.py --time                    per case: the median of 20 calls after a warm-up, in us
"""
import argparse
import contextlib
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PROJ_FORMS = {"default": {}, "two": {"ORBHIP_PROJ_TWO": "1"}, "rounds": {"ORBHIP_PROJ_ROUNDS": "1"},
              "cap2": {"ORBHIP_PROJ_CAP": "2"}, "dma": {"ORBHIP_PROJ_DMA": "1"}}
# orbhip_test_proj_stats' form per switch (cap2: 1 where a list holds more than 2 entries, else 0)
WANT_FORM = {"default": 0, "two": 0, "rounds": 2, "cap2": None, "dma": 0}


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def digest(x):
    """The digest of an array, a scalar (by value) or a tuple / list of them (one entry each)."""
    if isinstance(x, (tuple, list)):
        return [digest(v) for v in x]
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray) and x.ndim > 0:
        return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()
    return int(x)


def cases():
    """[(name, env switches, call, form)]: call() returns the outputs to digest, for a projection search
    with its route (form, rounds, list entries) as the last entry; form = the route's form the case
    is there for, or None."""
    import bow_numpy as B
    import proj_cases as P
    import stereo_track_cases as C
    import triangulation_numpy as T
    from helpers import MATCH_HIST_IDS, MATCH_HISTOGRAMS, planted_match_set, proj_stats
    from orb_slam3_ros2_amd import ORBmatcher
    from orb_slam3_ros2_amd._lib import Context
    from orb_slam3_ros2_amd.matcher import ProjFrame
    from orb_slam3_ros2_amd.synthetic import (synthetic_init_pair, synthetic_projection_scene,
                                              synthetic_stereo_new_points_scene)
    ctx = Context()
    out = []

    def routed(call):
        def run():
            r = call()
            st = proj_stats(ctx)
            return tuple(r) + ((st["form"], st["rounds"], st["entries"]),)
        return run

    # ---- the projection searches: mono and stereo scenes, every form ----
    mono = synthetic_projection_scene(n_kp=1000, n_mp=900, seed=5)
    fmono = ProjFrame(mono["kps"], mono["desc"], mono["pose_q"], mono["pose_t"], mono["fx"], mono["fy"], mono["cx"],
                      mono["cy"], claimed=mono["claimed"])
    chain = P.chain(102, "last", rot_outliers=(3, 50, 51))
    fchain = ProjFrame(chain["kps"], chain["desc"], chain["pose_q"], chain["pose_t"], chain["fx"], chain["fy"],
                       chain["cx"], chain["cy"], claimed=chain["claimed"])
    scenes = [("mono", mono, fmono, None), ("chain102", chain, fchain, None)] + \
             [("stereo_" + m, C.scene(m), C.frame(C.scene(m)), C.last_pose(C.scene(m))) for m in ("forward", "backward")]
    for form, sw in PROJ_FORMS.items():
        for tag, s, f, lp in scenes:
            for ori in (True, False):
                out.append((f"last/{tag}/ori{int(ori)}/{form}", sw, routed(
                    lambda s=s, f=f, lp=lp, ori=ori: ORBmatcher(0.9, ori, ctx=ctx).SearchByProjectionLastFrame(
                        f, s["points"], s["mp_desc"], s["last_octave"], s["last_angle"], s.get("th_last", 15.0),
                        last_pose=lp)), 1 if tag == "chain102" and form == "cap2" else WANT_FORM[form]))
            if tag == "chain102":
                continue
            for th, ratio, far in C.LOCAL_PARAMS[::2]:
                out.append((f"local/{tag}/th{th:g}/{form}", sw, routed(
                    lambda s=s, f=f, th=th, ratio=ratio, far=far: ORBmatcher(ratio, False, ctx=ctx).SearchLocalPoints(
                        f, s["points"], s["normals"], s["min_dist"], s["max_dist"], s["mp_desc"], s["skip"], th=th,
                        far_points=far, th_far=5.0)), WANT_FORM[form]))

    # ---- SearchForInitialization: the parallel rounds and the chain kernel ----
    for seed, n1 in ((9, 1200), (21, 700)):
        k1, d1, k2, d2, prev = synthetic_init_pair(n1=n1, seed=seed)
        for ori in (True, False):
            for form, sw in (("rounds", {}), ("chain", {"ORBHIP_INIT_CHAIN": "1"})):
                out.append((f"init/n{n1}/ori{int(ori)}/{form}", sw,
                            lambda a=(k1, d1, k2, d2, prev), ori=ori: ORBmatcher(0.9, ori, ctx=ctx)
                            .SearchForInitialization(*a, 100), None))

    # ---- SearchByBoW ----
    for name in B.SCENES:
        sc = B.scene(name)
        for ratio, ori in B.SEARCH_PARAMS:
            out.append((f"bow/{name}/r{ratio:g}/ori{int(ori)}", {},
                        lambda sc=sc, ratio=ratio, ori=ori: ORBmatcher(ratio, ori, ctx=ctx).SearchByBoW(
                            sc["kd"], sc["ka"], sc["kn"], sc["kw"], sc["kv"], sc["fd"], sc["fa"], sc["fn"], sc["fw"]),
                        None))

    # ---- SearchForTriangulation, mono and stereo ----
    tri = [(f"parity{k}", T.parity_scene(k)) for k in range(len(T.PARITY_SCENES))] + \
          [("stereo", synthetic_stereo_new_points_scene(300, 3, seed=0))]
    for tag, s in tri:
        for ori in (True, False):
            out.append((f"tri/{tag}/ori{int(ori)}", {},
                        lambda s=s, ori=ori: ORBmatcher(0.6, ori, ctx=ctx).SearchForTriangulation(
                            s["kf1"], s["neighbours"], s["scale_factors"], s["level_sigma2"]), None))

    # ---- the brute-force match: one pair through k_match_fused and k_match_top2 + k_match_finish ----
    for hid, (hist, _, _) in zip(MATCH_HIST_IDS, MATCH_HISTOGRAMS):
        ds = planted_match_set(1250, 1100, hist, (0, 40), seed=40 + len(hist))
        for path, sw in (("fused", {}), ("finish", {"ORBHIP_MATCH_UNFUSED": "1"})):
            out.append((f"match/{hid}/{path}", sw,
                        lambda ds=ds: ORBmatcher(0.9, True, ctx=ctx).match_bf(ds.q, ds.qa, ds.t, ds.ta, 50), None))
    ds = planted_match_set(1250, 1100, {2: 300, 5: 200, 9: 100, 12: 20}, (0, 60), seed=77)
    for path, sw in (("fused", {}), ("finish", {"ORBHIP_MATCH_UNFUSED": "1"})):
        out.append((f"match/ori0/{path}", sw,
                    lambda ds=ds: ORBmatcher(0.9, False, ctx=ctx).match_bf(ds.q, ds.qa, ds.t, ds.ta, 50), None))

    # ---- a batch of 5 pairs (frame f matched against frame f + 1): k_match_top2<256> + k_match_finish ----
    cap, counts = 640, [640, 600, 513, 640, 65, 17]
    frames, nxt = [None] * len(counts), None
    for f in range(len(counts) - 1, -1, -1):
        if nxt is None:
            rng = np.random.default_rng(900 + f)
            frames[f] = (rng.integers(0, 256, (counts[f], 32), dtype=np.uint8),
                         rng.integers(0, 360, counts[f]).astype(np.float32))
        else:
            n = counts[f]
            h = {2: n // 4, 5: n // 8, 9: n // 16, 12: n // 32}
            p = planted_match_set(n, len(nxt[0]), {b: c for b, c in h.items() if c}, (0, 60), seed=900 + f, trains=nxt)
            frames[f] = (p.q, p.qa)
        nxt = frames[f]
    rng = np.random.default_rng(9)
    kps = rng.uniform(0, 360, (len(counts), cap, 6)).astype(np.float32)
    desc = rng.integers(0, 256, (len(counts), cap, 32), dtype=np.uint8)
    for f, (d, a) in enumerate(frames):
        desc[f, :len(d)] = d
        kps[f, :len(d), 3] = a

    def batch():
        import torch
        dev = torch.device("cuda:0")
        npairs = len(counts) - 1
        mm = torch.zeros((npairs, cap), dtype=torch.int32, device=dev)
        outs = (mm, torch.zeros_like(mm), torch.zeros_like(mm), torch.zeros(npairs, dtype=torch.int32, device=dev))
        ORBmatcher(0.9, True, ctx=ctx).match_pairs_device(torch.from_numpy(kps).to(dev), torch.from_numpy(desc).to(dev),
                                                          torch.from_numpy(np.array(counts, np.int32)).to(dev), *outs)
        torch.cuda.synchronize()
        mm, bb, ss, nm = (x.cpu().numpy() for x in outs)
        # rows past a pair's query count are unspecified
        return [a[p, :counts[p]] for p in range(npairs) for a in (mm, bb, ss)] + [nm]
    out.append(("match/batch5", {}, batch, None))
    return out


def run(timed):
    res = {}
    for name, sw, call, want_form in cases():
        with env(**sw):
            r = call()
            if want_form is not None:
                assert r[-1][0] == want_form, (name, "ran on form", r[-1][0], "not", want_form)
            if timed:
                ts = []
                for _ in range(3):
                    call()
                for _ in range(20):
                    t0 = time.perf_counter()
                    call()
                    ts.append(time.perf_counter() - t0)
                res[name] = round(1e6 * statistics.median(ts), 1)
                print(f"{name}: {res[name]} us", flush=True)
            else:
                res[name] = dict(results=digest(r))
    return res


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = [n for n in sorted(set(a) | set(b)) if a.get(n) != b.get(n)]
    for n in bad:
        print(f"{n}: DIFFERENT" if n in a and n in b else f"{n}: missing")
    print(f"{len(set(a) | set(b)) - len(bad)} of {len(set(a) | set(b))} cases bit-identical")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    res = run(args.time)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1, sort_keys=True)
        print(f"{len(res)} cases -> {args.out}")
