"""SHA-256 digests of every output of a fixed, seeded list of bundle-adjustment solves, one per
path of the back-end's host driver (ba_solve_batch): for proving that a change of the driver
changes no result bit. Reads nothing but the package next to this file.

  python tools/ba_digests.py --out new.json            solve the cases, write their digests
  python tools/ba_digests.py --compare a.json b.json   list the cases whose digests differ (exit 1 if any)
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def digest(results):
    """One entry per BAResult: the digest of each output array and the scalar words."""
    out = []
    for r in results:
        sha = lambda a: hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()   # noqa: E731
        out.append(dict(pose_q=sha(r.pose_q), pose_t=sha(r.pose_t), points=sha(r.points), edge_chi2=sha(r.edge_chi2),
                        edge_depth_ok=sha(r.edge_depth_ok), initial_chi2=sha(np.float64(r.initial_chi2)),
                        final_chi2=sha(np.float64(r.final_chi2)), final_chi2_value=float(r.final_chi2),
                        iterations=int(r.iterations_done), trials=int(r.lm_trials)))
    return out


def cases():
    from ba_stereo_cases import edge_count_problem
    from orb_slam3_ros2_amd import Optimizer
    from orb_slam3_ros2_amd.optimizer import BAProblem
    from orb_slam3_ros2_amd.sharding import shard_problem_nd
    from orb_slam3_ros2_amd.synthetic import synthetic_ba_problem as ba

    small8 = [ba(n_kf=7 + (i % 3), n_pts=60 + 10 * i, seed=60 + i)[0] for i in range(8)]
    rejecting = ba(n_kf=50, n_pts=3000, seed=31, rot_noise=0.1, trans_noise=0.2, pt_noise=0.5)[0]
    loop = ba(n_kf=100, n_pts=3000, layout="loop", window=20, seed=35)[0]
    gba = BAProblem(**{**loop.__dict__, "iterations": 5, "huber_delta": float(np.sqrt(5.99))})
    seg = [shard_problem_nd(gba, r, 2)[0] for r in range(2)]

    def launches_per_trial(opt, run):
        l0 = opt.stats()["dag_launches"]
        res = run()
        return res, (opt.stats()["dag_launches"] - l0) / max(1, res[0].lm_trials)

    out = {}

    def case(name, run, **note):
        opt = Optimizer()
        res, per = launches_per_trial(opt, lambda: run(opt))
        out[name] = dict(results=digest(res), dag_launches_per_trial=per, **note)

    case("lone_lba_register_lds", lambda o: [o.LocalBundleAdjustment(ba(n_kf=7, n_pts=60, seed=51)[0])])
    case("lone_lba_dag", lambda o: [o.LocalBundleAdjustment(ba(n_kf=23, n_pts=300, seed=52)[0])])
    for f in "01":
        with env(ORBHIP_BA_FUSED=f):
            case("batch8_fused" + f, lambda o: o.solve_batch(small8))
    case("batch8_plus_dag_size", lambda o: o.solve_batch(small8 + [ba(n_kf=82, n_pts=900, seed=53)[0]]))
    with env(ORBHIP_BA_SMALL_WORDS="1"):
        case("rejected_trials_large_path", lambda o: [o.LocalBundleAdjustment(rejecting)])
    assert out["rejected_trials_large_path"]["results"][0]["trials"] > \
        out["rejected_trials_large_path"]["results"][0]["iterations"], "no trial was rejected"
    case("stereo_lba", lambda o: [o.LocalBundleAdjustment(edge_count_problem())])
    with env(ORBHIP_ND_MIN="0"):   # n = 594: below the default size for the dissection
        with env(ORBHIP_ND_K="2"):   # (the automatic plan does not pay at this size)
            case("gba_dissection", lambda o: [o.solve(gba)])
        case("shards_local_segments", lambda o: o.solve_shards_local(seg))
        with env(ORBHIP_SHARD_ND="0"):
            case("shards_local_replicated", lambda o: o.solve_shards_local(seg))
    # the dissected forms launch two persistent solves per problem and trial, the plain DAG solve one
    assert out["gba_dissection"]["dag_launches_per_trial"] == 2, "the lone GBA was not dissected"
    assert out["shards_local_segments"]["dag_launches_per_trial"] == 4, "the shards were not solved by segments"
    assert out["lone_lba_dag"]["dag_launches_per_trial"] == 1 and out["lone_lba_register_lds"]["dag_launches_per_trial"] == 0
    case("stop_flag_set", lambda o: [o.LocalBundleAdjustment(ba(n_kf=10, n_pts=200, seed=54)[0], ctypes.c_int(1))])
    return out


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    bad = 0
    for name in sorted(set(a) | set(b)):
        ra, rb = a.get(name, {}).get("results"), b.get(name, {}).get("results")
        diff = []
        if ra is None or rb is None or len(ra) != len(rb):
            diff = ["missing"]
        else:
            diff = sorted({k for x, y in zip(ra, rb) for k in x if x[k] != y[k]})
        bad += bool(diff)
        print(f"{name}: {'DIFFERENT ' + ','.join(diff) if diff else 'identical'} ({len(ra or [])} results)")
    print(f"{len(set(a) | set(b)) - bad} of {len(set(a) | set(b))} cases bit-identical")
    return 1 if bad else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2)
    args = ap.parse_args()
    if args.compare:
        sys.exit(compare(*args.compare))
    res = cases()
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(f"{len(res)} cases -> {args.out}")
