"""Shared test helpers: compare product keypoints/descriptors with the oracle's; the numerics of
the dense-solver tests (SPD test matrices, a long-double reference solve, the backward error);
the BA result comparison against the oracle; the brute-force matcher's route hook and data sets
with matches planted by construction; device frame layouts (padded rows, offset base pointers, odd
strides inside a poisoned buffer) for the extraction tests; the stage-by-stage comparison of one
frame's extraction (pyramid, FAST candidates, kept keypoints, error word) with the oracle."""
import numpy as np

from orb_slam3_ros2_amd._lib import KP_DTYPE

U = 2.0 ** -53          # fp64 unit roundoff
ETA_CAP = 8.0           # backward error cap of the dense solvers, in units of U
FWD_CAP = 8.0           # forward error cap, in units of cond * U
REL = 1e-4              # north_star: BA state against the oracle
# The condition number the forward bound uses on band_spd's family M M^T + n I: the family's own
# bound (M M^T has its spectrum in [0, 4n]), not each matrix's 2-norm value (1.2 .. 5). A 2-norm
# condition number does not bound a max-norm forward error, and the band matrices show it: in units
# of their own cond_2 u, fp64 LAPACK's Cholesky is at 2.2, its LU at 6.6 and the fp64 model of the
# panel algorithm at 3.8 (n = 600, band), which would leave the cap of 8 two times above the
# references instead of the six to ten times it has on every other case. In units of 5 u the same
# references are at 0.8 / 2.4 / 1.4 (band) and 1.3 / 2.2 / 1.2 (dense).
BAND_COND = 5.0


def spd_with_spectrum(n: int, cond: float, rng) -> np.ndarray:
    """A = Q diag(ev) Q^T, Q from the QR of a normal matrix, ev = geomspace(1, cond, n) * 1e3."""
    Q, _ = np.linalg.qr(rng.normal(size=(n, n)))
    ev = np.geomspace(1.0, cond, n) * 1e3
    A = (Q * ev) @ Q.T
    return 0.5 * (A + A.T)


def band_spd(n: int, shape: str, rng) -> np.ndarray:
    """M M^T + n I (cond <= 5): M dense ("dense"), lower banded with bandwidth 120 ("band"), or the
    band plus a coupling of the last 120 rows to the first 120 columns ("loop", C5's shape)."""
    if shape == "dense":
        M = rng.normal(size=(n, n))
    else:
        bw = 120
        M = np.zeros((n, n))
        for i in range(n):
            lo = max(0, i - bw)
            M[i, lo:i + 1] = rng.normal(size=i + 1 - lo)
        if shape == "loop":
            M[n - 120:, :120] = rng.normal(size=(120, 120)) * 0.3
    A = M @ M.T + n * np.eye(n)
    return 0.5 * (A + A.T)


def _need_longdouble():
    # not a skip: without an extended type the reference below is no better than the code under test
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "np.longdouble has no 64-bit mantissa on this host"


def solve_longdouble(A: np.ndarray, b: np.ndarray) -> np.ndarray:
    """x = A^{-1} b by a column Cholesky and two triangular solves, all in np.longdouble."""
    _need_longdouble()
    n = A.shape[0]
    L = np.tril(A).astype(np.longdouble)
    for j in range(n):
        if j:
            L[j:, j] -= L[j:, :j] @ L[j, :j]
        d = np.sqrt(L[j, j])
        assert d > 0, "reference Cholesky: not positive definite"
        L[j, j] = d
        L[j + 1:, j] /= d
    y = b.astype(np.longdouble)
    for j in range(n):           # column-oriented forward solve
        y[j] /= L[j, j]
        y[j + 1:] -= L[j + 1:, j] * y[j]
    for j in range(n - 1, -1, -1):   # backward solve with L^T
        y[j] /= L[j, j]
        y[:j] -= L[j, :j] * y[j]
    return y


def backward_error(A: np.ndarray, x: np.ndarray, b: np.ndarray) -> float:
    """The normwise backward error |b - A x|_inf / (|A|_inf |x|_inf + |b|_inf), in long double."""
    _need_longdouble()
    Al, xl, bl = A.astype(np.longdouble), x.astype(np.longdouble), b.astype(np.longdouble)
    r = np.abs(bl - Al @ xl).max()
    return float(r / (np.abs(Al).sum(axis=1).max() * np.abs(xl).max() + np.abs(bl).max()))


def check_solve(A: np.ndarray, x: np.ndarray, b: np.ndarray, cond: float | None = None) -> tuple:
    """The solver yardstick: backward error <= ETA_CAP u and, when cond is given, the forward error
    against solve_longdouble <= FWD_CAP cond u. The caps come from the references, not from the
    kernels: fp64 LAPACK stays below 0.37 u / 0.42 cond u and an fp64 model of the panel algorithm
    (explicit inverses of the diagonal factors) below 0.82 u / 0.46 cond u on these families.
    Returns (eta / u, forward / (cond u) or None) and prints them (pytest -s shows the figures)."""
    eta = backward_error(A, x, b) / U
    fwd = None
    if cond is not None:
        ref = solve_longdouble(A, b)
        fwd = float(np.abs(x.astype(np.longdouble) - ref).max() / np.abs(ref).max()) / (cond * U)
    print(f"SOLVE n={A.shape[0]} cond={cond} eta/u={eta:.3f} fwd/(cond u)={fwd if fwd is None else round(fwd, 3)}")
    assert eta <= ETA_CAP, (eta, fwd)
    assert fwd is None or fwd <= FWD_CAP, (eta, fwd)
    return eta, fwd


def qsign(q):
    q = q.astype(np.float64)
    return q * np.where(q[:, 3:4] < 0, -1.0, 1.0)


def compare_ba(g, o, prob, exact_schedule=True, point_rel=REL):
    """A GPU BAResult against the oracle's dict: the LM schedule, chi2, poses and points."""
    # Run to full convergence, g2o stops on rho == 0 (bit-equal chi2 of two trials): where that
    # happens depends on the last bits of the sums, so the schedule is compared only for runs
    # that stop on the iteration budget (the LocalBundleAdjustment case, optimize(10)).
    dq = np.abs(qsign(g.pose_q) - qsign(o["pose_q"])).max()
    tscale = max(1.0, np.abs(o["pose_t"]).max())
    dt = np.abs(g.pose_t.astype(np.float64) - o["pose_t"]).max() / tscale
    pscale = max(1.0, np.abs(o["points"]).max())
    dp = np.abs(g.points.astype(np.float64) - o["points"]).max() / pscale
    dchi = abs(g.final_chi2 - o["final_chi2"]) / max(abs(o["final_chi2"]), 1e-300)
    print(f"BA schedule gpu {g.iterations_done}/{g.lm_trials} oracle {o['iterations_done']}/{o['lm_trials']} "
          f"dchi2={dchi:.2e} dq={dq:.2e} dt={dt:.2e} dp={dp:.2e}")
    if exact_schedule:
        assert (g.iterations_done, g.lm_trials) == (o["iterations_done"], o["lm_trials"])
    assert abs(g.final_chi2 - o["final_chi2"]) <= REL * abs(o["final_chi2"])
    assert dq < REL and dt < REL and dp < point_rel, (dq, dt, dp)
    gout = (g.edge_chi2 > 5.991) | (g.edge_depth_ok == 0)
    oout = (o["edge_chi2"] > 5.991) | (o["edge_depth_ok"] == 0)
    # flags may only differ for edges whose chi2 sits within rounding of the threshold
    diff = np.nonzero(gout != oout)[0]
    assert all(abs(o["edge_chi2"][e] - 5.991) < 1e-3 for e in diff)


def oracle_kps_to_struct(k6: np.ndarray) -> np.ndarray:
    out = np.zeros(k6.shape[0], KP_DTYPE)
    for i, f in enumerate(["x", "y", "size", "angle", "response"]):
        out[f] = k6[:, i]
    out["octave"] = k6[:, 5].astype(np.int32)
    return out


def diff_report(gk, gd, ok, od, max_lines=10) -> str:
    lines = [f"n gpu={len(gk)} oracle={len(ok)}"]
    n = min(len(gk), len(ok))
    for f in KP_DTYPE.names:
        bad = np.nonzero(gk[f][:n] != ok[f][:n])[0]
        if len(bad):
            lines.append(f"field {f}: {len(bad)} mismatches, first idx {bad[:5].tolist()}")
    if gd is not None and od is not None:
        bad = np.nonzero(np.any(gd[:n] != od[:n], axis=1))[0]
        if len(bad):
            lines.append(f"desc: {len(bad)} rows differ, first {bad[:5].tolist()}")
    for i in range(min(n, max_lines)):
        if any(gk[f][i] != ok[f][i] for f in KP_DTYPE.names):
            lines.append(f"  [{i}] gpu={gk[i]} oracle={ok[i]}")
    return "\n".join(lines)


# ---- ORBmatcher's rotation-consistency filter, restated once for every test model ----

HISTO_LENGTH = 30


def c_round(v) -> int:
    """C round() / roundf(): halves away from zero (np.round rounds them to even)."""
    v = float(v)
    return int(np.floor(v + 0.5)) if v >= 0 else -int(np.floor(-v + 0.5))


def rotation_bin(angle1, angle2) -> int:
    """rot = angle1 - angle2 (+ 360 when negative), bin = round(rot * (1.0f / HISTO_LENGTH)), bin 30 -> 0:
    every float operation of the reference as one np.float32 operation."""
    f32 = np.float32
    rot = f32(angle1) - f32(angle2)
    if rot < 0.0:
        rot = rot + f32(360.0)
    b = c_round(rot * (f32(1.0) / f32(HISTO_LENGTH)))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima over the histogram's bin sizes: (ind1, ind2, ind3), -1 = dropped."""
    f32 = np.float32
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        s = int(s)
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


# Small histograms at the filter's two rules, for scenes of one match per query: {bin: matches} ->
# matches kept. "12-1": 1 < 0.1f * 12, the single match goes. "ties": four equal bins, the three of
# lower index stay. A pair of angles (30 b, 0) lands in bin b (30 b * (1.0f / 30) rounds to b).
ROT_EDGE_HISTS = {"12-1": ({2: 12, 5: 1}, 12), "ties": ({3: 6, 7: 6, 9: 6, 11: 6}, 18)}


def rot_edge_bins(name):
    """(the bin of each of the scene's matches in a fixed shuffled order, matches kept)."""
    hist, kept = ROT_EDGE_HISTS[name]
    bins = np.concatenate([np.full(c, b) for b, c in hist.items()])
    return np.random.default_rng(len(bins)).permutation(bins), kept


# ---- the brute-force matcher: its dispatch route and data sets with matches by construction ----

def match_route(npairs: int, max_q: int, max_t: int, fused_allowed: bool = True) -> dict:
    """The matcher's dispatch decision for a call shape (the function run_match itself follows),
    under the current ORBHIP_MATCH_* switches. kernel: "fused" or "tc64" / "tc256" / "tc512" /
    "tc1024" (k_match_top2<N> + k_match_finish); nch chunks per pair; xrun the xcd_runs run length
    (0 = dispatch order); pk 1 = 4-byte partials."""
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 4)()
    assert lib().orbhip_test_match_route(npairs, max_q, max_t, int(fused_allowed), out) == 0
    return {"kernel": "fused" if out[0] == 0 else f"tc{out[0]}", "nch": out[1], "xrun": out[2], "pk": out[3]}


def proj_route(n: int, nq: int, max_octave: int = 0) -> dict:
    """The projection searches' decisions for a call's sizes (the functions both searches call),
    under the current ORBHIP_PROJ_* switches: lists = the list/resolve form applies (max_octave
    stands for the keypoints' largest octave), ent_cap = list entries the resolve holds in LDS,
    cap = entries per list, fused = one launch."""
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 4)()
    assert lib().orbhip_test_proj_route(n, nq, max_octave, out) == 0
    return {"lists": bool(out[0]), "ent_cap": out[1], "cap": out[2], "fused": bool(out[3])}


def proj_stats(ctx) -> dict:
    """The last projection search on this context: form 0 = lists + resolve, 1 = a list overflowed
    and the rounds produced the result, 2 = rounds only, -1 = none yet or no queries; its rounds;
    the list entries the resolve saw (form 0) and that call's ent_cap."""
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 4)()
    assert lib().orbhip_test_proj_stats(ctx.handle, out) == 0
    return {"form": out[0], "rounds": out[1], "entries": out[2], "ent_cap": out[3]}


def init_route(n1: int, n2: int, nq0: int, nr0: int) -> dict:
    """SearchForInitialization's envelope for a call's sizes (the function init_search follows): rc =
    the return code the sizes earn (0, -1 ORBHIP_ERR_ARG, -5 ORBHIP_ERR_UNSUPPORTED), lds = the
    chain's dynamic LDS bytes, list_cap = entries per query list, cap = parallel rounds at most."""
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 4)()
    assert lib().orbhip_test_init_route(n1, n2, nq0, nr0, out) == 0
    return {"rc": out[0], "lds": out[1], "list_cap": out[2], "cap": out[3]}


def init_stats(ctx) -> dict:
    """The last SearchForInitialization on this context: form 0 = the rounds converged, 1 = the chain
    after a claim-slot overflow, 2 = the chain after the round cap, 3 = the chain by ORBHIP_INIT_CHAIN,
    -1 = none yet / no queries / an error; round = the round that changed nothing (else the rounds
    run); init_ahead after the call; the octave-0 counts; the queries with need == 1 and need == 2."""
    import ctypes
    from orb_slam3_ros2_amd._lib import lib
    out = (ctypes.c_int32 * 8)()
    assert lib().orbhip_test_init_stats(ctx.handle, out) == 0
    return {"form": out[0], "round": out[1], "init_ahead": out[2], "nq0": out[3], "nr0": out[4], "need1": out[5],
            "need2": out[6]}


class PlantedSet:
    """q (nq, 32) / qa (nq,), t (nt, 32) / ta (nt,); per query: train (the train it was planted
    from, -1 = random query), bin (its rotation bin), flips (its distance to that train)."""

    def __init__(self, q, qa, t, ta, train, bin_, flips):
        self.q, self.qa, self.t, self.ta, self.train, self.bin, self.flips = q, qa, t, ta, train, bin_, flips

    @property
    def planted(self):
        return self.train >= 0


def _flip_masks(rng, n: int):
    """rank[i, bit]: the position of `bit` in query i's own random bit order; flipping the bits of
    rank < k gives distance exactly k, and the same k always picks the same bits."""
    perm = np.argsort(rng.random((n, 256)), axis=1)
    rank = np.empty((n, 256), np.int64)
    rank[np.arange(n)[:, None], perm] = np.arange(256)[None, :]
    return rank


def _mask_bytes(rank_row, k):
    return np.packbits(rank_row < k, axis=-1, bitorder="little")


def planted_match_set(nq: int, nt: int, hist=None, flips=(0, 40), seed=0, plants=(), trains=None) -> PlantedSet:
    """Random descriptors never match (best ~ 100), so the matches are built in.

    Trains: random 32-byte descriptors, angles integer degrees in [0, 360) (or `trains` = (t, ta),
    copied). For every bin b of `hist` = {bin: count}, `count` queries (random positions) copy a
    train (distinct trains while nt allows) and flip k bits, k uniform in `flips` (inclusive); their
    angle is train_angle + rot (- 360 from 360 on), rot = 30 b for b in 0..11 and 350 for b = 12, so
    every angle and every difference is an exact float and the query lands in bin b. `plants` =
    (query, train index, k) fix distances exactly: the first plant of a query derives the query
    from that train (bin 0); a further plant of the same query overwrites its train with the query
    flipped in k bits (the same k picks the same bits: two plants with equal k make two equal
    trains). Planted queries and trains of `plants` are kept apart from those of `hist`. Every
    other query is random."""
    rng = np.random.default_rng(seed)
    if trains is None:
        t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
        ta = rng.integers(0, 360, nt).astype(np.float32)
    else:
        t, ta = np.array(trains[0], np.uint8).reshape(nt, 32), np.array(trains[1], np.float32).reshape(nt)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    qa = rng.integers(0, 360, nq).astype(np.float32)
    train = np.full(nq, -1, np.int64); bin_ = np.full(nq, -1, np.int64); nflip = np.full(nq, -1, np.int64)
    rank = _flip_masks(rng, nq)
    used_q, used_t = set(), set()
    for (qi, ti, k) in plants:
        assert 0 <= qi < nq and 0 <= ti < nt and 0 <= k <= 256 and ti not in used_t
        used_t.add(ti)
        if qi not in used_q:
            used_q.add(qi)
            q[qi] = t[ti] ^ _mask_bytes(rank[qi], k)
            qa[qi] = ta[ti]
            train[qi], bin_[qi], nflip[qi] = ti, 0, k
        else:
            t[ti] = q[qi] ^ _mask_bytes(rank[qi], k)
            ta[ti] = qa[qi]
            if (k, ti) < (nflip[qi], train[qi]):
                train[qi], nflip[qi] = ti, k
    hist = dict(hist or {})
    total = sum(hist.values())
    assert all(0 <= b <= 12 for b in hist) and total <= nq - len(used_q) and (total == 0 or nt > len(used_t))
    if total:
        free_q = np.array([i for i in range(nq) if i not in used_q])
        free_t = np.array([i for i in range(nt) if i not in used_t])
        qs = rng.permutation(free_q)[:total]
        ts = rng.permutation(free_t)[:total] if total <= len(free_t) else rng.choice(free_t, total)
        ks = rng.integers(flips[0], flips[1] + 1, total)
        bins = np.concatenate([np.full(c, b) for b, c in sorted(hist.items())])
        rot = np.where(bins == 12, 350, 30 * bins).astype(np.float32)
        q[qs] = t[ts] ^ _mask_bytes(rank[qs], ks[:, None])
        a = ta[ts] + rot
        qa[qs] = np.where(a >= 360, a - 360, a).astype(np.float32)
        train[qs], bin_[qs], nflip[qs] = ts, bins, ks
    return PlantedSet(q, qa, t, ta, train, bin_, nflip)


# histogram {bin: count} -> (bins ComputeThreeMaxima keeps, matches kept)
MATCH_HISTOGRAMS = [
    ({3: 40, 7: 40, 9: 40, 11: 40}, (3, 7, 9), 120),      # four equal bins: the lower indices win
    ({0: 100, 5: 10, 8: 9}, (0, 5), 110),                 # 10 < 0.1f * 100 is false, 9 is below
    ({0: 99, 5: 10, 8: 9}, (0, 5), 109),
    ({0: 101, 5: 10, 8: 10}, (0,), 101),                  # 10 < 10.1: the second AND the third go
    ({2: 100, 6: 9, 7: 9}, (2,), 100),
    ({4: 100, 1: 10, 12: 10, 6: 10}, (4, 1, 6), 120),     # three tied runners-up: bin 12 is the one dropped
    ({12: 7}, (12,), 7),                                  # rot 350 -> the last bin that can fill
    ({0: 1}, (0,), 1),
    ({}, (), 0),
    ({1: 5, 2: 6, 3: 7, 4: 8}, (4, 3, 2), 21),
]
MATCH_HIST_IDS = ["-".join(f"{b}x{c}" for b, c in h.items()) or "empty" for h, _, _ in MATCH_HISTOGRAMS]


# ---- device frame layouts: padded rows, offset base pointers, odd strides ----

POISONS = (0xFF, "random")   # a constant, and a seeded byte stream (FAST corners wherever it is sampled)


def place_frames(frames_u8: np.ndarray, stride: int, offset: int, frame_stride: int, poison):
    """frames_u8 [B, H, W] inside one poisoned uint8 CUDA buffer of offset + (B - 1) * frame_stride +
    H * stride + 64 bytes: row r of frame f at byte offset + f * frame_stride + r * stride. Every
    byte that is not a pixel (row padding, frame gaps, the bytes before and after) holds `poison`:
    an int = that constant, "random" = a seeded random stream. Returns the [B, H, W] view
    (stride(0) = frame_stride, stride(1) = stride, storage offset = offset)."""
    import torch
    B, H, W = frames_u8.shape
    assert frames_u8.dtype == np.uint8 and stride >= W and offset >= 0 and (B == 1 or frame_stride >= stride * H)
    size = offset + (B - 1) * frame_stride + H * stride + 64
    if poison == "random":
        fill = np.random.default_rng(0xB0B).integers(0, 256, size, dtype=np.uint8)
    else:
        fill = np.full(size, int(poison), np.uint8)
    buf = torch.from_numpy(fill).to("cuda")
    assert buf.data_ptr() % 256 == 0, "the base allocation is expected to be 256-byte aligned"
    view = torch.as_strided(buf, (B, H, W), (frame_stride, stride, 1), offset)
    view.copy_(torch.from_numpy(np.ascontiguousarray(frames_u8)).to("cuda"))
    torch.cuda.synchronize()
    return view


def frame_layout(lid: str, w: int, h: int) -> tuple:
    """(stride, offset, frame_stride) of a named layout at frame size w x h. P packed; A rows and
    frames padded, all 4-byte aligned; A4 the stride rounded up to 4 (w % 4 != 0): a row's last
    dword straddles image and padding; M1 / M2 / M3 an aligned stride behind a base pointer off by
    1 / 2 / 3; O / O2 / O3 the smallest stride >= w that is 1 / 2 / 3 mod 4; X an aligned stride
    with a frame stride that is 2 mod 4: even frames aligned, odd frames not."""
    r4 = (w + 3) & ~3
    if lid == "P":
        return w, 0, w * h
    if lid == "A":
        return r4 + 64, 0, (r4 + 64) * h + 256
    if lid == "A4":
        assert w % 4 != 0
        return r4, 0, r4 * h
    if lid in ("M1", "M2", "M3"):
        return r4 + 64, int(lid[1]), (r4 + 64) * h
    if lid in ("O", "O2", "O3"):
        m = 1 if lid == "O" else int(lid[1])
        s = w + ((m - w) % 4)
        return s, 0, s * h
    if lid == "X":
        return r4 + 64, 0, (r4 + 64) * h + 2
    raise ValueError(lid)


def layout_class(lid: str) -> str:
    return {"P": "packed", "A": "dword-padded", "A4": "dword-padded", "X": "mixed-per-frame"}.get(
        lid, "misaligned-byte" if lid.startswith("M") else "odd-stride-byte")


def extract_device_frames(ext, frames_t, lap=(0, 1000)) -> list:
    """extract_batch_device on a [B, H, W] CUDA view -> per frame (n, mono, keypoints as KP_DTYPE,
    descriptors [n, 32])."""
    import torch
    B, H, W = frames_t.shape
    cap = ext.max_keypoints(W, H)
    dev = frames_t.device
    kps = torch.zeros((B, cap, 6), dtype=torch.float32, device=dev)
    desc = torch.zeros((B, cap, 32), dtype=torch.uint8, device=dev)
    n = torch.full((B,), -1, dtype=torch.int32, device=dev)
    mono = torch.full((B,), -1, dtype=torch.int32, device=dev)
    ext.extract_batch_device(frames_t, kps, desc, n, mono, lap)
    torch.cuda.synchronize()
    kh, dh, nh, mh = kps.cpu().numpy(), desc.cpu().numpy(), n.cpu().numpy(), mono.cpu().numpy()
    out = []
    for f in range(B):
        c = max(int(nh[f]), 0)
        out.append((int(nh[f]), int(mh[f]), np.frombuffer(kh[f, :c].tobytes(), KP_DTYPE), dh[f, :c].copy()))
    return out


def assert_frames_equal_oracle(got: list, want: list, what="") -> None:
    """got: extract_device_frames' list; want: per frame (mono, keypoints KP_DTYPE, descriptors).
    n, monoIndex, all six keypoint fields and the descriptor bytes are equal, and n > 0."""
    assert len(got) == len(want)
    for f, ((n, mono, gk, gd), (omono, ok, od)) in enumerate(zip(got, want)):
        same = (n == len(ok) and mono == omono and all(np.array_equal(gk[k], ok[k]) for k in KP_DTYPE.names)
                and np.array_equal(gd, od))
        assert same, f"{what} frame {f}: n gpu={n} monoIndex gpu={mono} oracle={omono}\n" + diff_report(gk, gd, ok, od)
        assert n > 0, f"{what} frame {f}: no keypoints"


# ---- extraction stage by stage: the device's intermediates of one host frame against the oracle's ----

LEVEL_KP_DTYPE = np.dtype([("x", np.int16), ("y", np.int16), ("srl", np.uint32)])   # orbhip_plan.h LevelKp


def extract_debug(ext, img, lap=(0, 1000)) -> dict:
    """orbhip_test_extract_debug + orbhip_test_cells on one host frame (the host-frame path with the
    context's plan): pyr = levels 1.. as [h, w] arrays, cand = packed candidates by slot, ccnt = per
    cell, cells = (level, x0, y0, wc, hc, slot_off) rows, lvl = LevelKp slots, lcnt / lnlap per
    level, sizes = (n_slots_total, n_cells_total, kp_slots_total, device error word)."""
    from orb_slam3_ros2_amd._lib import lib, ptr
    L = lib()
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    nl = ext.nlevels
    info = ext.level_info(w, h)
    sizes = np.zeros(4, np.int32)
    rc = L.orbhip_test_extract_debug(ext.ctx.handle, ptr(img), w, h, int(lap[0]), int(lap[1]), None, None, None,
                                     None, None, None, ptr(sizes))
    assert rc == 0, f"orbhip_test_extract_debug (size query): {rc}"
    dims = [(int(info["h"][l]), int(info["w"][l])) for l in range(nl)]
    pyr = np.zeros(max(sum(a * b for a, b in dims[1:]), 1), np.uint8)   # never a null pointer: null = size query
    cand = np.zeros(max(int(sizes[0]), 1), np.uint32)
    ccnt = np.zeros(max(int(sizes[1]), 1), np.int32)
    lvl = np.zeros(max(int(sizes[2]), 1), LEVEL_KP_DTYPE)
    lcnt = np.zeros(nl, np.int32)
    lnlap = np.zeros(nl, np.int32)
    rc = L.orbhip_test_extract_debug(ext.ctx.handle, ptr(img), w, h, int(lap[0]), int(lap[1]), ptr(pyr), ptr(cand),
                                     ptr(ccnt), ptr(lvl), ptr(lcnt), ptr(lnlap), ptr(sizes))
    assert rc == 0, f"orbhip_test_extract_debug: {rc}"
    cells = np.zeros((max(int(sizes[1]), 1), 6), np.int32)
    assert L.orbhip_test_cells(ext.ctx.handle, w, h, ptr(cells), int(sizes[1])) == int(sizes[1])
    levels, off = [], 0
    for a, b in dims[1:]:
        levels.append(pyr[off: off + a * b].reshape(a, b))
        off += a * b
    return dict(pyr=levels, cand=cand[: sizes[0]], ccnt=ccnt[: sizes[1]], cells=cells[: sizes[1]], lvl=lvl[: sizes[2]],
                lcnt=lcnt, lnlap=lnlap, sizes=sizes, info=info)


def _multiset_diff(got, want, what, names):
    """got / want: integer arrays [n, k]. Equal as multisets, else an AssertionError naming `what`, both
    sizes and up to five entries that only one side has."""
    from collections import Counter
    g = got[np.lexsort(got.T[::-1])] if len(got) else got
    o = want[np.lexsort(want.T[::-1])] if len(want) else want
    if g.shape == o.shape and np.array_equal(g, o):
        return
    cg, co = Counter(map(tuple, got.tolist())), Counter(map(tuple, want.tolist()))
    only_g = sorted((cg - co).elements())[:5]
    only_o = sorted((co - cg).elements())[:5]
    raise AssertionError(f"{what}: gpu {len(got)} oracle {len(want)} {names}; only on the gpu {only_g}; "
                         f"only in the oracle {only_o}")


def compare_extract_stages(ext, oracle, img, lap=(0, 1000), what="") -> dict:
    """Every stage of one host frame on the device against the oracle, exactly, in pipeline order; the
    first stage and level that differ are named, with up to five differing entries.

    pyramid      levels 1 .. L - 1 byte for byte against oracle.pyramid.
    candidates   per level the multiset of (x, y, score) and its size against oracle.extract_levels'
                 cand list. Both sides count x and y from the border box's origin (16, 16) of the
                 level: the device packs cg.x0 + 3 + px - G.min_bx (k_fast_cells, at pack_cand), the
                 oracle returns fast16's window position plus the cell's offset j * wCell, before
                 minBorderX is added (vToDistributeKeys). A cell's run is cand[slot_off : slot_off + ccnt]
                 from the orbhip_test_cells table; it must fit the cell's slot range.
    kept         per level lvl_cnt LevelKp entries (x, y, score byte) against the kept list, as a
                 multiset and in number. Both sides are level pixels: the device writes cand_x + min_bx
                 (k_octree's output loop), the oracle adds minBorderX after DistributeOctTree. A level's
                 slots start at the sum of the kp_cap = n_feat + 3 + 4 * nIni of the levels before it,
                 nIni = round(box_w / box_h) as in DistributeOctTree; the caps must add up to
                 kp_slots_total. The lapping flags' number per level is the oracle's as well.
    error word   sizes[3] == 0.
    Nothing is left out: every level, every cell, no tolerance. Returns the device's stages."""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    nl = ext.nlevels
    d = extract_debug(ext, img, lap)
    tag = f"{what} {w}x{h}".strip()
    err = int(d["sizes"][3])
    opyr = oracle.pyramid(img, ext.scaleFactor, nl)
    for l in range(1, nl):
        g, o = d["pyr"][l - 1], opyr[l]
        assert g.shape == o.shape, f"{tag}: stage pyramid level {l}: size gpu {g.shape} oracle {o.shape} (err {err})"
        if not np.array_equal(g, o):
            ys, xs = np.nonzero(g != o)
            first = [(int(x), int(y), int(g[y, x]), int(o[y, x])) for y, x in zip(ys[:5], xs[:5])]
            raise AssertionError(f"{tag}: stage pyramid level {l}: {len(ys)} bytes differ, first (x, y, gpu, oracle) "
                                 f"{first} (err {err})")
    ocand, okept = oracle.extract_levels(img, ext.nfeatures, ext.scaleFactor, nl, ext.iniThFAST, ext.minThFAST)
    cells, ccnt, cand = d["cells"], d["ccnt"], d["cand"]
    ends = np.append(cells[1:, 5], d["sizes"][0]) if len(cells) else np.zeros(0, np.int32)
    for l in range(nl):
        runs = []
        for ci in np.flatnonzero(cells[:, 0] == l):
            n, lo, hi = int(ccnt[ci]), int(cells[ci, 5]), int(ends[ci])
            assert 0 <= n <= hi - lo, f"{tag}: stage candidates level {l}: cell {ci} holds {n} in {hi - lo} slots (err {err})"
            runs.append(cand[lo: lo + n])
        packed = np.concatenate(runs) if runs else np.zeros(0, np.uint32)
        got = np.stack([packed & 0xFFF, (packed >> 12) & 0xFFF, packed >> 24], axis=1).astype(np.int64)
        want = ocand[l][:, [0, 1, 4]].astype(np.int64)
        assert np.array_equal(want, ocand[l][:, [0, 1, 4]]), "the oracle's candidates are integers"
        _multiset_diff(got, want, f"{tag}: stage candidates level {l} (err {err})", "(x, y, score) from the box origin")
    f32 = np.float32
    base, scales = 0, d["info"]["scales"]
    for l in range(nl):
        lw, lh = int(d["info"]["w"][l]), int(d["info"]["h"][l])
        n_ini = c_round(f32(lw - 32) / f32(lh - 32))
        cap = int(d["info"]["feats"][l]) + 3 + 4 * n_ini
        n = int(d["lcnt"][l])
        assert 0 <= n <= cap, f"{tag}: stage kept level {l}: count {n} beyond the level's {cap} slots (err {err})"
        rec = d["lvl"][base: base + n]
        got = np.stack([rec["x"], rec["y"], rec["srl"] & 0xFF], axis=1).astype(np.int64)
        want = okept[l][:, [0, 1, 4]].astype(np.int64)
        _multiset_diff(got, want, f"{tag}: stage kept level {l} (err {err})", "(x, y, score) in level pixels")
        xs = okept[l][:, 0] if l == 0 else okept[l][:, 0] * scales[l]
        onlap = int(np.count_nonzero((xs >= f32(lap[0])) & (xs <= f32(lap[1]))))
        glap = int(np.count_nonzero((rec["srl"] >> 8) & 1))
        assert glap == onlap and int(d["lnlap"][l]) == onlap, \
            f"{tag}: stage kept level {l}: lapping flags gpu {glap} / lvl_nlap {int(d['lnlap'][l])} oracle {onlap} (err {err})"
        base += cap
    assert base == int(d["sizes"][2]), f"{tag}: stage kept: level caps add up to {base}, kp_slots_total {int(d['sizes'][2])}"
    assert err == 0, f"{tag}: stage error word: {err}"
    return d
