"""Crafted scenes for SearchForInitialization's routes and edges (tests/test_init_routes*.py), and a
Python restatement of the DEVICE formulation (csrc/init_kernels.hip), not of upstream's loop: ranks
in walk order, per-query candidate lists, their 16 smallest entries through the per-lane top-4
(with the `lost` rule), `need`, the fixed-point rounds with their per-rank claimants, the chain.

Every builder returns a dict: k1 / d1 / k2 / d2 / prev (the call's inputs), window, ratio, bounds,
and "plant" = what the scene was built to reach, worked out by hand in the builder's docstring:
need1 / need2 (queries with need == 1 / 2), full_scans (queries that scan their whole list in the
converged state), rounds (the index of the round that changes nothing; None where the rounds do not
end the search), max_claimants (the most claimants of one rank in one round) and form (0 the rounds
converge, 1 a rank has more claimants than claim slots, 2 the round cap). "expect" maps an F1 index
to the F2 index it must match (-1 none) where the scene plants it.

Construction, as in proj_cases.py: descriptors derive from one random base by flipping known bits,
so every distance is exact; with the default bounds a grid cell is 10 x 10 px; a keypoint meant to
be inside a window lies well inside it, one meant to be outside at least two radii away (the window
and grid scenes excepted: there the boundary is the point).
"""
import numpy as np

from helpers import c_round, rotation_bin, three_maxima
from orb_slam3_ros2_amd._lib import KP_DTYPE
from proj_cases import LATTICE, flip_low_bits

f32 = np.float32
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
INT_MAX = 2 ** 31 - 1
BOUNDS = (0.0, 640.0, 0.0, 480.0)
UNDISTORTED = (-14.5, 652.25, -11.75, 489.5)     # a negative minimum, as an undistorted frame has
K16, LANES, KEEP, SLOTS, MAX_ROUNDS, TH_LOW = 16, 64, 4, 8, 64, 50   # kInitK, wave, top-4, kInitC, kInitMaxRounds


def flip_bits(base, bits):
    """`base` with the listed bit positions flipped."""
    mask = np.zeros(256, np.uint8)
    mask[list(bits)] = 1
    return np.bitwise_xor(base, np.packbits(mask, bitorder="little"))


def kps(xy, octave=0, angle=0.0):
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0].astype(np.float32), xy[:, 1].astype(np.float32)
    k["octave"], k["angle"], k["size"], k["response"] = octave, angle, 31.0, 50.0
    return k


def scene(k1, d1, k2, d2, prev, window, ratio=0.9, bounds=BOUNDS, plant=None, expect=None, **extra):
    s = dict(k1=k1, d1=np.ascontiguousarray(d1, np.uint8).reshape(-1, 32), k2=k2,
             d2=np.ascontiguousarray(d2, np.uint8).reshape(-1, 32),
             prev=np.ascontiguousarray(prev, np.float32).reshape(-1, 2), window=window, ratio=ratio, bounds=bounds,
             plant=plant, expect=expect or {})
    s.update(extra)
    return s


# ---------------------------------------------------------------------------------------------
# the device formulation
# ---------------------------------------------------------------------------------------------

def accept(m1, m2, ratio):
    """d1 <= TH_LOW && (float)d1 < (float)d2 * nnratio on two list entries (None: no entry)."""
    if m1 is None:
        return False
    d1 = m1 >> 21
    d2 = INT_MAX if m2 is None else m2 >> 21
    return d1 <= TH_LOW and f32(d1) < f32(d2) * f32(ratio)


def model(s, ratio=None, ori=True):
    """The device formulation on scene `s`. Returns a dict: n / m12 / prev (the call's results, from
    the chain), rounds_m12 (the rounds' result where they converge: equal by assertion), need (per
    query), need1, need2, full_scans, rounds, max_claimants, form, nq0, nr0 (the ranked keypoints),
    host_nr0 (F2's octave-0 keypoints, on the grid or not: the host's count), lens, cap,
    overflow_round."""
    ratio = s["ratio"] if ratio is None else ratio
    k1, d1, k2, d2 = s["k1"], s["d1"], s["k2"], s["d2"]
    minx, maxx, miny, maxy = [f32(b) for b in s["bounds"]]
    invw, invh = f32(64) / (maxx - minx), f32(48) / (maxy - miny)
    r = f32(s["window"])
    # k_init_prep: ranks (cell, then index) of the octave-0 F2 keypoints on the grid; query slots
    cells = []
    for k in range(len(k2)):
        px, py = c_round(f32(k2["x"][k] - minx) * invw), c_round(f32(k2["y"][k] - miny) * invh)
        if k2["octave"][k] == 0 and 0 <= px < 64 and 0 <= py < 48:
            cells.append((px * 48 + py, k, px, py))
    cells.sort()
    slot = np.array([c[1] for c in cells], np.int64)
    RPX, RPY = np.array([c[2] for c in cells], np.int64), np.array([c[3] for c in cells], np.int64)
    RX, RY = k2["x"][slot].astype(np.float32), k2["y"][slot].astype(np.float32)
    qlist = [i for i in range(len(k1)) if k1["octave"][i] == 0]
    nq, nr = len(qlist), len(slot)
    # k_init_cands
    lists, topk, need = [], [], []
    for i1 in qlist:
        x, y = f32(s["prev"][i1, 0]), f32(s["prev"][i1, 1])
        x0, x1 = max(0, int(np.floor((x - minx - r) * invw))), min(63, int(np.ceil((x - minx + r) * invw)))
        y0, y1 = max(0, int(np.floor((y - miny - r) * invh))), min(47, int(np.ceil((y - miny + r) * invh)))
        keys = []
        if x0 < 64 and x1 >= 0 and y0 < 48 and y1 >= 0 and nr:
            ok = ((RPX >= x0) & (RPX <= x1) & (RPY >= y0) & (RPY <= y1) & (np.abs(RX - x) < r) & (np.abs(RY - y) < r))
            for rk in np.nonzero(ok)[0]:
                k = slot[rk]
                d = int(POP[np.bitwise_xor(d1[i1], d2[k])].sum())
                keys.append((d << 21) | (int(rk) << 5) | rotation_bin(k1["angle"][i1], k2["angle"][k]))
        # per-lane sorted top-4 (lane = rank mod 64), then 16 pops of the smallest lane head
        heads = {}
        for key in keys:
            heads.setdefault(((key >> 5) & 0xFFFF) % LANES, []).append(key)
        kept = sorted(key for lane in heads.values() for key in sorted(lane)[:KEEP])[:K16]
        popped = {}
        for key in kept:
            lane = ((key >> 5) & 0xFFFF) % LANES
            popped[lane] = popped.get(lane, 0) + 1
        lost = any(popped.get(lane, 0) == KEEP and len(v) > KEEP for lane, v in heads.items())
        lists.append(keys)
        topk.append(kept)
        need.append(2 if lost else (1 if len(keys) > K16 else 0))

    def select(q, md):
        """(m1, m2, scanned): the two smallest eligible entries as the chain and the rounds pick them."""
        elig = [key for key in topk[q] if (key >> 21) < md((key >> 5) & 0xFFFF)]
        full = need[q] == 2 or (need[q] == 1 and len(elig) < 2)
        if full:
            elig = sorted(key for key in lists[q] if (key >> 21) < md((key >> 5) & 0xFFFF))
        return (elig[0] if elig else None), (elig[1] if len(elig) > 1 else None), full

    # k_init_round: the fixed point
    cap = min(MAX_ROUNDS, nq + 2)
    picks = [None] * nq
    form, rounds, max_claimants, full_scans, overflow_round = 2, None, 0, 0, None
    for rnd in range(cap):
        claims = {}
        for j, p in enumerate(picks):
            if p is not None:
                claims.setdefault((p >> 5) & 0xFFFF, []).append((j, p >> 21))
        new, scans = [], 0
        for q in range(nq):
            m1, m2, full = select(q, lambda rk: min([d for j, d in claims.get(rk, []) if j < q], default=INT_MAX))
            scans += full
            new.append(m1 if accept(m1, m2, ratio) else None)
        count = {}
        for p in new:
            if p is not None:
                count[(p >> 5) & 0xFFFF] = count.get((p >> 5) & 0xFFFF, 0) + 1
        max_claimants = max([max_claimants] + list(count.values()))
        if max_claimants > SLOTS:
            form, overflow_round = 1, rnd
            break
        if new == picks:
            form, rounds, full_scans = 0, rnd, scans
            break
        picks = new

    def finish(pk):
        owner, hist = {}, [0] * 30
        for q, p in enumerate(pk):
            if p is not None:
                owner[(p >> 5) & 0xFFFF] = q      # the last claimant keeps the rank
                hist[p & 31] += 1                 # every push, stolen ones included
        keep = three_maxima(hist) if ori else None
        m12 = np.full(len(k1), -1, np.int32)
        for q, p in enumerate(pk):
            if p is not None and owner[(p >> 5) & 0xFFFF] == q and (not ori or (p & 31) in keep):
                m12[qlist[q]] = slot[(p >> 5) & 0xFFFF]
        return m12

    # k_init_greedy: the chain
    state, cl = {}, [None] * nq
    for q in range(nq):
        m1, m2, _ = select(q, lambda rk: state.get(rk, INT_MAX))
        if accept(m1, m2, ratio):
            cl[q] = m1
            state[(m1 >> 5) & 0xFFFF] = m1 >> 21
    m12 = finish(cl)
    out = dict(n=int((m12 >= 0).sum()), m12=m12, need=need, need1=need.count(1), need2=need.count(2),
               full_scans=full_scans, rounds=rounds, max_claimants=max_claimants, form=form, nq0=nq, nr0=nr,
               lens=[len(v) for v in lists], cap=cap, host_nr0=int((k2["octave"] == 0).sum()), overflow_round=overflow_round, rounds_m12=finish(picks) if form == 0 else None)
    prev = s["prev"].copy()
    hit = m12 >= 0
    prev[hit, 0], prev[hit, 1] = k2["x"][m12[hit]], k2["y"][m12[hit]]
    out["prev"] = prev
    return out


# ---------------------------------------------------------------------------------------------
# a, b: one crowded grid cell, rank == index
# ---------------------------------------------------------------------------------------------

CELL_CENTRE = (320.0, 240.0)      # cell (32, 24) covers [315, 325) x [235, 245)


def _one_cell(n):
    """n positions inside cell (32, 24), 1 px and more from its borders (pitch 0.4 px, 20 per row)."""
    assert n <= 400
    j = np.arange(n)
    return np.stack([316.0 + 0.4 * (j % 20), 236.0 + 0.4 * (j // 20)], 1)


def _cell_scene(flips, twins, pad, seed):
    """F2: keypoint j = the base B with its flips[j] lowest bits flipped, all in one cell (rank ==
    index). F1: an exact twin of every F2 index in `twins`, then `pad` octave-0 keypoints with no
    candidate, then Q = B; all at the cell's centre with window 10."""
    rng = np.random.default_rng(seed)
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    d2 = np.stack([flip_low_bits(B, f) for f in flips])
    k2 = kps(_one_cell(len(flips)), 0, 10.0)
    d1 = np.concatenate([d2[list(twins)].reshape(-1, 32), rng.integers(0, 256, (pad, 32), dtype=np.uint8), B[None]])
    xy = [CELL_CENTRE] * len(twins) + [(60.0 + 5 * i, 60.0) for i in range(pad)] + [CELL_CENTRE]
    k1 = kps(xy, 0, 40.0)
    return k1, d1, k2, d2, np.array(xy, np.float32), len(k1) - 1


def lost(lane=7, pad=0):
    """need == 2. F2 indices lane + 64 k (k = 0..5: ONE lane of k_init_cands) are 1..6 bits from Q,
    every other one 30..36. Twins of the first four come before Q and take them at distance 0, so Q's
    eligible set is {5, 6, 30...}: it matches lane + 256 (5 < 6 * 0.9). The lane keeps 4 of its 6
    entries and pops all 4 among the 16 smallest: `lost`, need = 2, for Q and for each twin (to a
    twin the lane's six are 0..5 away, the rest 26 and more). A kernel without `lost` holds {1, 2, 3,
    4, twelve of 30...} for Q, finds 12 eligible and no match (30 against 30). Rounds: round 0 Q
    takes `lane` (1 against 2) beside its twin (2 claimants), round 1 it moves, round 2 is still.
    `pad` unmatched queries move Q through the four slots of its block."""
    n2 = lane + 5 * 64 + 3
    close = [lane + 64 * k for k in range(6)]
    flips = [30 + j % 7 for j in range(n2)]
    for k, j in enumerate(close):
        flips[j] = k + 1
    k1, d1, k2, d2, prev, Q = _cell_scene(flips, close[:4], pad, 300 + lane)
    expect = {i: close[i] for i in range(4)}
    expect[Q] = close[4]
    return scene(k1, d1, k2, d2, prev, 10, expect=expect, Q=Q, q_slot=(4 + pad) % 4,
                 plant=dict(need1=0, need2=5, full_scans=5, rounds=2, max_claimants=2, form=0))


def few_eligible(mode, n2=65):
    """need == 1 with fewer than two eligible entries among the 16 smallest. F2 indices 1..16 (16
    lanes, so nothing is lost) are 1..16 bits from Q and belong to twins that come first; every
    list holds all n2 > 16 keypoints, so need = 1 for every query.
    "pair": Q has no eligible entry among its 16 and scans: 17 bits at index n2 - 1 (the last,
    partly filled 64-stride of the list) against 20 at n2 - 2: a match (17 < 18). The twins keep
    two and more eligible (their own, a later twin's, the pair): full_scans = 1.
    With n2 = 65 / 129 only the best lies in the last stride, with 66 / 130 both.
    "one": 15 twins; index 16 (16 bits) stays eligible, alone among the 16, and the scan brings 17
    bits at n2 - 1 as second best: 16 < 15.3 fails, no match (a kernel that took the second best
    from the 16 alone would see INT_MAX and match).
    "zero": 18 keypoints 1..18 bits from Q, 18 twins: nothing is eligible anywhere, no match; the
    last twin has only its own keypoint eligible among its 16 and scans too (full_scans = 2).
    Rounds: round 0 Q takes index 1 (1 against 2) beside its twin, round 1 it moves, round 2 is still."""
    if mode == "zero":
        n2 = 18
        flips = list(range(1, 19))
        twins, want, scans = list(range(18)), -1, 2
    else:
        flips = [30 + j % 7 for j in range(n2)]
        for j in range(1, 17):
            flips[j] = j
        flips[n2 - 1] = 17
        if mode == "one":
            twins, want, scans = list(range(1, 16)), -1, 1
        else:
            flips[n2 - 2] = 20
            twins, want, scans = list(range(1, 17)), n2 - 1, 1
    k1, d1, k2, d2, prev, Q = _cell_scene(flips, twins, 0, 400 + n2 + len(mode))
    expect = {i: t for i, t in enumerate(twins)}
    expect[Q] = want
    return scene(k1, d1, k2, d2, prev, 10, expect=expect, Q=Q,
                 plant=dict(need1=len(twins) + 1, need2=0, full_scans=scans, rounds=2, max_claimants=2, form=0))


# ---------------------------------------------------------------------------------------------
# c: the dependency chain
# ---------------------------------------------------------------------------------------------

def chain(N):
    """F2 keypoints k_0..k_N on one row 7 px apart (window 5), k_i = B with bit i flipped; query q_i
    midway between k_i and k_i+1 with k_i+1's descriptor and 20 neutral bits flipped: 20 from
    k_i+1, 22 from k_i. k_0 lies outside q_0's window, so q_0 matches k_1 (one candidate). While
    k_i is eligible q_i is rejected (20 < 22 * 0.9 fails); once q_i-1 holds k_i at 20 it is not (22
    >= 20) and q_i matches k_i+1. Round r of the fixed point sets q_r right: round N is the first
    that changes nothing, within the cap of min(64, N + 2) rounds only for N <= 63."""
    rng = np.random.default_rng(500 + N)
    B = rng.integers(0, 256, 32, dtype=np.uint8)
    xy2 = np.array([(20.0 + 7.0 * i, 242.0) for i in range(N + 1)])
    xy2[0] = (20.0, 400.0)
    k2 = kps(xy2, 0, 10.0)
    d2 = np.stack([flip_bits(B, [i]) for i in range(N + 1)])
    xy1 = np.array([(23.5 + 7.0 * i, 242.0) for i in range(N)])
    d1 = np.stack([flip_bits(d2[i + 1], range(128, 148)) for i in range(N)])
    return scene(kps(xy1, 0, 40.0), d1, k2, d2, xy1, 5, expect={i: i + 1 for i in range(N)},
                 plant=dict(need1=0, need2=0, full_scans=0, rounds=N if N <= 63 else None, max_claimants=1,
                            form=0 if N <= 63 else 2))


CHAIN_N = (5, 15, 17, 62, 63, 64, 70)


# ---------------------------------------------------------------------------------------------
# d: claim slots
# ---------------------------------------------------------------------------------------------

def claimants(C, steal):
    """C queries around one F2 keypoint. Equal distances (4): round 0 puts all C on the rank, in
    round 1 only the first stays, round 2 is still; the first keeps the match. Strictly decreasing
    distances (30 - i): every query steals from the one before, the picks of round 0 stand (round 1
    is still) and the last keeps the match. C <= 8 fits the claim slots, 9 and more overflow."""
    B = np.zeros(32, np.uint8) + 0x5A
    k2 = kps([(300.0, 200.0)], 0, 0.0)
    k1 = kps([(303.0, 203.0)] * C, 0, np.linspace(0, 40, C, dtype=np.float32))
    d1 = np.stack([flip_low_bits(B, 30 - i if steal else 4) for i in range(C)])
    prev = np.stack([k1["x"], k1["y"]], 1)
    expect = {i: -1 for i in range(C)}
    expect[C - 1 if steal else 0] = 0
    return scene(k1, d1, k2, B[None], prev, 10, expect=expect,
                 plant=dict(need1=0, need2=0, full_scans=0, rounds=(1 if steal else 2) if C <= SLOTS else None,
                            max_claimants=C, form=0 if C <= SLOTS else 1))


CLAIMANTS = (7, 8, 9, 16)


# ---------------------------------------------------------------------------------------------
# e: size edges
# ---------------------------------------------------------------------------------------------

SIZES_Q = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65)
SIZES_R = (1, 15, 16, 17, 63, 64, 65, 129)


def sized(nq0, nr0):
    """nq0 octave-0 queries against nr0 ranked F2 keypoints in a 200 x 150 px region (window 40: the
    lists of the larger cases pass 16 entries). Three in four queries derive from an F2 keypoint
    (moved a few px, 0..30 bits flipped; several of one keypoint where nq0 > nr0: steals), the others
    lie in an empty corner and have no candidate. Keypoints of octave > 0 are interleaved in both frames (slot
    != index, rank != index), F2 has two octave-0 keypoints off the grid, and F2 is shuffled."""
    rng = np.random.default_rng(1000 * nq0 + nr0)
    B = rng.integers(0, 256, (nr0, 32), dtype=np.uint8)
    xy2 = np.stack([rng.uniform(220.0, 420.0, nr0), rng.uniform(160.0, 310.0, nr0)], 1)
    ang2 = rng.choice([10.0, 10.0, 10.0, 100.0], nr0)
    rows1, rows2 = [], [(xy2[j], 0, ang2[j], B[j]) for j in range(nr0)]
    for j in range(nr0 // 3 + 1):      # other octaves, off-grid keypoints
        rows2.append((xy2[j % nr0] + 1.0, 1 + j % 3, 10.0, B[j % nr0]))
    rows2.append((np.array([700.0, 240.0]), 0, 10.0, B[0]))
    rows2.append((np.array([300.0, -40.0]), 0, 10.0, B[0]))
    for i in range(nq0):
        if i % 4 == 3:
            rows1.append((np.array([20.0 + 3.0 * (i % 50), 440.0]), 0, 40.0, rng.integers(0, 256, 32, dtype=np.uint8)))
        else:
            j = int(rng.integers(0, nr0)) if i % 5 else (i // 5) % nr0
            bits = rng.permutation(256)[: int(rng.integers(0, 31))]
            rows1.append((xy2[j] + rng.normal(size=2) * 3.0, 0, 40.0, flip_bits(B[j], bits)))
        if i % 2 == 0:
            rows1.append((rows1[-1][0], 2, 40.0, rows1[-1][3]))
    perm = rng.permutation(len(rows2))
    rows2 = [rows2[p] for p in perm]

    def pack(rows):
        k = kps(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], np.float32))
        return k, np.stack([r[3] for r in rows])
    k1, d1 = pack(rows1)
    k2, d2 = pack(rows2)
    return scene(k1, d1, k2, d2, np.stack([k1["x"], k1["y"]], 1), 40, sizes=(nq0, nr0))


# ---------------------------------------------------------------------------------------------
# f: gate boundaries
# ---------------------------------------------------------------------------------------------

# (best, second) distances of one query each; None: a single candidate (bestDist2 = INT_MAX);
# "=": two candidates at the same distance (other bits): the lower rank is best, the ratio test fails
GATES = [(50, None), (51, None), (9, 10), (18, 20), (45, 50), (27, 30), (7, 10), (14, 20), (35, 50), (6, 10),
         (12, "=")]
GATE_RATIOS = (0.9, 0.7, 0.6)


def gate_expect(ratio):
    """Whether each query of GATES matches: the reference's test in float."""
    out = []
    for d1, d2 in GATES:
        d2 = INT_MAX if d2 is None else (d1 if d2 == "=" else d2)
        out.append(bool(d1 <= TH_LOW and f32(d1) < f32(d2) * f32(ratio)))
    return out


def gates():
    """One query per entry of GATES on the lattice (window 10, its candidates 2 px away)."""
    rng = np.random.default_rng(600)
    xy1, d1, xy2, d2 = [], [], [], []
    for (a, b), P in zip(GATES, LATTICE):
        Bq = rng.integers(0, 256, 32, dtype=np.uint8)
        xy1.append(P); d1.append(Bq)
        xy2.append((P[0] + 2.0, P[1])); d2.append(flip_low_bits(Bq, a))
        if b is not None:
            xy2.append((P[0], P[1] + 2.0))
            d2.append(flip_bits(Bq, range(100, 100 + a)) if b == "=" else flip_low_bits(Bq, b))
    return scene(kps(xy1, 0, 40.0), d1, kps(xy2, 0, 10.0), d2, np.array(xy1, np.float32), 10,
                 plant=dict(need1=0, need2=0, full_scans=0, rounds=1, max_claimants=1, form=0))


# ---------------------------------------------------------------------------------------------
# g: window and grid
# ---------------------------------------------------------------------------------------------

def _coord(minv, inv, c):
    """A float coordinate near grid position c (in cells)."""
    return f32(f32(minv) + f32(c) / inv)


def half_coord(minv, inv, k0):
    """(k, x): the first even k >= k0 with a float x where (x - minv) * inv == k + 0.5 exactly in
    float (roundf takes it to k + 1; not every k has one under every bounds)."""
    for k in range(k0, k0 + 8, 2):
        x = _coord(minv, inv, k + 0.5)
        for step in (f32(np.inf), f32(-np.inf)):
            cand = x
            for _ in range(64):
                if f32(cand - f32(minv)) * inv == f32(k + 0.5):
                    return k, f32(cand)
                cand = np.nextafter(cand, step)
    raise AssertionError("no float lands on a half cell")


def _below_half(minv, inv, k, h):
    """The largest float below h whose grid position is below k + 0.5 (several floats may share h's)."""
    x = np.nextafter(h, f32(-np.inf))
    while f32(x - f32(minv)) * inv >= f32(k + 0.5):
        x = np.nextafter(x, f32(-np.inf))
    return f32(x)


def window_grid(bounds=BOUNDS):
    """One query per case with one candidate 5 bits away (window 10); "expect" says which match.
    The strict window test: the candidate at exactly prev +- r (outside) and one float inside, in x
    and in y. The grid: a candidate in the window whose cell is 64 / 48 / -1 (off the grid, never a
    candidate) beside one in cell 63 / 47 / 0, on each side, under queries whose windows lie partly
    off the grid; four queries whose windows lie wholly off it."""
    minx, maxx, miny, maxy = [f32(b) for b in bounds]
    invw, invh = f32(64) / (maxx - minx), f32(48) / (maxy - miny)
    rng = np.random.default_rng(700)
    r = f32(10)
    cases = []                         # (prev, candidate or None, matches)
    P = [(f32(a), f32(b)) for a, b in LATTICE[:8]]
    up, down = f32(np.inf), f32(-np.inf)
    cases += [(P[0], (P[0][0] + r, P[0][1]), False), (P[1], (np.nextafter(P[1][0] + r, down), P[1][1]), True),
              (P[2], (P[2][0] - r, P[2][1]), False), (P[3], (np.nextafter(P[3][0] - r, up), P[3][1]), True),
              (P[4], (P[4][0], P[4][1] + r), False), (P[5], (P[5][0], np.nextafter(P[5][1] + r, down)), True),
              (P[6], (P[6][0], P[6][1] - r), False), (P[7], (P[7][0], np.nextafter(P[7][1] - r, up)), True)]
    X = lambda c: _coord(minx, invw, c)     # noqa: E731
    Y = lambda c: _coord(miny, invh, c)     # noqa: E731
    cases += [((X(63.2), Y(10.0)), (X(63.6), Y(10.0)), False), ((X(63.2), Y(20.0)), (X(63.4), Y(20.0)), True),
              ((X(30.0), Y(47.2)), (X(30.0), Y(47.6)), False), ((X(40.0), Y(47.2)), (X(40.0), Y(47.4)), True),
              ((X(0.3), Y(30.0)), (X(-0.6), Y(30.0)), False), ((X(0.3), Y(35.0)), (X(-0.4), Y(35.0)), True),
              ((X(20.0), Y(0.3)), (X(20.0), Y(-0.6)), False), ((X(25.0), Y(0.3)), (X(25.0), Y(-0.4)), True),
              ((X(-3.0), Y(24.0)), None, False), ((X(67.0), Y(24.0)), None, False),
              ((X(32.0), Y(-3.0)), None, False), ((X(32.0), Y(51.0)), None, False)]
    xy1, d1, xy2, d2, expect = [], [], [], [], {}
    for i, (p, c, hit) in enumerate(cases):
        Bq = rng.integers(0, 256, 32, dtype=np.uint8)
        xy1.append(p); d1.append(Bq)
        if c is not None:
            expect[i] = len(xy2) if hit else -1
            xy2.append(c); d2.append(flip_low_bits(Bq, 5))
        else:
            expect[i] = -1
    k2 = kps(xy2, 0, 10.0)
    k2["x"], k2["y"] = np.array([c[0] for c in xy2], np.float32), np.array([c[1] for c in xy2], np.float32)
    k1 = kps(xy1, 0, 40.0)
    prev = np.array(xy1, np.float32)
    return scene(k1, d1, k2, d2, prev, 10, bounds=bounds, expect=expect,
                 plant=dict(need1=0, need2=0, full_scans=0, rounds=1, max_claimants=1, form=0))


def half_cells(bounds=BOUNDS):
    """roundf at k + 0.5 through the walk order. With nnratio 1.5 two candidates at one distance pass
    the ratio test and the first in walk order (cell, then index) is the match. Per case: keypoint
    L (the lower index) at a coordinate h where (h - min) * inv is k + 0.5 exactly, k even, keypoint
    H (the higher index) 1 px below h in cell k. roundf takes h to cell k + 1, so H comes first and
    matches (rounding to even, or down, would put both in cell k and match L). Beside it the same
    pair with L at the last float below the half: both in cell k, L matches. In x and in y."""
    minx, maxx, miny, maxy = [f32(b) for b in bounds]
    invw, invh = f32(64) / (maxx - minx), f32(48) / (maxy - miny)
    rng = np.random.default_rng(800)
    xy1, d1, xy2, d2, expect = [], [], [], [], {}
    for i, (axis, exact) in enumerate([(0, True), (0, False), (1, True), (1, False)]):
        if axis == 0:
            k, h = half_coord(minx, invw, 4 + 8 * i)
            other = _coord(miny, invh, 10.0 + 6 * i)
            L = (h if exact else _below_half(minx, invw, k, h), other)
            H = (h - f32(1), other)
            q = (h - f32(2), other)
        else:
            k, h = half_coord(miny, invh, 4 + 8 * i)
            other = _coord(minx, invw, 10.0 + 6 * i)
            L = (other, h if exact else _below_half(miny, invh, k, h))
            H = (other, h - f32(1))
            q = (other, h - f32(2))
        Bq = rng.integers(0, 256, 32, dtype=np.uint8)
        xy1.append(q); d1.append(Bq)
        expect[i] = len(xy2) + (1 if exact else 0)
        xy2 += [L, H]
        d2 += [flip_low_bits(Bq, 5), flip_bits(Bq, range(100, 105))]
    k2 = kps(xy2, 0, 10.0)
    k2["x"], k2["y"] = np.array([c[0] for c in xy2], np.float32), np.array([c[1] for c in xy2], np.float32)
    return scene(kps(xy1, 0, 40.0), d1, k2, d2, np.array(xy1, np.float32), 10, ratio=1.5, bounds=bounds, expect=expect,
                 plant=dict(need1=0, need2=0, full_scans=0, rounds=1, max_claimants=1, form=0))


# ---------------------------------------------------------------------------------------------
# every crafted scene by name (the size edges and the envelope have their own tests)
# ---------------------------------------------------------------------------------------------

CRAFTED = {}
# The lanes: the whole-list scans reduce lanes (the chain: 64, entry e in lane e mod 64; the rounds:
# 16, entry e in lane e mod 16) by a butterfly of xor 1, xor 2, half-row mirror, row mirror, rows
# 0 <-> 1 / 2 <-> 3 and halves, read in lane 0. A lane's entries reach lane 0 only through the steps
# that lane needs: 3 needs xor 1 and xor 2, 9 the two mirrors, 20 the row swap, 40 the half swap.
for _lane, _pad in [(7, 0), (7, 1), (7, 2), (7, 3), (0, 0), (63, 0), (3, 0), (9, 0), (20, 0), (40, 0)]:
    CRAFTED[f"lost-lane{_lane}-pad{_pad}"] = (lost, (_lane, _pad))
for _mode, _n2 in [("pair", 65), ("pair", 129), ("pair", 66), ("pair", 130), ("one", 65), ("zero", 18)]:
    CRAFTED[f"few-{_mode}-{_n2}"] = (few_eligible, (_mode, _n2))
for _N in CHAIN_N:
    CRAFTED[f"chain-{_N}"] = (chain, (_N,))
for _C in CLAIMANTS:
    CRAFTED[f"claim-equal-{_C}"] = (claimants, (_C, False))
    CRAFTED[f"claim-steal-{_C}"] = (claimants, (_C, True))
CRAFTED["gates"] = (gates, ())
CRAFTED["window"] = (window_grid, ())
CRAFTED["window-undistorted"] = (window_grid, (UNDISTORTED,))
CRAFTED["halves"] = (half_cells, ())
CRAFTED["halves-undistorted"] = (half_cells, (UNDISTORTED,))

_cache = {}


def ahead_after(ahead, m):
    """ws->init_ahead after a call in the default form whose rounds go as the model `m` says, from
    its value before: rounds are launched `ahead` at a time; a batch that does not end the search
    doubles it (16 at most), the round r that changes nothing sets clamp(r + 2, 3, 16), an overflow
    leaves it."""
    r = 0
    while r < m["cap"]:
        R = min(ahead, m["cap"] - r)
        if m["overflow_round"] is not None and m["overflow_round"] < r + R:
            return ahead
        if m["rounds"] is not None and m["rounds"] < r + R:
            return min(16, max(3, m["rounds"] + 2))
        r += R
        ahead = min(16, 2 * ahead)
    return ahead


def crafted(name):
    """The scene of that name, built once."""
    if name not in _cache:
        fn, args = CRAFTED[name]
        _cache[name] = fn(*args)
    return _cache[name]
