"""Test-side model of the nested dissection's plan (csrc/ba_nd.h / ba_nd.hip), in plain Python.

It restates the rules the header and the kernel comments give, not the planner's code:

  * S is a (cyclic) block band of half-bandwidth w poses over np optimised poses, cut into K
    segments at seg[r] = floor(r np / K). Segment r = an interior followed by its own separator,
    the last w poses of the segment (the last segment of a line has none). Its matrix holds the
    interior (6 rows per pose, padded with identity rows to whole 32-row tiles), then the previous
    segment's separator (none for the first segment of a line), then its own.
  * A plan is refused when an interior is narrower than the band (two interiors would couple),
    when an interior is one tile or less, when a segment's matrix is longer than the tiles
    k_nd_backsolve's dynamic LDS holds (128 KiB: 84 tiles), or when the separator system (6 w
    rows per separator) is larger than the DAG solver's 4096.
  * The tile envelope rf[R] of a segment: the first tile column any row of tile row R couples
    to, under a pose adjacency (the full band of +-w poses by default, or the blocks of a given
    system); a padding row couples to itself only.
  * k_nd_backsolve runs four waves per segment. In phase 1 wave v takes the separator tile rows
    nti + v, + 4, ... of an interior column C that lie inside the envelope (rf[row] <= C); in
    phase 2 the interior rows C + 1 + v, + 4, ... below nti. The kernel keeps two tiles per wave
    and column in registers (kBsM) and loads the third and later ones inside the step, so the
    largest count a wave meets in a column tells which of its code paths a shape reaches:
    1 = the first register slot only, 2 = both slots, >= 3 = the in-step loads as well.
  * The second level: the K separators of a cyclic plan (K >= 6, a separator longer than one
    tile) form a cyclic chain of K // 2 segments of two separators each (the last takes a third
    when K is odd); the even separators are its interiors, the odd ones its separators.

tests/test_nd_model.py pins the figures of the shapes tests/test_nd_edges_gpu.py solves, so that
those tests cannot pass without reaching the paths they are there for."""
from __future__ import annotations

from dataclasses import dataclass, field

TILE = 32                    # rows of a tile (kDagTile)
WAVES = 4                    # waves of a k_nd_backsolve work-group
REG_TILES = 2                # tiles per wave and column held in registers (kBsM)
LDS_CAP = 128 * 1024         # dynamic LDS of k_nd_backsolve (kBsMaxLds)
SEP_MAX_ROWS = 4096          # the separator system runs on one DAG solve (kDagMaxN)
K_MAX = 32                   # the automatic plan tries K = 2 .. 32

REFUSED_NARROW = "an interior narrower than the band"
REFUSED_ONE_TILE = "an interior of one tile or less"
REFUSED_LDS = "a segment longer than the back-substitution's LDS"
REFUSED_SEPARATOR = "a separator system larger than the DAG solver's limit"


def tiles(rows: int) -> int:
    return -(-rows // TILE)


def bs_lds_bytes(nt: int) -> int:
    """k_nd_backsolve's dynamic LDS for segments of nt tiles: x, y (nt x 32 doubles each), the four
    waves' phase-1 partial sums (4 nt x 32), phase 2's partials (4 x 32) and one 32-vector, then nt
    ints of envelope."""
    return 8 * (2 * nt * TILE + WAVES * nt * TILE + WAVES * TILE + TILE) + 4 * nt


MAX_SEG_TILES = max(nt for nt in range(1, 200) if bs_lds_bytes(nt) <= LDS_CAP)


def bandwidth(n_pose: int, bi, bj) -> tuple:
    """nd_bandwidth's rule on pose blocks: (largest |j - i|, largest cyclic distance)."""
    wl = wc = 0
    for i, j in zip(bi, bj):
        d = abs(int(j) - int(i))
        wl = max(wl, d)
        wc = max(wc, min(d, n_pose - d))
    return wl, wc


def band_of(n_pose: int, bi, bj) -> tuple:
    """(w, cyclic) as the planner reads them off the blocks: a band that is narrower when distances
    wrap around is a loop."""
    wl, wc = bandwidth(n_pose, bi, bj)
    cyclic = wl > wc
    return max(1, wc if cyclic else wl), cyclic


def band_adjacency(n_pose: int, w: int, cyclic: bool) -> list:
    """Every pose coupled to the poses within w of it (itself included)."""
    adj = []
    for p in range(n_pose):
        if cyclic:
            adj.append(sorted({(p + d) % n_pose for d in range(-w, w + 1)}))
        else:
            adj.append(list(range(max(0, p - w), min(n_pose, p + w + 1))))
    return adj


def block_adjacency(n_pose: int, bi, bj) -> list:
    """The adjacency of a system's pose blocks (both directions, itself included)."""
    adj = [{p} for p in range(n_pose)]
    for i, j in zip(bi, bj):
        adj[int(i)].add(int(j))
        adj[int(j)].add(int(i))
    return [sorted(a) for a in adj]


@dataclass
class Segment:
    r: int
    interior: tuple          # poses [i0, i1)
    prev_sep: tuple | None   # poses of the previous segment's separator, or None
    own_sep: tuple | None    # poses of its own separator, or None
    padding: int             # identity rows after the interior (nip - ni)
    nti: int                 # interior tiles
    NT: int                  # tiles of the segment's matrix
    rows: int                # rows of the segment's matrix (n)

    @property
    def interior_poses(self) -> int:
        return self.interior[1] - self.interior[0]

    @property
    def nip(self) -> int:
        return TILE * self.nti


@dataclass
class Plan:
    n_pose: int
    K: int
    w: int
    cyclic: bool
    seg: list                # K + 1 segment starts
    segments: list = field(default_factory=list)
    refused: str | None = None

    @property
    def ok(self) -> bool:
        return self.refused is None

    @property
    def n_sep(self) -> int:
        return self.K if self.cyclic else self.K - 1

    @property
    def max_NT(self) -> int:
        return max(s.NT for s in self.segments)

    def separator_poses(self, t: int) -> tuple:
        return self.seg[t + 1] - self.w, self.seg[t + 1]


def _segments(seg: list, w: int, cyclic: bool) -> list:
    K = len(seg) - 1
    out = []
    for r in range(K):
        own = cyclic or r < K - 1
        prev = cyclic or r > 0
        i0, i1 = seg[r], seg[r + 1] - (w if own else 0)
        t = (r - 1) % K
        rows_i = 6 * (i1 - i0)
        nti = tiles(rows_i)
        rows = TILE * nti + 6 * w * (int(prev) + int(own))
        out.append(Segment(r, (i0, i1), (seg[t + 1] - w, seg[t + 1]) if prev else None,
                           (seg[r + 1] - w, seg[r + 1]) if own else None, TILE * nti - rows_i, nti, tiles(rows), rows))
    return out


def plan(n_pose: int, w: int, cyclic: bool, K: int) -> Plan:
    """The plan for a forced K >= 2, or the reason it is refused (first rule broken, segment by
    segment, then the separator system)."""
    seg = [r * n_pose // K for r in range(K + 1)]
    p = Plan(n_pose, K, w, cyclic, seg, _segments(seg, w, cyclic))
    for s in p.segments:
        if s.interior_poses < w:
            p.refused = REFUSED_NARROW
        elif 6 * s.interior_poses <= TILE:
            p.refused = REFUSED_ONE_TILE
        elif s.NT > MAX_SEG_TILES:
            p.refused = REFUSED_LDS
        if p.refused:
            return p
    if 6 * w * p.n_sep > SEP_MAX_ROWS:
        p.refused = REFUSED_SEPARATOR
    return p


def second_level(p: Plan) -> Plan | None:
    """The separator system's own dissection, or None when it is solved densely: the separators
    renumbered as poses t w .. t w + w - 1, inner segment r = separators 2r (its interior) and
    2r + 1 (its separator); with K odd the last one's interior is separators K - 3 and K - 2."""
    K, w = p.n_sep, p.w
    if not p.cyclic or K < 6 or 6 * w <= TILE:
        return None
    K2 = K // 2
    seg = [2 * r * w for r in range(K2)] + [K * w]
    q = Plan(K * w, K2, w, True, seg, _segments(seg, w, True))
    return q if q.max_NT <= MAX_SEG_TILES else None


def second_level_adjacency(p: Plan) -> list:
    """Couplings of the separator system: a separator with itself and (the fill of the interior
    between them) with the next one around the loop."""
    K, w = p.n_sep, p.w
    adj = []
    for t in range(K):
        near = [(t - 1) % K, t, (t + 1) % K]
        adj += [sorted(u * w + k for u in set(near) for k in range(w))] * w
    return adj


def modelled_chain(p: Plan, levels: int = 2) -> int:
    """The planner's cost of a plan: the longest interior + the separator system (dissected once
    more when that is shorter) + 3, in tile intervals."""
    sep = tiles(6 * p.w * p.n_sep)
    if p.cyclic and levels > 1 and p.n_sep >= 6 and 6 * p.w > TILE:
        sep = min(sep, tiles(6 * p.w * (2 if p.n_sep % 2 else 1)) + tiles(6 * p.w * (p.n_sep // 2)) + 3)
    return max(s.nti for s in p.segments) + sep + 3


def automatic_candidates(n_pose: int, w: int, cyclic: bool, k_cap: int = K_MAX) -> list:
    """Every plan the automatic choice (K = 0) considers: K = 2 .. min(32, k_cap, np / 2w) that is
    not refused (k_cap: half the device's resident work-groups)."""
    if n_pose < 8:
        return []
    ks = range(2, min(K_MAX, k_cap, n_pose // max(1, 2 * w)) + 1)
    return [q for q in (plan(n_pose, w, cyclic, k) for k in ks) if q.ok]


def automatic_plan(n_pose: int, w: int, cyclic: bool, levels: int = 2, k_cap: int = K_MAX) -> Plan | None:
    """The automatic choice: the candidate of the shortest modelled chain (the smallest K among
    equals), made only when that chain is at most 0.7 of the undissected solve's (tiles of S)."""
    best = None
    for q in automatic_candidates(n_pose, w, cyclic, k_cap):
        if best is None or modelled_chain(q, levels) < modelled_chain(best, levels):
            best = q
    if best is None or 10 * modelled_chain(best, levels) > 7 * tiles(6 * n_pose):
        return None
    return best


def local_rows(s: Segment) -> list:
    """S's row of every row of the segment's matrix (-1: padding): interior, previous separator,
    own separator."""
    rows = [6 * q + c for q in range(*s.interior) for c in range(6)] + [-1] * s.padding
    for z in (s.prev_sep, s.own_sep):
        if z is not None:
            rows += [6 * q + c for q in range(*z) for c in range(6)]
    assert len(rows) == s.rows
    return rows


def envelope(s: Segment, adj: list) -> list:
    """rf[R] for the NT tile rows of a segment under a pose adjacency."""
    rows = local_rows(s)
    first_row = {}
    for i, g in enumerate(rows):
        if g >= 0 and g % 6 == 0:
            first_row[g // 6] = i
    rf = []
    for R in range(s.NT):
        f = R
        for i in range(TILE * R, min(s.rows, TILE * R + TILE)):
            if rows[i] < 0:
                continue
            cols = [first_row[q] for q in adj[rows[i] // 6] if q in first_row]
            f = min(f, min(cols + [i]) // TILE)
        rf.append(f)
    return rf


def wave_maxima(s: Segment, rf: list) -> tuple:
    """(phase 1, phase 2): the most tiles one wave meets in one interior column."""
    p1 = p2 = 0
    for C in range(s.nti):
        for v in range(WAVES):
            p1 = max(p1, sum(1 for R in range(s.nti + v, s.NT, WAVES) if rf[R] <= C))
            p2 = max(p2, sum(1 for R in range(C + 1 + v, s.nti, WAVES) if rf[R] <= C))
    return p1, p2


def segment_figures(p: Plan, adj: list | None = None) -> list:
    """Per segment (interior poses, nti, NT, phase 1, phase 2, padding rows), under the full band's
    adjacency unless one is given."""
    if adj is None:
        adj = band_adjacency(p.n_pose, p.w, p.cyclic)
    out = []
    for s in p.segments:
        p1, p2 = wave_maxima(s, envelope(s, adj))
        out.append((s.interior_poses, s.nti, s.NT, p1, p2, s.padding))
    return out
