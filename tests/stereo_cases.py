"""Planted scenes for ComputeStereoMatches' structural edges (tests/test_stereo_cases*.py): the
64-lane candidate search and its butterfly, the Hamming thresholds, the window / octave / row gates,
the guard and iniu / endu on scaled levels, the acceptance tail, and k_stereo_median's two-pass
byte-radix select.

MATCH maps a scene name to its builder; `match_scene(oracle, name)` returns the dict that
stereo_numpy.parity_scene returns (left, right, kps_l, desc_l, kps_r, desc_r, pyr_l, pyr_r, scale,
inv_scale, bf, b) plus "labels" (one per left keypoint) and "plant": the figures the scene was built
to reach, per left keypoint, None where nothing is planted:
  best_r, best_dist, n_tied   the search's winner, its distance, the candidates that share it
  scaled                      (scaleduL, scaledvL, scaleduR0), None entries free
  status, inc, sad, sub       one list, or {0: list, 1: list} by center_patch; status SAD_FORMED
                              stands for "a SAD was formed" (1, 5, 7 or 8), PAST_SEARCH for
                              "neither 2 nor 3"
  u_right                     the accepted value (bit pattern), where the construction fixes it
MEDIAN maps a name to the inputs of orbhip_test_stereo_median (status, sad, u_right, depth) plus
"plant": median (the SAD of rank size / 2), n_accepted, cut_sads / kept_sads (SAD values that must /
must not be cut) and rank_edge ("last" / "first": the rank is the last v / the first v + 1 of a
two-valued set).

Construction: all images are 320 x 240, the extractor's eight levels. Descriptors derive from one
random 256-bit word by flipping an exact number of bits, so every distance is known. Search scenes
use one left keypoint at (200, 120), octave 0, with bf / b = 40: candidates lie at x in [170, 195],
fillers share the row band but lie left of minU = 160 and carry descriptors 0..5 bits from the left
one (a broken x gate makes them win). Patch scenes paint noise-free images: TEX is a random texture
whose right image is the left one moved 10 px (true disparity 10) plus g(y) = y * y % 7 on every
row, so the best SAD is small, positive and depends on the row; PAINT holds bars, columns and flat
blocks on a constant ground.
"""
import numpy as np

from init_cases import flip_bits
from orb_slam3_ros2_amd._lib import KP_DTYPE

import stereo_numpy as S

f32 = np.float32
WIDTH, HEIGHT = 320, 240
W, L = S.W, S.L
SAD_FORMED, PAST_SEARCH = 0, -1
UP, DOWN = f32(np.inf), f32(-np.inf)
UL, VL = 200.0, 120.0            # the search scenes' left keypoint (bf / b = 40: the window is [160, 200])
_LOW = np.stack([np.packbits(np.arange(256) < k, bitorder="little") for k in range(257)])   # k lowest bits set


def upstream_median_loop(sads, accepted):
    """Upstream's own cut: sort (SAD, iL), take sorted[size / 2].first, walk back from the end until
    the first SAD below thDist. -> the indices cut."""
    v = sorted((int(sads[i]), int(i)) for i in accepted)
    if not v:
        return []
    th = f32(f32(1.5) * f32(1.4)) * f32(v[len(v) // 2][0])
    cut = []
    for k in range(len(v) - 1, -1, -1):
        if f32(v[k][0]) < th:
            break
        cut.append(v[k][1])
    return cut


# ---------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------

def g_row(y):
    return (np.asarray(y, np.int64) ** 2) % 7


def _tex():
    left = np.random.default_rng(77).integers(30, 221, (HEIGHT, WIDTH)).astype(np.uint8)
    right = left[:, np.minimum(np.arange(WIDTH) + 10, WIDTH - 1)] + g_row(np.arange(HEIGHT))[:, None].astype(np.uint8)
    return left, np.ascontiguousarray(right)


def _same():
    left = np.random.default_rng(78).integers(0, 256, (HEIGHT, WIDTH)).astype(np.uint8)
    return left, left.copy()


def _paint():
    """Ground 60 (the right image + g(y) above row 140). Rows 22..128: 3-px bars (200) for the
    disparity cases; rows 142..183: 1-px columns for the equal-SAD cases; rows 205..225: flat blocks
    0 / 255 and the centred maximum."""
    left = np.full((HEIGHT, WIDTH), 60, np.uint8)
    right = left.copy()
    right[:140] += g_row(np.arange(140))[:, None].astype(np.uint8)

    def bar(img, v, c, half=1, val=200):
        img[v - 8: v + 9, c - half: c + half + 1] = val + (g_row(np.arange(v - 8, v + 9))[:, None] if img is right and v < 140 else 0)
    for v, cr in ((30, 150), (60, 111), (90, 110), (120, 150)):
        bar(left, v, 150)
        bar(right, v, cr)
    right[112: 129, 152] = 130 + g_row(np.arange(112, 129))     # the asymmetric one: d1 > d3
    bar(left, 150, 150, 0); bar(right, 150, 138, 0); bar(right, 150, 142, 0)     # minima at -2 and +2
    bar(left, 175, 150, 0); bar(right, 175, 135, 0); bar(right, 175, 141, 0)     # minima at -5 and +1
    left[205: 226, 100: 201] = 0
    right[205: 226, 100: 201] = 255
    left[205: 226, 220: 311] = 0
    left[215, 270] = 255
    right[205: 226, 220: 311] = 255
    right[215, 220: 311] = 0
    return left, right


_IMAGES = {"tex": _tex, "same": _same, "paint": _paint}
_img_cache = {}


def images(oracle, kind):
    """(left, right, pyr_l, pyr_r) of one image pair, built once."""
    if kind not in _img_cache:
        left, right = _IMAGES[kind]()
        o = S.ORB
        _img_cache[kind] = (left, right, oracle.pyramid(left, o["scale_factor"], o["nlevels"]),
                            oracle.pyramid(right, o["scale_factor"], o["nlevels"]))
    return _img_cache[kind]


# ---------------------------------------------------------------------------------------------
# the scene builder
# ---------------------------------------------------------------------------------------------

def kps(x, y, octave):
    x = np.atleast_1d(np.asarray(x, f32))
    k = np.zeros(len(x), KP_DTYPE)
    k["x"], k["y"], k["octave"], k["size"], k["angle"], k["response"] = x, np.asarray(y, f32), octave, 31.0, 0.0, 50.0
    return k


def flipped(base, k, rng):
    """`base` with exactly k bits flipped, at random positions."""
    return flip_bits(base, rng.permutation(256)[:k])


PLANT_KEYS = ("best_r", "best_dist", "n_tied", "scaled", "status", "inc", "sad", "sub", "u_right")


class Scene:
    def __init__(self, oracle, kind, bf=40.0, b=1.0, seed=0):
        self.oracle, self.kind, self.bf, self.b = oracle, kind, bf, b
        self.rng = np.random.default_rng(seed)
        self.kl, self.dl, self.kr, self.dr, self.labels = [], [], [], [], []
        self.plant = {k: [] for k in PLANT_KEYS}
        self.nr = 0

    def word(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def left(self, x, y, octave, desc, label="", **plant):
        assert set(plant) <= set(PLANT_KEYS), plant
        self.kl.append(kps(x, y, octave))
        self.dl.append(np.asarray(desc, np.uint8).reshape(1, 32))
        self.labels.append(label)
        for k in PLANT_KEYS:
            self.plant[k].append(plant.get(k))
        return len(self.kl) - 1

    def right(self, x, y, octave, desc):
        """One right keypoint or an array of them; -> the index of the first."""
        k = kps(x, y, octave)
        self.kr.append(k)
        self.dr.append(np.asarray(desc, np.uint8).reshape(len(k), 32))
        self.nr += len(k)
        return self.nr - len(k)

    def pair(self, xl, xr, y, octave=0, label="", yr=None, octave_r=None, **plant):
        """A left and a right keypoint with one random descriptor; best_r is planted as the right one."""
        d = self.word()
        ir = self.right(xr, y if yr is None else yr, octave if octave_r is None else octave_r, d)
        plant.setdefault("best_r", ir)
        return self.left(xl, y, octave, d, label, **plant)

    def done(self):
        left, right, pl, pr = images(self.oracle, self.kind)
        cat = lambda v, empty: np.concatenate(v) if v else empty     # noqa: E731
        s = dict(left=left, right=right, pyr_l=pl, pyr_r=pr, bf=self.bf, b=self.b, labels=self.labels, plant=self.plant,
                 kps_l=cat(self.kl, np.zeros(0, KP_DTYPE)), desc_l=cat(self.dl, np.zeros((0, 32), np.uint8)),
                 kps_r=cat(self.kr, np.zeros(0, KP_DTYPE)), desc_r=cat(self.dr, np.zeros((0, 32), np.uint8)))
        s["scale"], s["inv_scale"] = S.scale_tables(self.oracle, WIDTH, HEIGHT)
        return s


# ---------------------------------------------------------------------------------------------
# search scenes
# ---------------------------------------------------------------------------------------------

def search(oracle, n_r, cands, others=True, seed=1):
    """One left keypoint at (UL, VL) against n_r right keypoints in its row band. `cands` maps iR to
    a distance; with `others`, every third remaining index is a candidate at least 10 bits worse
    than the best; every other index is a filler left of minU, 0..5 bits away."""
    s = Scene(oracle, "tex", seed=seed)
    base = s.word()
    i = np.arange(n_r)
    best = min(cands.values())
    x = (20 + i % 130).astype(f32)
    y = (VL - 1 + i % 3).astype(f32)
    desc = np.bitwise_xor(base[None], _LOW[i % 6])
    if others:
        oth = i % 3 == 1
        x[oth] = (170 + i % 25)[oth]
        desc[oth] = np.bitwise_xor(base[None], _LOW[np.minimum(best + 10 + i % 60, 140)])[oth]
    for c, d in cands.items():
        x[c], y[c] = 170 + c % 25, VL
        desc[c] = flipped(base, d, s.rng)
    s.right(x, y, 0, desc)
    win = min(c for c, d in cands.items() if d == best)
    hit = best < S.TH_HIGH
    s.left(UL, VL, 0, base, f"n_r {n_r}", best_r=win if hit else -1, best_dist=best if hit else S.TH_HIGH,
           n_tied=sum(d == best for d in cands.values()) if hit else 0,
           status=PAST_SEARCH if best < S.TH_ORB_DIST else 3)
    return s.done()


def nl_scene(oracle, n_l):
    """n_l left keypoints (work-groups of four waves, full and partial); only the last has a match,
    the others lie on rows without a right keypoint."""
    s = Scene(oracle, "tex", seed=40 + n_l)
    for k in range(n_l - 1):
        s.left(UL, 20.0 + 12 * k, 0, s.word(), "empty row", best_r=-1, status=2)
    s.pair(UL, 185.0, VL, label="the last", best_dist=0, n_tied=1, status=PAST_SEARCH)
    return s.done()


def window(oracle, exact):
    """xR at minU, one float below it, at maxU = uL and one float above it. exact: bf / b = 40 and
    uL = 200, every operation exact; else bf / b = 40.3 / 1.1 and uL = 200.7, where the division and
    the subtraction both round. One keypoint more with minU < 0 (uL = 12.5, xR = 0)."""
    bf, b, ul = (40.0, 1.0, f32(200.0)) if exact else (40.3, 1.1, f32(200.7))
    max_d = f32(bf) / f32(b)
    min_u = f32(ul - max_d)
    assert (np.float64(ul) - np.float64(f32(bf)) / np.float64(f32(b)) == np.float64(min_u)) == exact
    s = Scene(oracle, "tex", bf, b, seed=50 + exact)
    for row, (xr, hit, label) in zip((30, 70, 110, 150), ((min_u, True, "xR == minU"),
                                                          (np.nextafter(min_u, DOWN), False, "xR one float below minU"),
                                                          (ul, True, "xR == maxU"),
                                                          (np.nextafter(ul, UP), False, "xR one float above maxU"))):
        i = s.pair(ul, xr, float(row), label=label, status=PAST_SEARCH if hit else 3)
        if not hit:
            s.plant["best_r"][i] = -1
    if exact:
        s.pair(12.5, 0.0, 190.0, label="minU < 0", status=9)     # the right centre is at column 0
    return s.done()


def octave(oracle, oct_l):
    """Right octaves octL - 2 .. octL + 2 (those inside [0, 8)), one per left keypoint and row."""
    s = Scene(oracle, "tex", seed=60 + oct_l)
    for k, o in enumerate(range(oct_l - 2, oct_l + 3)):
        if 0 <= o < 8:
            ok = abs(o - oct_l) <= 1
            i = s.pair(UL, 190.0, 30.0 + 40 * k, oct_l, f"right octave {o}", octave_r=o, status=PAST_SEARCH if ok else 3)
            if not ok:
                s.plant["best_r"][i] = -1
    return s.done()


def row_band(oracle, oct_r, y_r):
    """One right keypoint; left rows at lo - 1, lo, hi, hi + 1 (vL = row + 0.25) and at
    hi + 0.999 (row hi: inside) and lo - 1 + 0.999 (row lo - 1: outside)."""
    s = Scene(oracle, "tex", seed=70 + oct_r)
    scale, _ = S.scale_tables(oracle, WIDTH, HEIGHT)
    r = f32(2) * scale[oct_r]
    lo, hi = int(np.floor(f32(y_r) - r)), int(np.ceil(f32(y_r) + r))
    assert 0 < lo and hi < HEIGHT - 1
    d = s.word()
    s.right(190.0, y_r, oct_r, d)
    for v, hit, label in ((lo - 1 + 0.25, False, "lo - 1"), (lo + 0.25, True, "lo"), (hi + 0.25, True, "hi"),
                          (hi + 1 + 0.25, False, "hi + 1"), (f32(hi + 0.999), True, "hi + 0.999"),
                          (f32(lo - 1 + 0.999), False, "lo - 1 + 0.999")):
        s.left(UL, v, oct_r, d, label, best_r=0 if hit else -1, status=PAST_SEARCH if hit else 2)
    return s.done()


def row_clamp(oracle):
    """A right keypoint at y = 1 (lo clamps to 0) and one at y = 238.5 (hi clamps to 239); left rows
    on and past both clamps, (int)(-0.5f) = 0 and rows -1 and 240, which have no candidates."""
    s = Scene(oracle, "tex", seed=80)
    d = s.word()
    s.right([190.0, 190.0], [1.0, 238.5], 0, np.stack([d, d]))
    for v, br, label in ((0.25, 0, "row 0"), (3.25, 0, "row 3 = hi"), (4.25, -1, "row 4"), (-0.5, 0, "(int)-0.5 = 0"),
                         (-1.0, -1, "row -1"), (239.5, 1, "row 239"), (236.25, 1, "row 236 = lo"),
                         (235.25, -1, "row 235"), (240.0, -1, "row 240")):
        s.left(UL, v, 0, d, label, best_r=br, status=9 if br >= 0 and (v < 5 or v > 234) else
               (PAST_SEARCH if br >= 0 else 2))
    return s.done()


def row_only(oracle):
    """A right keypoint in the row that fails the octave gate: status 3 with best_r = -1; its twin
    on a row without any right keypoint: status 2."""
    s = Scene(oracle, "tex", seed=81)
    d = s.word()
    s.right(190.0, 100.0, 3, d)
    s.left(UL, 100.0, 0, d, "octave gate only", best_r=-1, status=3)
    s.left(UL, 180.0, 0, d, "empty row", best_r=-1, status=2)
    return s.done()


# ---------------------------------------------------------------------------------------------
# patch scenes
# ---------------------------------------------------------------------------------------------

def coord_for(target, lv, scale, inv):
    """A float32 coordinate x with roundf(x * inv[lv]) == target, near the middle of its interval."""
    x = f32(f32(target) * scale[lv])
    for _ in range(16):
        got = S.std_round(x * inv[lv])
        if got == target:
            return x
        x = np.nextafter(x, UP if got < target else DOWN)
    raise AssertionError("no coordinate found")


def guard(oracle, lv):
    """On level lv (wl x hl): scaleduL in {W - 1, W, wl - W - 1, wl - W}, scaledvL likewise against
    hl, scaleduR0 in {L + W - 1, L + W, wl - (L + W + 1) - 1, wl - (L + W + 1), wl - (L + W)}.
    Expected: the left window 9 / SAD / SAD / 9 in v and at the right border in u. At the left
    border in u the right centre decides first: uR0 <= uL (the x gate), so scaleduR0 <= W < L + W and
    both keypoints get 9. The right centre: 9, SAD, SAD, 4, 4 (iniu / endu is tested before the
    guard). maxD = 400, so the x gate admits every uR <= uL."""
    s = Scene(oracle, "same", bf=400.0, b=1.0, seed=90 + lv)
    scale, inv = S.scale_tables(oracle, WIDTH, HEIGHT)
    hl, wl = images(oracle, "same")[2][lv].shape
    mu, mv = wl // 2, hl // 2
    cases = [(W - 1, mv - 12, W - 1, 9), (W, mv - 10, W, 9), (wl - W - 1, mv - 8, wl - W - 16, SAD_FORMED),
             (wl - W, mv - 6, wl - W - 15, 9),
             (mu, W - 1, mu - 8, 9), (mu, W, mu - 8, SAD_FORMED), (mu, hl - W - 1, mu - 8, SAD_FORMED),
             (mu, hl - W, mu - 8, 9),
             (mu, mv + 2, L + W - 1, 9), (mu, mv + 4, L + W, SAD_FORMED), (wl - 8, mv + 6, wl - (L + W + 1) - 1, SAD_FORMED),
             (wl - 8, mv + 8, wl - (L + W + 1), 4), (wl - 8, mv + 10, wl - (L + W), 4)]
    for sul, svl, sur0, st in cases:
        xl, xr, y = coord_for(sul, lv, scale, inv), coord_for(sur0, lv, scale, inv), coord_for(svl, lv, scale, inv)
        assert xr <= xl
        s.pair(xl, xr, y, lv, f"suL {sul} svL {svl} suR0 {sur0} of {wl} x {hl}", scaled=(sul, svl, sur0), status=st)
    return s.done()


def _half_coord(lv, scale, inv, k0, k1):
    """(k, x): a float32 x whose product x * inv[lv] is k + 0.5 exactly in float32."""
    for k in range(k0, k1):
        x = f32(f32(k + 0.5) * scale[lv])
        for step in (UP, DOWN):
            c = x
            for _ in range(32):
                if c * inv[lv] == f32(k + 0.5):
                    return k, f32(c)
                c = np.nextafter(c, step)
    return None


def round_half(oracle):
    """Level 0: uL, uR0 and vL at k + 0.5, one at a time, on the texture with true disparity 10:
    roundf takes each to k + 1, where the best increment is 0 and the SAD is 11 * sum g(row); at k
    the increment would be -1 / +1, or the SAD that of another set of rows. Then the first level
    >= 1 that has a float x with x * inv == k + 0.5 exactly: the keypoint's patch is read at k + 1
    (the builder asserts that column k gives another SAD or increment)."""
    s = Scene(oracle, "tex", seed=100)
    _, _, pl, pr = images(oracle, "tex")
    scale, inv = S.scale_tables(oracle, WIDTH, HEIGHT)

    def best(lv, sul, svl, sur0, cp):
        d = S.patch_sads(pl[lv], pr[lv], sul, svl, sur0, cp)
        return int(d.min()), int(np.argmin(d)) - L

    for xl, v, xr, sc, wrong, label in ((100.5, 80.0, 91.0, (101, 80, 91), (100, 80, 91), "uL = 100.5"),
                                        (101.0, 100.0, 90.5, (101, 100, 91), (101, 100, 90), "uR0 = 90.5"),
                                        (101.0, 140.5, 91.0, (101, 141, 91), (101, 140, 91), "vL = 140.5")):
        sad = {}
        for cp in (0, 1):
            sad[cp], inc = best(0, *sc, cp)
            assert inc == 0 and best(0, *wrong, cp) != (sad[cp], 0), label
        s.pair(xl, xr, v, label=label, scaled=sc, inc=0, sad={0: [sad[0]], 1: [sad[1]]}, status=1)
    for lv in range(1, 8):
        hl, wl = pl[lv].shape
        found = _half_coord(lv, scale, inv, 30, wl - 20)
        if found is None:
            continue
        k, x = found
        xr = f32(x - f32(12) * scale[lv])
        svl = hl // 2
        sur0 = S.std_round(xr * inv[lv])
        for cp in (0, 1):
            assert best(lv, k + 1, svl, sur0, cp) != best(lv, k, svl, sur0, cp)
        s.pair(x, xr, coord_for(svl, lv, scale, inv), lv, f"level {lv}: uL * inv = {k}.5", scaled=(k + 1, svl, sur0),
               status=SAD_FORMED)
        break
    else:
        raise AssertionError("no level has a half product")
    # the planted sad of the first three is per keypoint: flatten the {cp: [v]} entries
    sads = {cp: [p[cp][0] if p else None for p in s.plant["sad"]] for cp in (0, 1)}
    s.plant["sad"] = sads
    return s.done()


def increments(oracle):
    """The true shift (right column 140 for uL = 150) at increment -5, -4, 0, +4, +5 from scaleduR0."""
    s = Scene(oracle, "tex", seed=110)
    for k, inc in enumerate((-5, -4, 0, 4, 5)):
        s.pair(150.0, 140.0 - inc, 40.0 + 40 * k, label=f"increment {inc}", inc=inc, status=5 if abs(inc) == L else 1)
    return s.done()


def sad_first_min(oracle):
    """1-px columns on a flat ground. Right columns at scaleduR0 - 2 and + 2: equal minimal SADs at
    increments -2 and +2, the first wins (uRight = 138, d1 == d3). Right columns at - 5 and + 1:
    equal minima at -5 and +1, the first is an end: status 5."""
    s = Scene(oracle, "paint", seed=120)
    s.pair(150.0, 140.0, 150.0, label="minima at -2 and +2", inc=-2, status=1, u_right=f32(138.0), scaled=(150, 150, 140))
    s.pair(150.0, 140.0, 175.0, label="minima at -5 and +1", inc=-5, status=5, scaled=(150, 175, 140))
    return s.done()


def sad_big(oracle):
    """Flat blocks 0 against 255: SAD 121 * 255 = 30855 at every increment (0 with centred
    patches), status 5. A left patch 0 with centre 255 against a right strip 255 with the centre
    row 0: with centred patches every increment gives 110 * 510 + 10 * 255 = 58650. (One increment
    can reach 120 * 510 = 61200, a right centre 0 in a surround of 255, but its neighbours then see
    that 0 in their surround and stay near 30345, and the best SAD is the minimum of the eleven.)"""
    s = Scene(oracle, "paint", seed=130)
    s.pair(150.0, 140.0, 215.0, label="0 against 255", inc=-5, status=5, sad={0: 30855, 1: 0})
    s.pair(270.0, 255.0, 215.0, label="centred maximum", inc=-5, status=5, sad={0: None, 1: 58650})
    s.plant["sad"] = {cp: [p[cp] for p in s.plant["sad"]] for cp in (0, 1)}
    return s.done()


def disparity(oracle):
    """Level 0, integer uL = 150, 3-px bars: d1 == d3, deltaR == 0, bestuR = the right bar's
    column. Disparity 0 (the 0.01 substitution), 39 = maxD - 1 (accepted), 40 = maxD (status 7), and a
    right bar with a grey column at its right (d1 > d3, deltaR > 0, disparity < 0: status 7)."""
    s = Scene(oracle, "paint", seed=140)
    s.pair(150.0, 150.0, 30.0, label="disparity 0", inc=0, status=1, sub=True, u_right=f32(np.float64(f32(150.0)) - 0.01))
    s.pair(150.0, 111.0, 60.0, label="disparity maxD - 1", inc=0, status=1, sub=False, u_right=f32(111.0))
    s.pair(150.0, 110.0, 90.0, label="disparity maxD", inc=0, status=7)
    s.pair(150.0, 150.0, 120.0, label="disparity < 0", inc=0, status=7)
    return s.done()


# ---------------------------------------------------------------------------------------------
# every matching scene by name
# ---------------------------------------------------------------------------------------------

MATCH = {}
LANE_NR = (1, 63, 64, 65, 127, 128, 129, 4097)
for _n in LANE_NR:
    for _p in sorted({p for p in (0, 63, 64, _n - 1) if p < _n}):
        MATCH[f"lane-{_n}-at-{_p}"] = (search, (_n, {_p: 20}))
TIE_A = 69
for _m in (1, 2, 4, 8, 16, 32):
    MATCH[f"tie-step-{_m}"] = (search, (130, {TIE_A: 20, TIE_A ^ _m: 20}))
MATCH["tie-stride"] = (search, (130, {7: 20, 71: 20}))
MATCH["tie-three"] = (search, (200, {100: 20, 37: 20, 165: 20}))
MATCH["last-index"] = (search, (65535, {65534: 20}, False))
MATCH["last-index-tie"] = (search, (65535, {0: 20, 65534: 20}, False))
for _d in (74, 75, 99, 100):
    MATCH[f"dist-{_d}"] = (search, (1, {0: _d}))
MATCH["window-exact"] = (window, (True,))
MATCH["window-inexact"] = (window, (False,))
for _o in (0, 3, 7):
    MATCH[f"octave-{_o}"] = (octave, (_o,))
for _o in (0, 4, 7):
    MATCH[f"row-oct{_o}-int"] = (row_band, (_o, 100.0))
    MATCH[f"row-oct{_o}-frac"] = (row_band, (_o, 100.3))
MATCH["row-clamp"] = (row_clamp, ())
MATCH["row-only"] = (row_only, ())
for _n in (1, 3, 4, 5):
    MATCH[f"nl-{_n}"] = (nl_scene, (_n,))
PATCH = []
for _lv in (0, 3, 7):
    MATCH[f"guard-lv{_lv}"] = (guard, (_lv,))
    PATCH.append(f"guard-lv{_lv}")
for _name, _fn in (("round-half", round_half), ("inc", increments), ("sad-first-min", sad_first_min),
                   ("sad-big", sad_big), ("disp", disparity)):
    MATCH[_name] = (_fn, ())
    PATCH.append(_name)

_cache = {}


def match_scene(oracle, name):
    """The scene of that name, built once."""
    if name not in _cache:
        fn, args = MATCH[name]
        _cache[name] = fn(oracle, *args)
    return _cache[name]


def planted(s, key, cp):
    """The planted list of `key` for center_patch cp."""
    p = s["plant"][key]
    return p[cp] if isinstance(p, dict) else p


# ---------------------------------------------------------------------------------------------
# median scenes
# ---------------------------------------------------------------------------------------------

SAD_MAX = 61710     # 121 * 510: above every SAD the rule can form (issue: accepted SADs lie in [0, 61710])


def median_scene(acc_sads, extra, seed, **plant):
    """The accepted SADs `acc_sads` (status 1) shuffled among `extra` entries of status 2..9: sad -1 on
    those that never formed one (2, 3, 4, 9), a random SAD on 5..8. u_right = 1000.25 + i,
    depth = 2000.5 + i everywhere."""
    rng = np.random.default_rng(seed)
    acc_sads = np.asarray(acc_sads, np.int64)
    n = len(acc_sads) + extra
    status = np.zeros(n, np.int32)
    sad = np.zeros(n, np.int32)
    pos = np.sort(rng.choice(n, size=len(acc_sads), replace=False)) if len(acc_sads) else np.zeros(0, np.int64)
    status[pos] = 1
    sad[pos] = rng.permutation(acc_sads)
    rest = np.flatnonzero(status == 0)
    status[rest] = 2 + np.arange(len(rest)) % 8
    formed = np.isin(status[rest], (5, 6, 7, 8))
    sad[rest] = np.where(formed, rng.integers(0, SAD_MAX + 1, len(rest)), -1)
    i = np.arange(n)
    plant["n_accepted"] = len(acc_sads)
    if len(acc_sads) and "median" not in plant:
        plant["median"] = None
    return dict(status=status, sad=sad, u_right=(1000.25 + i).astype(f32), depth=(2000.5 + i).astype(f32), plant=plant)


def _threshold(m):
    th = f32(f32(1.5) * f32(1.4)) * f32(m)
    lo, hi = int(np.floor(th)), int(np.ceil(th))
    edge = [lo, hi, hi + 1] if lo < hi else [lo - 1, lo, lo + 1]     # thDist itself where it is an integer
    return [m] * 7 + edge, [v for v in edge if f32(v) >= th], [v for v in edge if not f32(v) >= th]


def _build_median():
    M = {}
    rng = np.random.default_rng(900)
    for c in (0, 2, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4097):
        M[f"count-{c}"] = median_scene(rng.integers(0, SAD_MAX + 1, c), 9, 901 + c)
    M["count-1-sad0"] = median_scene([0], 5, 910, median=0, cut_sads=[0])
    M["count-1-sad7"] = median_scene([7], 5, 911, median=7, kept_sads=[7])
    for v in (0, 255, 256, 32768, SAD_MAX):
        M[f"equal-{v}"] = median_scene([v] * 37, 6, 920 + v % 97, median=v, **({"cut_sads": [0]} if v == 0 else {"kept_sads": [v]}))
    for v in (254, 255, 256, 511, 32767, SAD_MAX - 1):
        total = 10 if v < 1000 else 2050      # rank 5 / 1025: below and past the 1024-thread stride
        rank = total // 2
        M[f"two-{v}-last"] = median_scene([v] * (rank + 1) + [v + 1] * (total - rank - 1), 7, 930 + v % 89,
                                          median=v, rank_edge="last", v=v)
        M[f"two-{v}-first"] = median_scene([v] * rank + [v + 1] * (total - rank), 7, 931 + v % 89,
                                           median=v + 1, rank_edge="first", v=v)
    for hb in (0, 127, 128, 241):
        m = hb * 256 + 7
        lo = rng.integers(0, m, 40) if m > 0 else []
        hi = rng.integers(m + 1, SAD_MAX + 1, 40)
        M[f"high-byte-{hb}"] = median_scene(np.concatenate([lo, [m], hi]).astype(np.int64), 8, 940 + hb, median=m)
    # pass 1's filter: 300 SADs in the median's high byte (0x31) with low bytes 200..255, 200 below
    # and 320 above it with low bytes 0..39: a second histogram without the filter finds a low byte
    # below 40 at the same rank, a thDist some 400 lower, and cuts the SAD planted just below thDist
    inside = 0x3100 + rng.integers(200, 256, 300)
    below = (rng.integers(0, 0x31, 200) << 8) + rng.integers(0, 40, 200)
    above = (rng.integers(0x32, 0xF0, 320) << 8) + rng.integers(0, 40, 320)
    base = np.concatenate([inside, below, above])
    med = int(np.sort(base)[len(base) // 2])
    _, cut, kept = _threshold(med)
    allv = np.concatenate([base, [0, 1], [max(kept), min(cut)]])     # two below, two above: the same median
    M["filter"] = median_scene(allv, 11, 950, median=med, cut_sads=[min(cut)], kept_sads=[max(kept)])
    for m in (1, 10, 100, 1000, 14693):
        sads, cut, kept = _threshold(m)
        M[f"threshold-{m}"] = median_scene(sads, 4, 960 + m % 83, median=m, cut_sads=cut, kept_sads=kept)
    return M


MEDIAN = _build_median()


def median_expect(m):
    """The restatement's result on a median scene: (status, u_right, depth, n_stereo)."""
    st, u, z = m["status"].copy(), m["u_right"].copy(), m["depth"].copy()
    for i in S.median_cut(m["sad"], np.flatnonzero(m["status"] == 1)):
        st[i], u[i], z[i] = S.ST_MEDIAN, f32(-1), f32(-1)
    return st, u, z, int((st == 1).sum())
