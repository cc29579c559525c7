"""The planted stereo scenes (tests/stereo_cases.py) on the CPU: for every scene the restatement
(tests/stereo_numpy.py) must give the planted figures, so a scene that misses the edge it is named
for fails here, before tests/test_stereo_cases_gpu.py compares the device with the restatement on
it. The median scenes are checked against upstream's sort-and-walk-back loop as well."""
import os

import numpy as np
import pytest

import stereo_cases as C
import stereo_numpy as S

f32 = np.float32


def restate(s, cp):
    return S.restate(s, cp)


@pytest.mark.parametrize("cp", [0, 1])
@pytest.mark.parametrize("name", list(C.MATCH))
def test_scene_reaches_its_plant(oracle, name, cp):
    s = C.match_scene(oracle, name)
    r = restate(s, cp)
    n = len(s["kps_l"])
    assert n == len(s["labels"]) and n > 0
    planted_any = False
    for i in range(n):
        what = f"{name} [{i}] {s['labels'][i]}"
        for key, got in (("best_r", r.best_r), ("best_dist", r.best_dist), ("n_tied", r.n_tied), ("inc", r.best_inc),
                         ("sad", r.sad), ("sub", r.sub)):
            want = C.planted(s, key, cp)[i]
            if want is not None:
                planted_any = True
                assert got[i] == want, f"{what}: {key} {got[i]} planted {want}"
        want = C.planted(s, "status", cp)[i]
        if want == C.SAD_FORMED:
            assert r.sad[i] >= 0 and r.status[i] in (1, 5, 7, 8), f"{what}: status {r.status[i]}, no SAD formed"
        elif want == C.PAST_SEARCH:
            assert r.status[i] not in (2, 3), f"{what}: status {r.status[i]}"
        elif want is not None:
            assert r.status[i] == want, f"{what}: status {r.status[i]} planted {want}"
        want = C.planted(s, "scaled", cp)[i]
        if want is not None:
            for k in range(3):
                assert want[k] is None or r.scaled[i, k] == want[k], f"{what}: scaled {r.scaled[i].tolist()} planted {want}"
        want = C.planted(s, "u_right", cp)[i]
        if want is not None:
            assert r.u_right[i].view(np.uint32) == f32(want).view(np.uint32), f"{what}: u_right {r.u_right[i]!r}"
    assert planted_any
    assert r.events["max_abs_delta"] <= 0.5


def test_scene_names_cover_the_edges():
    names = set(C.MATCH)
    for n_r in C.LANE_NR:
        for p in (0, 63, 64, n_r - 1):
            assert (f"lane-{n_r}-at-{p}" in names) == (p < n_r)
    for m in (1, 2, 4, 8, 16, 32):
        assert f"tie-step-{m}" in names
    assert {"tie-stride", "tie-three", "last-index", "last-index-tie", "dist-74", "dist-75", "dist-99", "dist-100",
            "window-exact", "window-inexact", "octave-0", "octave-3", "octave-7", "row-clamp", "row-only", "nl-1",
            "nl-3", "nl-4", "nl-5", "guard-lv0", "guard-lv3", "guard-lv7", "round-half", "inc", "sad-first-min",
            "sad-big", "disp"} <= names


def test_search_scenes_hold_their_ties_and_lanes(oracle):
    """The tie scenes really tie (two or three candidates at the best distance, the lowest index
    wins, and the partners sit where the scene's name says); every other candidate of a lane scene is
    at least 10 bits worse; the fillers would win if the x gate let them through."""
    for m in (1, 2, 4, 8, 16, 32):
        s = C.match_scene(oracle, f"tie-step-{m}")
        r = restate(s, 0)
        assert r.n_tied[0] == 2 and r.best_r[0] == min(C.TIE_A, C.TIE_A ^ m) and r.best_dist[0] == 20
    r = restate(C.match_scene(oracle, "tie-stride"), 0)
    assert r.n_tied[0] == 2 and r.best_r[0] == 7
    r = restate(C.match_scene(oracle, "tie-three"), 0)
    assert r.n_tied[0] == 3 and r.best_r[0] == 37
    r = restate(C.match_scene(oracle, "last-index-tie"), 0)
    assert r.n_tied[0] == 2 and r.best_r[0] == 0
    s = C.match_scene(oracle, "last-index")
    assert len(s["kps_r"]) == 65535 and restate(s, 0).best_r[0] == 65534
    for name in ("lane-129-at-64", "lane-4097-at-4096", "lane-64-at-63"):
        s = C.match_scene(oracle, name)
        r = restate(s, 0)
        d = S._POP[s["desc_r"] ^ s["desc_l"][0]].sum(axis=1)
        in_x = (s["kps_r"]["x"] >= 160) & (s["kps_r"]["x"] <= 200)
        others = np.flatnonzero(in_x & (np.arange(len(d)) != r.best_r[0]))
        assert (d[others] >= 30).all() and d[r.best_r[0]] == 20
        assert (d[~in_x] <= 5).all() and (~in_x).sum() >= len(d) // 2


def test_patch_scenes_show_their_edges(oracle):
    for cp in (0, 1):
        s = C.match_scene(oracle, "sad-first-min")
        r = restate(s, cp)
        assert r.events["sad_tie"] == 2                      # both keypoints have two equal minima
        s = C.match_scene(oracle, "disp")
        r = restate(s, cp)
        assert r.events["disparity_sub"] == 1 and r.depth[0] == f32(s["bf"]) / f32(0.01)
        assert r.depth[1] == f32(40) / f32(39) and r.n_stereo == 2
        # disparity < 0 through deltaR > 0: d1 > d3 at increment 0
        d = S.patch_sads(s["pyr_l"][0], s["pyr_r"][0], 150, 120, 150, cp)
        assert int(np.argmin(d)) == C.L and d[C.L - 1] > d[C.L + 1]
        r = restate(C.match_scene(oracle, "inc"), cp)
        assert r.status.tolist() == [5, 1, 1, 1, 5] and (r.sad > 0).all()
    r = restate(C.match_scene(oracle, "sad-big"), 1)
    assert r.sad[1] > 255 * 121      # past what raw patches can reach


def test_guard_scenes_use_their_level(oracle):
    """On levels 3 and 7 the planted border keypoints would pass a guard taken from level 0."""
    for lv in (3, 7):
        s = C.match_scene(oracle, f"guard-lv{lv}")
        r = restate(s, 0)
        hl, wl = s["pyr_l"][lv].shape
        nine = np.flatnonzero(r.status == 9)
        assert (r.scaled[nine, 0] >= wl - C.W).sum() == 1 and (r.scaled[nine, 1] >= hl - C.W).sum() == 1
        assert (r.status == 4).sum() == 2 and wl < C.WIDTH - 2 * C.W


@pytest.mark.parametrize("name", list(C.MEDIAN))
def test_median_scene(name):
    m = C.MEDIAN[name]
    acc = np.flatnonzero(m["status"] == 1)
    p = m["plant"]
    assert len(acc) == p["n_accepted"] and len(m["status"]) > len(acc)
    assert set(m["status"].tolist()) >= ({2, 3, 4, 5, 7, 9} if len(m["status"]) - len(acc) >= 8 else {2, 3, 4, 5})
    assert (m["sad"][np.isin(m["status"], (2, 3, 4, 9))] == -1).all()
    assert (m["sad"][acc] >= 0).all() and (m["sad"][acc] <= C.SAD_MAX).all()
    cut = S.median_cut(m["sad"], acc)
    assert sorted(cut) == sorted(C.upstream_median_loop(m["sad"], acc))
    st, u, z, ns = C.median_expect(m)
    assert ns == len(acc) - len(cut) and (st == 8).sum() == len(cut) + (m["status"] == 8).sum()
    keep = np.ones(len(st), bool)
    keep[cut] = False
    assert np.array_equal(st[keep], m["status"][keep]) and np.array_equal(u[keep], m["u_right"][keep])
    assert (u[cut] == -1).all() and (z[cut] == -1).all() if len(cut) else True
    if not len(acc):
        return
    srt = np.sort(m["sad"][acc])
    rank = len(acc) // 2
    if p.get("median") is not None:
        assert srt[rank] == p["median"], (srt[rank], p["median"])
    if "rank_edge" in p:
        v = p["v"]
        assert set(srt.tolist()) == {v, v + 1}
        if p["rank_edge"] == "last":
            assert srt[rank] == v and srt[rank + 1] == v + 1
        else:
            assert srt[rank - 1] == v and srt[rank] == v + 1
    cut_sads = set(m["sad"][cut].tolist())
    for v in p.get("cut_sads", []):
        assert v in cut_sads, (v, cut_sads)
    for v in p.get("kept_sads", []):
        assert v not in cut_sads and v in set(m["sad"][acc].tolist()), (v, cut_sads)


def test_median_scene_set():
    names = set(C.MEDIAN)
    for c in (0, 2, 3, 4, 255, 256, 257, 1023, 1024, 1025, 4097):
        assert C.MEDIAN[f"count-{c}"]["plant"]["n_accepted"] == c
    assert {"count-1-sad0", "count-1-sad7", "filter"} <= names
    for hb in (0, 127, 128, 241):
        assert C.MEDIAN[f"high-byte-{hb}"]["plant"]["median"] >> 8 == hb
    # the filter scene: the second histogram without the filter would select another value
    m = C.MEDIAN["filter"]
    sads = m["sad"][m["status"] == 1]
    med = m["plant"]["median"]
    inside = sads[(sads >> 8) == (med >> 8)]
    assert len(inside) >= 250 and len(sads) - len(inside) >= 500
    rank1 = len(sads) // 2 - (sads < (med >> 8) << 8).sum()
    wrong = (med & ~255) | int(np.sort(sads & 255)[rank1])
    assert np.sort(inside & 255)[rank1] == med & 255 and wrong < med - 100
    assert f32(m["plant"]["kept_sads"][0]) >= f32(f32(1.5) * f32(1.4)) * f32(wrong)     # the unfiltered select cuts it
    # the threshold scenes: a SAD equal to thDist exists where thDist is an integer
    on_th = 0
    for mm in (1, 10, 100, 1000, 14693):
        p = C.MEDIAN[f"threshold-{mm}"]["plant"]
        th = f32(f32(1.5) * f32(1.4)) * f32(mm)
        assert p["cut_sads"] and p["kept_sads"] and len(p["cut_sads"]) + len(p["kept_sads"]) == 3
        assert max(p["kept_sads"]) + 1 == min(p["cut_sads"])
        assert min(p["cut_sads"]) == int(np.ceil(th)) and all(f32(v) < th for v in p["kept_sads"])
        on_th += f32(min(p["cut_sads"])) == th
    assert on_th >= 1


def test_median_hook_is_exported_but_not_declared():
    from orb_slam3_ros2_amd import _lib
    assert hasattr(_lib.lib(), "orbhip_test_stereo_median") and "orbhip_test_stereo_median" not in _lib.EXPORTED
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "orbhip.h")) as f:
        assert "orbhip_test_stereo_median" not in f.read()
