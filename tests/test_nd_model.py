"""CPU: the plan model of the nested dissection (tests/nd_model.py) on the shapes
tests/test_nd_edges_gpu.py solves, and on the shapes tests/test_nd_gpu.py has always solved.

k_nd_backsolve keeps two tiles per wave and interior column in registers and loads any further
one inside the step. Which of those paths a system reaches is a property of its plan alone, so it
is pinned here, without a device: were a case of the GPU tests to drift off the path it was
chosen for (another segmentation rule, another tile size), these assertions fail first.

Per segment: (interior poses, nti, NT, phase-1 maximum, phase-2 maximum, padding rows); the
maxima are the most tiles one of the four waves meets in one interior column (1: first register
slot, 2: both slots, >= 3: the in-step loads too)."""
import pytest

import nd_model as M

# (n_pose, w, cyclic, K) -> per-segment figures; the shapes test_nd_edges_gpu.py solves
PLANNED = {
    (100, 24, True, 2): [(26, 5, 14, 3, 1, 4)] * 2,
    (192, 48, True, 2): [(48, 9, 27, 5, 2, 0)] * 2,                      # interior = w, no padding
    (203, 48, True, 2): [(53, 10, 28, 5, 3, 2), (54, 11, 29, 5, 3, 28)],   # uneven; even and odd nti
    (264, 65, True, 2): [(67, 13, 38, 7, 3, 14)] * 2,
    (150, 24, False, 2): [(51, 10, 15, 2, 2, 14), (75, 15, 20, 2, 2, 30)],
    # a line: no previous separator / both / no own separator
    (300, 48, False, 3): [(52, 10, 19, 3, 3, 8), (52, 10, 28, 5, 3, 8), (100, 19, 28, 3, 3, 8)],
    (664, 114, True, 2): [(218, 41, 84, 11, 6, 4)] * 2,                  # the LDS ceiling
    (576, 48, True, 6): [(48, 9, 27, 5, 2, 0)] * 6,                      # second level
}
REFUSED = {
    (191, 48, True, 2): M.REFUSED_NARROW,   # interiors of 47 and 48 poses
    (666, 114, True, 2): M.REFUSED_LDS,     # 85 tiles
}
# what tests/test_nd_gpu.py solves: (n_pose, w, cyclic, K), K = 0 the automatic plan
OLD_SHAPES = [(120, 7, True, 0), (120, 7, True, 2), (120, 7, True, 5), (96, 5, False, 3), (96, 5, False, 0),
              (399, 19, True, 0), (399, 19, True, 8), (200, 3, True, 16), (399, 19, True, 6), (399, 19, True, 7),
              (399, 19, True, 10)]


def test_lds_ceiling_is_84_tiles():
    assert M.MAX_SEG_TILES == 84
    assert M.bs_lds_bytes(84) == 130640 <= M.LDS_CAP < M.bs_lds_bytes(85)


@pytest.mark.parametrize("case", sorted(PLANNED))
def test_planned_case_reaches_its_paths(case):
    p = M.plan(*case)
    assert p.ok, p.refused
    assert p.seg == [r * case[0] // case[3] for r in range(case[3] + 1)]
    fig = M.segment_figures(p)
    print(case, fig)
    assert fig == PLANNED[case]
    for s, f in zip(p.segments, fig):
        assert s.rows == M.TILE * s.nti + 6 * p.w * ((s.prev_sep is not None) + (s.own_sep is not None))
        assert s.padding == s.nip - 6 * s.interior_poses and 0 <= s.padding < M.TILE
        assert s.interior_poses >= p.w and s.NT <= M.MAX_SEG_TILES


def test_cases_cover_every_backsolve_path():
    """Over the planned cases: phase 1 and phase 2 each at 1 or 2 (registers only) and at >= 3
    (in-step loads), phase 2 at exactly 2 (the second slot, no in-step load); interiors of even
    and of odd tile counts (the two register sets end on either parity); an interior without
    padding and padded ones; segments with one and with two separators."""
    fig = [f for c in PLANNED for f in PLANNED[c]]
    assert {min(f[3], 3) for f in fig} == {2, 3} and {min(f[4], 3) for f in fig} == {1, 2, 3}
    assert {f[1] % 2 for f in fig} == {0, 1}
    assert any(f[5] == 0 for f in fig) and any(f[5] > 0 for f in fig)
    line = M.plan(300, 48, False, 3).segments
    assert [(s.prev_sep is None, s.own_sep is None) for s in line] == [(True, False), (False, False), (False, True)]
    # phase 1 needs w >= 22 poses for its in-step loads, phase 2 w >= 43 (whole band inside an
    # interior): the narrowest bands that reach them on a 2-segment loop
    for w, ph in ((21, 0), (22, 0), (42, 1), (43, 1)):
        f = M.segment_figures(M.plan(8 * w, w, True, 2))
        assert (max(x[3 + ph] for x in f) > M.REG_TILES) == (w in (22, 43)), (w, f)


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_refused_case(case):
    assert M.plan(*case).refused == REFUSED[case]


def test_refusal_rules():
    assert M.plan(40, 2, True, 8).refused == M.REFUSED_ONE_TILE      # interiors of 3 poses: 18 rows
    assert M.plan(40, 2, True, 4).ok                                # 8 poses: 48 rows
    assert M.plan(1400, 99, True, 7).refused == M.REFUSED_SEPARATOR   # 7 separators of 594 rows
    assert M.plan(1400, 97, True, 7).ok                             # 4074 rows
    p = M.plan(666, 114, True, 2)
    assert [s.NT for s in p.segments] == [85, 85]
    assert M.plan(664, 114, True, 2).max_NT == 84


def test_automatic_plan_of_the_wide_band():
    """664 poses, w = 114: only K = 2 leaves interiors as wide as the band, its segments are 84
    tiles and its chain (41 + 43 + 3 of 125 tile intervals) pays: the automatic plan. 666 and 680
    poses: K = 2 alone is possible there too, at 85 and 86 tiles: never planned."""
    a = M.automatic_plan(664, 114, True)
    assert a is not None and a.K == 2 and a.max_NT == 84
    assert [q.K for q in M.automatic_candidates(664, 114, True)] == [2]
    assert M.modelled_chain(a) == 87 and M.tiles(6 * 664) == 125
    for n_pose, nt in ((666, 85), (680, 86)):
        assert 680 // (2 * 114) == 2 and M.plan(n_pose, 114, True, 2).refused == M.REFUSED_LDS
        assert M.plan(n_pose, 114, True, 2).segments[0].NT == nt
        assert M.automatic_candidates(n_pose, 114, True) == [] and M.automatic_plan(n_pose, 114, True) is None
    assert M.automatic_candidates(60, 40, False) == []   # test_nd_not_planned_for_a_dense_system


def test_second_level_of_576_48_6():
    p = M.plan(576, 48, True, 6)
    q = M.second_level(p)
    assert q is not None and q.K == 3 and q.seg == [0, 96, 192, 288] and q.w == 48
    # inner interiors = the even separators, inner separators = the odd ones
    assert [s.interior for s in q.segments] == [(0, 48), (96, 144), (192, 240)]
    assert [s.own_sep for s in q.segments] == [(48, 96), (144, 192), (240, 288)]
    fig = M.segment_figures(q, M.second_level_adjacency(p))
    assert fig == [(48, 9, 27, 5, 2, 0)] * 3
    assert M.second_level(M.plan(192, 48, True, 2)) is None      # fewer than 6 separators
    assert M.second_level(M.plan(300, 48, False, 3)) is None     # a line
    assert M.second_level(M.plan(200, 3, True, 16)) is None      # separators of 18 rows: within one tile
    q7 = M.second_level(M.plan(399, 19, True, 7))                # K odd: the last interior holds two separators
    assert q7.seg == [0, 38, 76, 133] and [s.interior_poses for s in q7.segments] == [19, 19, 38]


@pytest.mark.parametrize("shape", OLD_SHAPES)
def test_old_shapes_stay_within_the_registers(shape):
    """Every system tests/test_nd_gpu.py solves (w <= 19), whichever K the automatic plan takes: in
    the dissection itself phase 1 meets at most 2 tiles per wave and column and phase 2 exactly 1.
    The second level (the separator system's own dissection, K >= 6) stays within the two register
    slots too; its phase 2 reaches the second slot only where K is odd, in the last inner segment
    (an interior of two separators, 38 poses, coupled throughout). No in-step load anywhere. Hence
    the cases above."""
    n_pose, w, cyclic, K = shape
    plans = [M.plan(n_pose, w, cyclic, K)] if K else M.automatic_candidates(n_pose, w, cyclic)
    assert plans and all(p.ok for p in plans)
    for p in plans:
        fig = M.segment_figures(p)
        assert max(f[3] for f in fig) <= 2 and {f[4] for f in fig} == {1}, (p.K, fig)
        q = M.second_level(p)
        if q is not None:
            fig = M.segment_figures(q, M.second_level_adjacency(p))
            assert max(f[3] for f in fig) <= M.REG_TILES, (p.K, fig)
            assert [f[4] for f in fig[:-1]] == [1] * (q.K - 1) and fig[-1][4] <= (2 if p.K % 2 else 1), (p.K, fig)
            if (w, p.K) == (19, 7):
                assert fig[-1][4] == 2


def test_bandwidth_rule():
    assert M.bandwidth(10, [0, 0, 3], [2, 9, 3]) == (9, 2)
    assert M.band_of(10, [0, 0, 3], [2, 9, 3]) == (2, True)
    assert M.band_of(10, [0, 1], [2, 4]) == (3, False)
