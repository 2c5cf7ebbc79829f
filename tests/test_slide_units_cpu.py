"""The second work unit of a workgroup, without a GPU: what tests/test_gpu_slide_units.py relies on.  The geometry of every case (units,
workgroups, trips per workgroup, restated in tests/slide_units_reference.py), the kinds of pixels its rasters hold, and the successions
of the segmenter's rows counted on the reference's output alone."""
import numpy as np
import pytest

import load_reference as lr
import segment_reference as sg
import slide_units_reference as su
import spatial_reference as sp
import stain_reference as sref


def test_trips():
    assert su.trips(9, 9) == (1, 1) and su.trips(2049, 2048) == (1, 2) and su.trips(4096, 2048) == (2, 2) and su.trips(4396, 2048) == (2, 3)


@pytest.mark.parametrize("shrink", [1, 2])
def test_strip_cases_reach_the_third_unit(shrink):
    """cases 1 and 2: 4 396 units of 16 rows for 2 048 workgroups, on the load pass and on the histogram passes"""
    for band_xq in (su.LOAD, su.HIST):
        nq, n_xc, units, blocks = su.slide_units(su.STRIP_W, shrink, su.STRIP_H, *band_xq)
        assert (nq, n_xc, units, blocks) == (3 * shrink if shrink == 1 else 5, 1, 4396, su.CAP) and su.trips(units, blocks) == (2, 3)
    r = su.strip_raster(shrink)
    assert r.shape == su.source_shape(su.STRIP_H, su.STRIP_W, shrink) + (3,)
    assert (3 * r.shape[1]) % 16 != 0                               # the tight stride takes the byte loads
    t, q = lr.classes(r, shrink, su.BG, sref.tables(), 1)
    pos, core = t & (q >= sg.THRES_BIN), t & (q >= sg.CORE_BIN)
    assert 0 < core.sum() < pos.sum() < t.sum() < t.size            # glass, tissue, positive and core pixels all occur
    band = 16
    for u in (0, 1, 299, 2047):                                     # a workgroup's consecutive units differ in content
        a, b, c = (t[(u + k * su.CAP) * band:(u + k * su.CAP + 1) * band] for k in range(3))
        assert not np.array_equal(a, b) and (len(c) == 0 or not np.array_equal(b[:len(c)], c))


def test_flush_case_flushes_once_in_the_middle_and_goes_on():
    """case 3: every workgroup counts HIST_FLUSH units, flushes, and has one or two units left"""
    nq, n_xc, units, blocks = su.slide_units(1, 1, su.FLUSH_H, *su.HIST)
    assert (nq, n_xc, blocks) == (1, 1, su.CAP) and units == su.HIST_FLUSH * su.CAP + su.CAP + 9
    lo, hi = su.trips(units, blocks)
    assert (lo - su.HIST_FLUSH, hi - su.HIST_FLUSH) == (1, 2) and hi < 2 * su.HIST_FLUSH
    assert (16 * su.CAP) % su.FLUSH_PERIOD != 0 and all(su.FLUSH_PERIOD % p for p in range(2, 65))        # a prime: no shared period
    col, block, reps, rem = su.flush_column()
    assert col.shape == (su.FLUSH_H, 1, 3) and reps * su.FLUSH_PERIOD + rem == su.FLUSH_H and 0 < rem
    assert np.array_equal(col[-rem - su.FLUSH_PERIOD:-rem], block) and np.array_equal(col[-rem:], block[:rem])
    t, q = lr.classes(block, 1, su.BG, sref.tables(), 1)
    assert 0 < (t & (q >= sg.CORE_BIN)).sum() < (t & (q >= sg.THRES_BIN)).sum() < t.sum() < t.size


def test_focus_cases_reach_the_second_unit():
    """case 4: (a) 4 396 units one across, the cell row changing inside most units; (b) two units across: as 2 048 is even, a
    workgroup's units have ONE width; (c) three across: the width changes between the trips of every workgroup that makes two"""
    W, H, cell = su.FOCUS_A
    for shrink in (1, 2):
        nq, n_xc, units, blocks = su.focus_units(W, shrink, H)
        assert (n_xc, units, blocks) == (1, 4396, su.CAP) and su.trips(units, blocks) == (2, 3)
    first = 1 + 32 * np.arange(4396)                                # a unit's first centre row; its last is 31 further, or H - 2
    crosses = first // cell != np.minimum(first + 31, H - 2) // cell
    assert crosses[su.CAP:2 * su.CAP].sum() > 1000 and crosses[2 * su.CAP:].sum() > 100 and (~crosses[su.CAP:]).sum() > 500
    W, H, _ = su.FOCUS_B
    nq, n_xc, units, blocks = su.focus_units(W, 1, H)
    assert (nq, n_xc, units, blocks) == (33, 2, 2062, su.CAP) and su.trips(units, blocks) == (1, 2)
    assert all(su.unit_wq(u, n_xc, nq, 32) == su.unit_wq(u + su.CAP, n_xc, nq, 32) for u in range(units - su.CAP))
    W, H, _ = su.FOCUS_C
    nq, n_xc, units, blocks = su.focus_units(W, 1, H)
    assert (nq, n_xc, units, blocks) == (65, 3, 2073, su.CAP) and su.trips(units, blocks) == (1, 2)
    widths = {(su.unit_wq(u, n_xc, nq, 32), su.unit_wq(u + su.CAP, n_xc, nq, 32)) for u in range(units - su.CAP)}
    assert widths == {(32, 1), (32, 32), (1, 32)}


def test_tissue_cases_pass_the_cap():
    """case 5"""
    assert su.tissue_units(1000, 1000, 24, 16) == (2, 126, 1, 126, 15876, su.TISSUE_CAP)
    assert su.tissue_units(1460, 1460, 16, 16) == (1, 92, 1, 92, 8464, su.TISSUE_CAP)
    assert su.trips(15876, su.TISSUE_CAP) == (1, 2) and su.trips(8464, su.TISSUE_CAP) == (1, 2)


def test_box_case_gives_a_wavefront_three_boxes():
    """case 6"""
    r, rows, k = su.box_case()
    M = len(rows)
    assert M == su.BOX_M == 2 * 8192 + 77 and su.box_walk_waves(M) == su.BOX_CAP == 8192 and su.trips(M, su.BOX_CAP) == (2, 3) and k < 77
    finite, e = lr.edges(rows, *su.BOX_HW)
    three = [k, k + su.BOX_CAP, k + 2 * su.BOX_CAP]                  # one wavefront's boxes: not finite, empty, off the slide
    assert not finite[three[0]] and finite[three[1]] and e[three[1], 0] == e[three[1], 2] and finite[three[2]] and e[three[2], 0] == e[three[2], 2] == 400
    assert e[k + 1, 0] > e[k + 1, 2] and lr.owned_pixels(rows, *su.BOX_HW)[[k + 1 + su.BOX_CAP, k + 1 + 2 * su.BOX_CAP]].min() > 0
    assert (lr.owned_pixels(rows, *su.BOX_HW) > 0).sum() > 0.9 * M


@pytest.mark.slow
def test_segment_rows_follow_each_other_as_the_kernel_tests_need():
    """case 7, on the reference alone: each succession of a workgroup's boxes (m, m + 2048) occurs at least 10 times"""
    M = su.SEG_M
    assert M == 2 * 2048 + 37 and su.segment_blocks(M) == su.SEG_CAP and su.trips(M, su.SEG_CAP) == (2, 3)
    short, short_flags, whole, whole_flags = su.segment_want()
    assert short_flags == sg.NONFINITE | sg.EMPTY | sg.LARGE | sg.NOT_RESIDENT and whole_flags == sg.NONFINITE | sg.EMPTY | sg.LARGE
    counts = su.segment_successions(short)
    print(counts)
    assert min(counts.values()) >= 10, counts
    ok = short[:, 0] == 0
    assert (ok & (short[:, 6] >= 2)).sum() >= 100 and (ok & (short[:, 8] > 0)).sum() >= 100 and (ok & (short[:, 17] != 0)).sum() >= 100
    away = short[:, 0] == sg.NOT_RESIDENT
    assert (whole[away, 0] == 0).all() and (whole[away, 7] > 0).sum() >= 10 and np.array_equal(whole[~away], short[~away])
    # through strips of 255 rows an owner-row `continue` falls between the boxes of one workgroup
    plan = sg.strip_plan(su.SEG_H, 255)
    owner = sg.windows(su.segment_rows(), su.SEG_H, su.SEG_W, su.SEG_MARGIN)[3]
    strip_of = np.searchsorted([p[3] for p in plan], owner, side="right")
    assert len(plan) == 46 and (strip_of[:-su.SEG_CAP] != strip_of[su.SEG_CAP:]).sum() > 1000


def test_pair_rows_give_a_group_three_centres():
    """case 8: more than 2 * 32 768 + 500 counted rows for 32 768 groups of 16 lanes"""
    rows = su.pair_rows()
    cls = sp.positions(rows, sp.SLIDE_H, sp.SLIDE_W, su.PAIR_CLASSES, 0.5)[2]
    counted = int((cls >= 0).sum())
    assert su.pair_groups(len(rows)) == su.PAIR_CAP == 32768 and counted >= 2 * su.PAIR_CAP + 500 and su.trips(counted, su.PAIR_CAP) == (2, 3)
    assert len(rows) - counted > 1000                               # flagged rows and rows below the threshold among them


def test_element_loops_pass_their_cap():
    """case 9 and the stateless element loops of the cut, the ingest and the unview kernels"""
    assert su.element_threads(su.APPLY_SIDE ** 2) == su.ELEMENT_CAP == 2097152 < su.APPLY_SIDE ** 2
    # the full-shape tests of the neighbours stop at the cap or far below it: 2 x 1024^2 pixels are exactly one trip
    assert su.element_threads(2 * 1024 * 1024) == 2 * 1024 * 1024
