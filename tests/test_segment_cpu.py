"""CPU: the restatement of THE SEGMENT RULE (tests/segment_reference.py) on hand-worked shapes, its ownership and residency model, its
flood fill against scipy, wsi.plaque_morphometry on hand-made words, the host argument checks of wsi.segment_boxes and
quantify_region(segment=True) (no device is touched), the inputs of the GPU tests (the counts they promise), header and binding."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import load_reference as lr
import segment_reference as sr
import stain_reference as sref
from amyloid_yolo_paper_amd import _lib, wsi

NAN, INF = float("nan"), float("inf")


def run(pos, core, rows, margin, min_area=1):
    """the rule on boolean images: every pixel is tissue, positive pixels have bin 44, core pixels bin 69; one call that holds and owns
    the whole slide"""
    q = np.where(pos, np.where(core, 69, 44), 0)
    H, W = pos.shape
    out, flags = np.full((len(rows), sr.COLS), -1, np.int64), np.zeros(1, np.int64)
    sr.add_classes(np.ones_like(pos), q, 0, 0, H, W, (0, H), sr.THRES_BIN, sr.CORE_BIN, margin, min_area, rows, out, flags)
    return out, int(flags[0])


def test_the_colours_of_the_gpu_tests_have_the_bins_the_issue_states():
    px = np.asarray([[sr.POSITIVE, sr.CORE, sr.NEGATIVE, sr.GLASS]], np.uint8)
    t, q = lr.classes(px, 1, sr.BG, sref.tables(), 1)
    assert t.tolist() == [[True, True, True, False]] and q[0, :3].tolist() == [44, 69, 0]
    assert lr.thres_bin(0.15) == sr.THRES_BIN and lr.thres_bin(1.0) == sr.CORE_BIN
    t2, q2 = lr.classes(sr.paint(np.asarray([[True, False]]), np.asarray([[True, False]]), None, 2), 2, sr.BG, sref.tables(), 1)
    assert q2.tolist() == [[69, 0]] and t2.all()                     # 2x2 blocks of one colour: the means are the colour


def test_the_rule_on_hand_worked_shapes():
    pos, core, rows, names = sr.hand_slide()
    out, flags = run(pos, core, rows, sr.HAND_MARGIN)
    got = {n: o.tolist() for n, o in zip(names, out)}
    # status, window, positives, candidates, area, core, bin_sum, perimeter, sum_x, sum_y, tight box, sides, in_box, 0
    assert got["one pixel"] == [0, 17, 1, 9, 9, 1, 1, 1, 0, 44, 4, 4, 4, 21, 5, 22, 6, 0, 1, 0]
    assert got["2x2"][5:11] == [4, 1, 4, 1, 3 * 44 + 69, 8] and got["2x2"][13:17] == [37, 5, 39, 7]
    assert got["diagonal pair"][5:11] == [2, 1, 2, 0, 88, 8]         # ONE component: 8-connectivity
    assert got["L"][5:11] == [7, 1, 7, 0, 7 * 44, 16]
    assert got["ring"][5:11] == [16, 1, 16, 2, 14 * 44 + 2 * 69, 20 + 12] and got["ring"][13:17] == [21, 20, 26, 25]
    assert got["tie"][5:8] == [8, 2, 4] and got["tie"][13:17] == [37, 21, 39, 23]     # the first in raster order
    assert got["only in the margin"][5:] == [4, 0] + [0] * 13        # positive pixels in the window, but no candidate
    assert got["one pixel in the box"][5:8] == [7, 1, 7] and got["one pixel in the box"][18] == 1
    assert got["top-left corner"][:8] == [0, 0, 0, 9, 9, 9, 1, 9] and got["top-left corner"][17] == 3
    assert got["top-right corner"][:5] == [0, 87, 0, 9, 8] and got["top-right corner"][17] == 2 | 4
    assert got["bottom-left corner"][:5] == [0, 0, 56, 8, 8] and got["bottom-left corner"][17] == 1 | 8
    assert got["bottom-right corner"][:5] == [0, 88, 56, 8, 8] and got["bottom-right corner"][17] == 4 | 8
    assert got["bottom-right corner"][7:9] == [16, 4]
    assert got["two sizes"][5:8] == [26, 3, 16] and got["two sizes"][13:17] == [25, 37, 29, 41]
    assert got["nothing"][0] == 0 and got["nothing"][5:] == [0] * 15
    assert got["not finite"] == [sr.NONFINITE] + [0] * 19 and got["inverted"] == [sr.EMPTY] + [0] * 19
    assert flags == sr.NONFINITE | sr.EMPTY
    # min_area removes candidates: the single pixels and the 3x3 block
    big, _ = run(pos, core, rows, sr.HAND_MARGIN, min_area=10)
    assert big[names.index("two sizes"), 5:8].tolist() == [26, 1, 16] and big[names.index("one pixel"), 5:8].tolist() == [1, 0, 0]
    assert (big[names.index("one pixel"), 7:] == 0).all()
    # margin 0: the window is the box, and what lies outside it connects nothing
    m0, _ = run(pos, core, rows, 0)
    k = names.index("one pixel in the box")
    assert m0[k, 1:5].tolist() == [68, 20, 4, 4] and m0[k, 5:8].tolist() == [1, 1, 1] and m0[k, 17] == 4
    assert m0[names.index("only in the margin"), 5] == 0


def test_statuses_windows_and_the_large_flag():
    pos = np.ones((300, 300), bool)
    rows = np.asarray([sr.row(10, 10, 249, 249), sr.row(10, 10, 250, 249), sr.row(10, 10, 249, 250), sr.row(0, 0, 300, 300),
                       sr.row(INF, 0, 5, 5), sr.row(5, 5, 5, 9), sr.row(-50, -50, -10, -10)], np.float32)
    out, flags = run(pos, 0 * pos > 0, rows, 8)
    assert out[0, :8].tolist() == [0, 2, 2, 255, 255, 65025, 1, 65025] and out[0, 10] == 1020 and out[0, 17] == 15
    assert out[1, :5].tolist() == [sr.LARGE, 2, 2, 256, 255] and out[2, :5].tolist() == [sr.LARGE, 2, 2, 255, 256]
    assert out[3, :5].tolist() == [sr.LARGE, 0, 0, 300, 300] and (out[1:4, 5:] == 0).all()
    assert out[4].tolist() == [sr.NONFINITE] + [0] * 19 and out[5].tolist() == [sr.EMPTY] + [0] * 19 and out[6, 0] == sr.EMPTY
    assert flags == sr.LARGE | sr.NONFINITE | sr.EMPTY


def test_any_partition_of_the_owner_rows_gives_the_bytes_of_one_call():
    raster, tie = sr.blob_raster(400, 90, 5)
    t, q = lr.classes(raster, 1, sr.BG, sref.tables(), 1)
    rows = np.concatenate([tie, lr.random_boxes(80, 400, 90, 3, cuts=(100, 101, 250)), np.asarray([sr.row(NAN, 0, 1, 1), sr.row(3, 3, 3, 3)], np.float32)])
    M, margin = len(rows), 6

    def call(region, own, out, flags):
        sr.add_classes(t[region[0]:region[1]], q[region[0]:region[1]], region[0], 0, 400, 90, own, sr.THRES_BIN, sr.CORE_BIN, margin, 1, rows, out, flags)

    want, want_f = np.full((M, sr.COLS), -1, np.int64), np.zeros(1, np.int64)
    call((0, 400), (0, 400), want, want_f)
    assert (want != -1).all() and (want[:, 7] > 0).sum() >= 30
    _, _, win, owner = sr.windows(rows, 400, 90, margin)
    for cuts in ((100,), (1, 100, 101, 399), tuple(range(25, 400, 25))):
        bounds = [0, *cuts, 400]
        got, got_f = np.full((M, sr.COLS), -1, np.int64), np.zeros(1, np.int64)
        for a, b in zip(bounds[:-1], bounds[1:]):
            mine = (owner >= a) & (owner < b)
            lo, hi = (int(win[mine, 1].min()), int((win[mine, 1] + win[mine, 3]).max())) if mine.any() else (a, a + 1)
            call((min(lo, a), max(hi, a + 1)), (a, b), got, got_f)    # a region that just holds the owned windows
        assert got.tobytes() == want.tobytes() and got_f[0] == want_f[0], cuts
    # a region one row short: NOT_RESIDENT for exactly the rows whose window needs that row
    got, got_f = np.full((M, sr.COLS), -1, np.int64), np.zeros(1, np.int64)
    call((0, 250), (0, 400), got, got_f)
    needs = (want[:, 0] == 0) & (win[:, 1] + win[:, 3] > 250)
    assert needs.sum() >= 5 and (got[needs, 0] == sr.NOT_RESIDENT).all() and (got[needs, 5:] == 0).all()
    assert np.array_equal(got[needs, 1:5], win[needs]) and np.array_equal(got[~needs], want[~needs])
    assert got_f[0] == want_f[0] | sr.NOT_RESIDENT
    # the strip plan of wsi.segment_boxes, restated: every window lies wholly in the strip that owns it, for every H and strip height
    for H in (1, 254, 255, 256, 300, 509, 510, 1000):
        for strip in (255, 256, 300, 2048):
            plan = sr.strip_plan(H, strip)
            assert plan[0][2] == 0 and plan[-1][3] == H and all(p[3] == n[2] for p, n in zip(plan[:-1], plan[1:]))
            for y0, y1, a, b in plan:
                assert y0 <= a < b and 0 <= y0 < y1 <= H and min(b - 1 + sr.MAX_SIDE, H) <= y1


def test_the_flood_fill_against_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(2)
    for k in range(40):
        mask = rng.random(tuple(rng.integers(1, 60, 2))) < (0.2, 0.45, 0.6, 0.8)[k % 4]
        lab, n = sr.components(mask)
        ref, n_ref = ndimage.label(mask, structure=np.ones((3, 3), int))
        assert n == n_ref and sorted(np.bincount(lab.ravel())[1:]) == sorted(np.bincount(ref.ravel())[1:])
        assert len(set(zip(lab[mask].tolist(), ref[mask].tolist()))) == n            # the same partition


def test_plaque_morphometry_on_hand_made_words():
    seg = np.zeros((5, sr.COLS), np.int32)
    # a 4x4 square at (10, 20) .. (14, 24) in a window at (2, 12) of 20 x 20: area 16, 4 core, bins 16 * 44, perimeter 16
    seg[0] = [0, 2, 12, 20, 20, 30, 2, 16, 4, 16 * 44, 16, 16 * 8 + 6 * 4, 16 * 8 + 6 * 4, 10, 20, 14, 24, 0, 12, 0]
    seg[1] = [0, 0, 0, 9, 9, 9, 1, 9, 0, 9 * 100, 12, 9, 9, 0, 0, 3, 3, 3, 9, 0]       # touches the window's first column and row
    seg[2] = [0, 5, 5, 10, 10, 7, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]            # nothing selected
    seg[3] = [sr.LARGE, 5, 5, 300, 10] + [0] * 15
    seg[4] = [0, 90, 40, 10, 8, 3, 1, 3, 3, 3 * 69, 8, 27, 21, 99, 47, 100, 48, 4 | 8, 1, 0]
    got = wsi.plaque_morphometry(seg)
    assert got["area_px"][:2].tolist() == [16.0, 9.0] and np.isnan(got["area_px"][2:4]).all()
    assert got["core_fraction"][0] == 0.25 and got["mean_od"][0] == 44.5 / 64 and got["compactness"][0] == 1.0
    assert got["centroid_x"][0] == 2 + 9.5 + 0.5 == 12.0 and got["centroid_y"][0] == 22.0
    assert got["tight_box"][0].tolist() == [10, 20, 14, 24] and got["outside_fraction"][0] == 0.25 and got["candidates"][0] == 2
    assert got["truncated"].tolist() == [False, True, False, False, True] and got["truncated"].dtype == np.bool_
    assert wsi.plaque_morphometry(seg, slide_hw=(48, 100))["truncated"].tolist() == [False, False, False, False, False]
    assert wsi.plaque_morphometry(seg, slide_hw=(50, 100))["truncated"].tolist() == [False, False, False, False, True]
    with_mpp = wsi.plaque_morphometry(seg, mpp=0.5, slide_hw=(48, 100))
    assert with_mpp["area_um2"][0] == 4.0 and with_mpp["equiv_diameter_um"][0] == 2.0 * math.sqrt(4.0 / math.pi)
    assert sorted(set(with_mpp) - set(got)) == ["area_um2", "equiv_diameter_um"]
    for hw, mpp in ((None, None), ((48, 100), 0.5)):
        want, have = sr.morphometry(seg, mpp, hw), wsi.plaque_morphometry(seg, mpp, hw)
        assert sorted(want) == sorted(have)
        for k in want:
            np.testing.assert_array_equal(np.asarray(have[k], np.float64), np.asarray(want[k], np.float64), err_msg=k)
    for k, v in got.items():
        assert len(v) == 5 and (k == "truncated" or np.isnan(v[2:4]).all()), k
    for bad in (np.zeros((3, 19), np.int32), np.zeros(20, np.int32), np.zeros((3, 20), np.float32)):
        with pytest.raises(ValueError):
            wsi.plaque_morphometry(bad)
    for mpp in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError):
            wsi.plaque_morphometry(seg, mpp=mpp)
    assert "NOT A EUCLIDEAN CIRCULARITY" in " ".join(wsi.plaque_morphometry.__doc__.split())


# ---- the inputs of the GPU tests: the counts they promise, on the reference alone ----------------------------------------------------------
def test_the_worst_windows_are_what_their_names_say():
    pos, rows = sr.worst_slide()
    out, flags = run(pos, 0 * pos > 0, rows, sr.WORST_MARGIN)
    got = dict(zip(sr.WORST, out.tolist()))
    assert all(got[k][:5] == [0, i * 255, 0, 255, 255] for i, k in enumerate(sr.WORST)) and flags == sr.LARGE
    assert got["full"][5:8] == [65025, 1, 65025] and got["full"][10] == 1020
    assert got["checkerboard"][5:8] == [32513, 1, 32513]                             # ONE component
    assert got["every other"][5:8] == [16384, 28 * 28, 1] and got["every other"][13:17] == [2 * 255 + 100, 100, 2 * 255 + 101, 101]
    for k in ("spiral", "serpentine", "comb"):
        assert got[k][5:8] == [32767, 1, 32767], k
    assert got["diagonal"][5:8] == [255, 1, 255] and got["diagonal"][10] == 1020
    assert got["two equal blobs"][5:8] == [200, 2, 100] and got["two equal blobs"][14] == 110
    assert got["empty"][5:] == [0] * 15 and out[-1, :5].tolist() == [sr.LARGE, 0, 0, 256, 255]


@pytest.mark.parametrize("shrink", [1, 2])
def test_the_random_inputs_show_what_the_gpu_test_promises(shrink):
    from test_gpu_load import hand_rows
    raster, rows, short = sr.random_case(shrink, hand_rows(300, 260))
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    want, flags = sr.segment(raster, shrink, sr.BG, sref.tables(), 1, sr.THRES_BIN, sr.CORE_BIN, sr.RANDOM_MARGIN, 1, rows)
    sr.assert_random_counts(want, flags)
    # a region deliberately short
    got, f = sr.segment(raster, shrink, sr.BG, sref.tables(), 1, sr.THRES_BIN, sr.CORE_BIN, sr.RANDOM_MARGIN, 1, rows, plan=[(0, short, 0, H)])
    assert (got[:, 0] == sr.NOT_RESIDENT).sum() >= 1 and f[0] & sr.NOT_RESIDENT


# ---- host argument checks: no device is touched ---------------------------------------------------------------------------------------------
def test_segment_boxes_rejects_bad_arguments_before_any_launch():
    r = np.full((64, 96, 3), 255, np.uint8)
    rows = np.zeros((2, 7), np.float32)
    for kw in (dict(margin=-1), dict(margin=128), dict(margin=8.0), dict(margin=True), dict(shrink=3), dict(shrink=0), dict(bg_level=-1),
               dict(bg_level=257), dict(bg_level=2.5), dict(thres=-0.1), dict(thres=NAN), dict(thres=INF), dict(thres="x"),
               dict(core_thres=-1.0), dict(core_thres=NAN), dict(core_thres=0.1), dict(thres=1.0, core_thres=0.5), dict(stain=2),
               dict(stain=-1), dict(stain=True), dict(basis=None), dict(basis="H_DAB"), dict(min_area=0), dict(min_area=1.5),
               dict(min_area=True), dict(strip=254), dict(strip=0), dict(strip=300.0), dict(strip=True)):
        with pytest.raises(ValueError):
            wsi.segment_boxes(r, rows, **kw)
    for bad_rows in (None, np.zeros((2, 6), np.float32), np.zeros(7, np.float32), [1, 2, 3]):
        with pytest.raises(ValueError):
            wsi.segment_boxes(r, bad_rows)
    for bad in (np.zeros((64, 96), np.uint8), np.zeros((64, 96, 4), np.uint8), np.zeros((64, 96, 3), np.float32), np.zeros((0, 96, 3), np.uint8)):
        with pytest.raises(ValueError):
            wsi.segment_boxes(bad, rows)
    with pytest.raises(ValueError):
        wsi.segment_boxes(np.zeros((1, 96, 3), np.uint8), rows, shrink=2)            # no halved pixel
    big = np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), ((1 << 24) + 1, 1, 3), (0, 0, 1))      # no memory is touched
    with pytest.raises(ValueError):
        wsi.segment_boxes(big, rows)
    # no rows: empty arrays without a launch (and without a device)
    got = wsi.segment_boxes(r, np.zeros((0, 7), np.float32), thres=0.15, core_thres=1.0, strip=255)
    assert got["segments"].shape == (0, 20) and got["segments"].dtype == np.int32 and got["flags"] == 0
    assert got["thres"] == 10 / 64 and got["core_thres"] == 1.0 and got["strips"] == (0, 1)
    assert wsi.segment_boxes(np.zeros((1000, 4, 3), np.uint8), np.zeros((0, 7), np.float32), strip=300)["strips"] == (0, 17)
    assert len(sr.strip_plan(1000, 300)) == 17


def test_the_owner_rows_of_the_host_are_the_rule_s():
    rows = np.concatenate([lr.random_boxes(300, 500, 200, 8), np.asarray([sr.row(NAN, 0, 1, 1), sr.row(3, 3, 3, 3), sr.row(0, 499.5, 9, INF)], np.float32)])
    for margin in (0, 8, 127):
        assert np.array_equal(wsi._segment_owner_rows(rows, 500, 200, margin), sr.windows(rows, 500, 200, margin)[3])


def test_quantify_region_with_segment_rejects_bad_arguments_before_any_launch():
    r = np.full((64, 96, 3), 255, np.uint8)
    for kw in (dict(), dict(dab_thres=-1.0), dict(dab_thres=0.15, seg_margin=128), dict(dab_thres=0.15, seg_margin=-1),
               dict(dab_thres=0.15, core_thres=0.1), dict(dab_thres=0.15, core_thres=NAN), dict(dab_thres=0.15, min_area=0),
               dict(dab_thres=0.15, min_area=2.5), dict(dab_thres=0.15, bg_level=300), dict(dab_thres=0.15, shrink=3)):
        with pytest.raises(ValueError):
            wsi.quantify_region(None, r, segment=True, **kw)          # no model is touched before the checks
    for kw in (dict(seg_margin=8), dict(core_thres=1.0), dict(min_area=1)):   # the arguments of the pass without the pass
        with pytest.raises(ValueError):
            wsi.quantify_region(None, r, dab_thres=0.15, load=True, **kw)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry_point():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "amyloid_yolo.h")) as f:
        header = f.read()
    assert "#define AY_ABI_VERSION 2\n" in header and "int ay_box_segments_u8(" in header and "THE SEGMENT RULE" in header
    for name, value in (("COLS", sr.COLS), ("MAX_SIDE", sr.MAX_SIDE), ("MAX_MARGIN", sr.MAX_MARGIN), ("NONFINITE", sr.NONFINITE),
                        ("EMPTY", sr.EMPTY), ("LARGE", sr.LARGE), ("NOT_RESIDENT", sr.NOT_RESIDENT), ("INTERNAL", sr.INTERNAL)):
        assert f"#define AY_SEG_{name} {value}\n" in header and getattr(wsi, f"SEG_{name}") == value, name
    proto = header[header.index("int ay_box_segments_u8("):]
    proto = proto[:proto.index(");")]
    assert len(re.sub(r"/\*.*?\*/", "", proto).split(",")) == 23
    res, args = _lib._SIGS["ay_box_segments_u8"]
    assert res is C.c_int and len(args) == 23 and args[3] is C.c_size_t and "ay_box_segments_u8" in _lib.exported_symbols()
    assert _lib.ABI_VERSION == 2
