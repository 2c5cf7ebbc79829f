"""CPU: the restatement of THE LOAD RULE (tests/load_reference.py) against the stain and tissue restatements and on hand-worked boxes,
wsi.box_morphometry, and the argument checks of wsi.stain_load / quantify_region(load=True), which raise before any device work."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import load_reference as lr
import stain_reference as sref
import tissue_reference as tr
from amyloid_yolo_paper_amd import _lib, wsi
from test_gpu_tissue import dark_and_bright

NAN, INF = float("nan"), float("inf")
BG = 170
# (shrink, thres_bin) -> (tissue, positive) of dark_and_bright(5, 97, 131) at bg 170, counted once on the CPU when the cases were chosen
KNOWN = {(1, 10): (8127, 4545), (1, 40): (8127, 2245), (2, 10): (2572, 1477), (2, 40): (2572, 54)}


@pytest.fixture(scope="module")
def raster():
    return dark_and_bright(5, 97, 131)


def row(x1, y1, x2, y2):
    return [x1, y1, x2, y2, 0.9, 0.9, 0.0]


# ---- the cells ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink,j", sorted(KNOWN))
def test_cell_sums_against_the_histogram_and_the_tissue_map(raster, shrink, j):
    t = sref.tables()
    h = sref.hist(raster, shrink, BG, t)
    for cell in (16, 24, 37, 128):
        cells, _, _ = lr.load(raster, shrink, BG, t, 1, j, cell)
        H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
        assert cells.shape == wsi.tile_grid(H, W, cell, 0)[:2] + (3,)
        tissue, positive = int(cells[:, :, 0].sum()), int(cells[:, :, 1].sum())
        assert (tissue, positive) == KNOWN[(shrink, j)] and 0 < positive < tissue
        assert positive == h[512 + j:1024].sum()                                    # the histogram's tail
        assert tissue == h[1024] == int(tr.tissue(raster, shrink, BG).sum())
        np.testing.assert_array_equal(cells[:, :, 0], tr.tissue_counts(raster, cell, shrink, 0, BG))
        assert (cells[:, :, 1] <= cells[:, :, 0]).all() and (cells[:, :, 2] >= j * cells[:, :, 1]).all()
        assert (cells[:, :, 2] <= 511 * cells[:, :, 1]).all()
    # the other stain: the same tissue, the other histogram
    c0, _, _ = lr.load(raster, shrink, BG, t, 0, j, 24)
    assert c0[:, :, 1].sum() == h[j:512].sum() and c0[:, :, 0].sum() == h[1024]
    # 512 makes nothing positive, 0 every tissue pixel
    none, _, _ = lr.load(raster, shrink, BG, t, 1, 512, 24)
    every, _, _ = lr.load(raster, shrink, BG, t, 1, 0, 24)
    assert none[:, :, 1:].sum() == 0 and np.array_equal(every[:, :, 1], every[:, :, 0])


@pytest.mark.parametrize("shrink", [1, 2])
def test_three_uneven_strips_give_what_the_whole_image_gives(raster, shrink):
    t = sref.tables()
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    rows = np.concatenate([lr.random_boxes(60, H, W, 3, cuts=(13, 14)), np.asarray([row(0, 0, W, H), row(3.2, 12.6, 40.0, 14.4)], np.float32)])
    for j in (10, 40):
        whole = lr.load(raster, shrink, BG, t, 1, j, 24, rows)
        strips = lr.load(raster, shrink, BG, t, 1, j, 24, rows, cuts=(13, 14))
        for a, b in zip(whole, strips):
            assert a.tobytes() == b.tobytes()
        assert 0 < whole[1][:, 2].sum() < whole[1][:, 1].sum()
        np.testing.assert_array_equal(whole[1][:, 0], lr.owned_pixels(rows, H, W))
        np.testing.assert_array_equal(whole[1][-2], [W * H, whole[0][:, :, 0].sum(), whole[0][:, :, 1].sum(), whole[0][:, :, 2].sum()])


# ---- the boxes ----------------------------------------------------------------------------------------------------------------------------
def test_box_rule_on_hand_worked_rows(raster):
    H, W = raster.shape[:2]
    t = sref.tables()
    rows = np.asarray([row(10.5, 10.5, 11.5, 11.5),          # 0: exactly pixel (10, 10)
                       row(10.5, 10.5, 10.5, 30.0),          # 1: empty in x
                       row(0.0, 0.0, W, H),                  # 2: the slide
                       row(-7.3, -1e9, 4.5, 2.49),           # 3: clamped at the top left: X 0..3, Y 0..1
                       row(W - 2.5, H - 1.5, 1e9, 3e38),     # 4: clamped at the bottom right: 3 columns, 2 rows
                       row(30.0, 40.0, 20.0, 50.0),          # 5: inverted in x
                       row(20.0, 50.0, 30.0, 40.0),          # 6: inverted in y
                       row(NAN, 1.0, 5.0, 5.0),              # 7
                       row(1.0, 1.0, INF, 5.0),              # 8
                       row(1.0, -INF, 5.0, 5.0),             # 9
                       row(10.49, 10.51, 11.51, 11.49),      # 10: centres 10.5 and 11.5 in x, none in y
                       row(W + 5.0, 3.0, W + 9.0, 8.0)],     # 11: beyond the slide
                      np.float32)
    finite, e = lr.edges(rows, H, W)
    assert finite.tolist() == [True] * 7 + [False] * 3 + [True] * 2
    assert e[0].tolist() == [10, 10, 11, 11] and e[1].tolist() == [10, 10, 10, 30] and e[2].tolist() == [0, 0, W, H]
    assert e[3].tolist() == [0, 0, 4, 2] and e[4].tolist() == [W - 3, H - 2, W, H]
    assert e[10].tolist() == [10, 11, 12, 11] and e[11].tolist() == [W, 3, W, 8]
    cells, boxes, flags = lr.load(raster, 1, 256, t, 1, 0, 16, rows)           # bg 256, threshold 0: every pixel tissue and positive
    assert boxes[:, 0].tolist() == [1, 0, W * H, 8, 6, 0, 0, 0, 0, 0, 0, 0] and flags[0] == lr.FLAG_NONFINITE
    np.testing.assert_array_equal(boxes[:, 0], lr.owned_pixels(rows, H, W))
    assert np.array_equal(boxes[:, 1], boxes[:, 0]) and np.array_equal(boxes[:, 2], boxes[:, 0])
    q = lr.classes(raster, 1, 256, t, 1)[1]
    assert boxes[0, 3] == q[10, 10] and boxes[3, 3] == q[0:2, 0:4].sum() and boxes[2, 3] == q.sum() == cells[:, :, 2].sum()
    assert (boxes[7:10] == 0).all()
    _, clean, no_flags = lr.load(raster, 1, 256, t, 1, 0, 16, rows[:7])
    assert no_flags[0] == 0 and np.array_equal(clean, boxes[:7])               # boxes are independent of each other
    # overlapping boxes each count their own pixels
    two = np.asarray([row(5, 5, 25, 25), row(5, 5, 25, 25), row(15, 15, 35, 35)], np.float32)
    _, b2, _ = lr.load(raster, 1, BG, t, 1, 10, 16, two)
    assert np.array_equal(b2[0], b2[1]) and b2[0, 0] == 400 == b2[2, 0] and 0 < b2[0, 2] < b2[0, 1] < 400


# ---- wsi.box_morphometry ---------------------------------------------------------------------------------------------------------------------
def test_box_morphometry_on_hand_made_counts():
    boxes = np.asarray([[100, 80, 50, 50 * 20], [100, 80, 0, 0], [0, 0, 0, 0], [4, 4, 4, 4 * 511], [9, 0, 0, 0]], np.int64)
    got = wsi.box_morphometry(boxes)
    assert sorted(got) == ["area_px", "fill", "mean_od"]
    np.testing.assert_array_equal(got["area_px"], [50.0, NAN, NAN, 4.0, NAN])
    np.testing.assert_array_equal(got["fill"], [0.5, 0.0, NAN, 1.0, 0.0])
    np.testing.assert_array_equal(got["mean_od"], [20.5 / 64, NAN, NAN, 511.5 / 64, NAN])       # bin 511 saturates at 8 OD
    got = wsi.box_morphometry(boxes, mpp=0.5)
    assert sorted(got) == ["area_px", "area_um2", "equiv_diameter_um", "fill", "mean_od"]
    np.testing.assert_array_equal(got["area_um2"], [12.5, NAN, NAN, 1.0, NAN])
    np.testing.assert_array_equal(got["equiv_diameter_um"], [2 * math.sqrt(12.5 / math.pi), NAN, NAN, 2 * math.sqrt(1.0 / math.pi), NAN])
    want = lr.morphometry(boxes, 0.5)
    for k in got:
        assert got[k].dtype == np.float64
        np.testing.assert_allclose(got[k], want[k], rtol=1e-15, atol=0)
    assert wsi.box_morphometry(np.zeros((0, 4), np.int64), 0.25)["fill"].shape == (0,)
    for bad in (np.zeros((3, 3), np.int64), np.zeros(4, np.int64), np.zeros((2, 4), np.float32), -np.ones((1, 4), np.int64)):
        with pytest.raises(ValueError):
            wsi.box_morphometry(bad)
    for mpp in (0.0, -1.0, NAN, INF):
        with pytest.raises(ValueError):
            wsi.box_morphometry(boxes, mpp)


# ---- host argument checks: no device is touched ------------------------------------------------------------------------------------------------
def test_stain_load_rejects_bad_arguments_before_any_launch():
    r = np.full((64, 96, 3), 255, np.uint8)
    rows = np.zeros((2, 7), np.float32)
    for kw in (dict(cell=15), dict(cell=0), dict(cell=16.0), dict(cell=True), dict(shrink=3), dict(shrink=0), dict(bg_level=-1),
               dict(bg_level=257), dict(thres=-0.1), dict(thres=NAN), dict(thres=INF), dict(thres="high"), dict(stain=2), dict(stain=-1),
               dict(stain=True), dict(basis="H_DAB"), dict(rows=np.zeros((2, 6), np.float32)), dict(rows=np.zeros(7, np.float32)),
               dict(rows=[1, 2, 3])):
        with pytest.raises(ValueError):
            wsi.stain_load(r, **kw)
    for bad in (np.zeros((64, 96), np.uint8), np.zeros((64, 96, 4), np.uint8), np.zeros((64, 96, 3), np.float32), np.zeros((0, 96, 3), np.uint8)):
        with pytest.raises(ValueError):
            wsi.stain_load(bad, rows)
    with pytest.raises(ValueError):
        wsi.stain_load(np.zeros((1, 96, 3), np.uint8), shrink=2)                     # no halved pixel
    with pytest.raises(ValueError):                                                # more than 2^24 pixels per side (no memory is touched)
        wsi.stain_load(np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), ((1 << 24) + 1, 1, 3), (0, 0, 1)))


def test_quantify_region_with_load_rejects_bad_arguments_before_any_launch():
    r = np.full((64, 96, 3), 255, np.uint8)
    for kw in (dict(), dict(dab_thres=-1.0), dict(dab_thres=NAN), dict(dab_thres=0.15, cell=8, probe_stride=8),
               dict(dab_thres=0.15, bg_level=300), dict(dab_thres=0.15, shrink=3), dict(dab_thres=0.15, stain_stats="stats")):
        with pytest.raises(ValueError):
            wsi.quantify_region(None, r, load=True, **kw)              # no model is touched before the checks
    with pytest.raises(ValueError):                                    # without load the two arguments still go together
        wsi.quantify_region(None, r, dab_thres=0.15)


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry_point():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "amyloid_yolo.h")) as f:
        header = f.read()
    assert "#define AY_ABI_VERSION 2\n" in header and "int ay_stain_load_u8(" in header
    assert f"#define AY_LOAD_MIN_CELL {lr.MIN_CELL}\n" in header and wsi.LOAD_MIN_CELL == lr.MIN_CELL
    assert f"#define AY_LOAD_FLAG_NONFINITE {lr.FLAG_NONFINITE}\n" in header and wsi.LOAD_FLAG_NONFINITE == lr.FLAG_NONFINITE
    res, args = _lib._SIGS["ay_stain_load_u8"]
    assert res is C.c_int and len(args) == 20 and args[3] is C.c_size_t and "ay_stain_load_u8" in _lib.exported_symbols()
    assert lr.thres_bin(0.15) == 10 and lr.thres_bin(100.0) == 512 and wsi._thres_bin(0.15, "") == 10 and wsi._thres_bin(9.0, "") == 512
