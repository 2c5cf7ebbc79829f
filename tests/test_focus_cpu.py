"""CPU: the restatement of THE FOCUS RULE (tests/focus_reference.py) on hand-worked cases and on its invariants, wsi.focus_summary, and
the argument checks of wsi.focus_map / quantify_region(focus=True), which raise before any device work."""
import ctypes as C
import itertools
import math
import os
import re

import numpy as np
import pytest

import focus_reference as fr
from amyloid_yolo_paper_amd import _lib, wsi

NAN, INF = float("nan"), float("inf")


def grey(values):
    return np.repeat(np.asarray(values, np.uint8)[:, :, None], 3, 2)


def row(x1, y1, x2, y2):
    return [x1, y1, x2, y2, 0.9, 0.9, 0.0]


# ---- the rule on hand-worked images ---------------------------------------------------------------------------------------------------------
def test_luma_by_hand():
    px = np.asarray([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [0, 0, 0], [90, 90, 90]]], np.uint8)
    # (77 * 255 + 128) >> 8 = 19763 >> 8; (150 * 255 + 128) >> 8 = 38378 >> 8; (29 * 255 + 128) >> 8 = 7523 >> 8; a grey pixel keeps its value
    assert fr.luma(px).tolist() == [[77, 149, 29, 255, 0, 90]]


def test_five_by_five_by_hand():
    flat = np.full((5, 5), 100)
    # 1. no texture: nine evaluated pixels, every Laplacian 0
    c, _, _ = fr.focus(grey(flat), 1, 220, 16)
    assert c.shape == (1, 1, 3) and c[0, 0].tolist() == [9, 0, 0]
    # 2. one pixel 10 brighter in the middle: +40 there, -10 at its four neighbours, 0 at the corners of the inner 3 x 3
    bump = flat.copy()
    bump[2, 2] = 110
    ev, lap = fr.evaluate(grey(bump), 1, 220)
    assert ev.sum() == 9 and not ev[0].any() and not ev[:, 0].any() and not ev[4].any() and not ev[:, 4].any()
    assert lap[1:4, 1:4].tolist() == [[0, -10, 0], [-10, 40, -10], [0, -10, 0]]
    c, _, _ = fr.focus(grey(bump), 1, 220, 16)
    assert c[0, 0].tolist() == [9, 0, 1600 + 4 * 100]
    assert fr.sharpness(*c[0, 0])[()] == 2000 / 9
    # 3. a glass pixel in the middle removes exactly itself and its four neighbours: the corners of the inner 3 x 3 stay, and (1, 1)
    #    sees the 120 above it: 400 - 120 - 300
    glass = flat.copy()
    glass[2, 2], glass[0, 1] = 255, 120
    ev, lap = fr.evaluate(grey(glass), 1, 220)
    assert np.argwhere(ev).tolist() == [[1, 1], [1, 3], [3, 1], [3, 3]]
    c, _, _ = fr.focus(grey(glass), 1, 220, 16)
    assert c[0, 0].tolist() == [4, -20, 400]
    # at bg_level 256 the same pixel is tissue: nine pixels again, and its 255 is texture
    ev, lap = fr.evaluate(grey(glass), 1, 256)
    assert ev.sum() == 9 and lap[2, 2] == 4 * 255 - 400 and lap[1, 2] == 400 - 255 - 300
    # at bg_level 0 nothing is tissue
    assert fr.focus(grey(glass), 1, 0, 16)[0].sum() == 0
    # 4. boxes: THE LOAD RULE's ownership of the evaluated pixels
    rows = np.asarray([row(0, 0, 5, 5), row(2.5, 2.5, 3.5, 3.5), row(3.5, 0.0, 4.5, 5.0), row(NAN, 0, 5, 5), row(3, 3, 1, 1)], np.float32)
    _, b, f = fr.focus(grey(bump), 1, 220, 16, rows)
    assert b.tolist() == [[9, 0, 2000], [1, 40, 1600], [3, -10, 100], [0, 0, 0], [0, 0, 0]] and f[0] == fr.FLAG_NONFINITE
    # 5. too small to hold an evaluated pixel
    for shape in ((2, 9), (9, 2), (1, 1)):
        c, b, f = fr.focus(grey(np.full(shape, 100)), 1, 256, 16, rows)
        assert c.sum() == 0 and b.sum() == 0 and f[0] == 0
    # 6. shrink 2: the 2 x 2 round-half-up means of a 10 x 10 raster are the 5 x 5 image (the odd 11th row and column are dropped)
    big = np.zeros((11, 11), np.int64)
    big[:10, :10] = np.kron(bump, np.ones((2, 2), np.int64))
    big[4, 4] += 2                                            # (110 * 3 + 112 + 2) >> 2 == 111
    c, _, _ = fr.focus(grey(big), 2, 220, 16)
    assert c[0, 0].tolist() == [9, 0, 44 * 44 + 4 * 121]


def test_any_split_of_the_rows_gives_the_whole_image():
    r = fr.glass_blobs(fr.texture(23, 37, 1), 2, n=4, radius=(2, 5))
    rows = np.concatenate([fr.lr.random_boxes(40, 23, 37, 3, cuts=(7, 16)), np.asarray([row(0, 0, 37, 23), row(INF, 0, 1, 1)], np.float32)])
    for shrink in (1, 2):
        H = 23 // shrink
        whole = fr.focus(r, shrink, 220, 16, rows)
        assert 0 < whole[0][:, :, 0].sum() < (H - 2) * (37 // shrink - 2) and whole[2][0] == 1
        assert whole[1][-2].tolist() == whole[0].sum((0, 1)).tolist()             # the box that is the slide
        for cuts in itertools.chain(itertools.combinations(range(0, H + 1), 1), [(1, 2), (2, 3, 4, H - 2), tuple(range(H + 1))]):
            bounds = [0, *cuts, H]
            parts = fr.focus(r, shrink, 220, 16, rows, strips=list(zip(bounds[:-1], bounds[1:])))
            for a, b in zip(whole, parts):
                assert a.tobytes() == b.tobytes(), (shrink, cuts)
        # a range that owns nothing adds nothing
        assert fr.focus(r, shrink, 220, 16, rows, strips=[(0, 1), (H - 1, H), (5, 5)])[0].sum() == 0


def test_cells_own_their_pixels_and_read_their_neighbours_across_the_border():
    r = fr.texture(40, 50, 5)
    ev, lap = fr.evaluate(r, 1, 256)
    c, _, _ = fr.focus(r, 1, 256, 16)
    assert c.shape == (3, 4, 3) and c[:, :, 0].sum() == 38 * 48
    assert c[1, 1].tolist() == [256, lap[16:32, 16:32].sum(), (lap[16:32, 16:32] ** 2).sum()]     # an inner cell: all of its pixels
    assert c[0, 0, 0] == 15 * 15 and c[2, 3, 0] == 7 * 1
    assert lap[16, 16] == 4 * fr.luma(r)[16, 16] - fr.luma(r)[15, 16] - fr.luma(r)[17, 16] - fr.luma(r)[16, 15] - fr.luma(r)[16, 17]


def test_checkerboard():
    H, W = 10, 13
    c, _, _ = fr.focus(fr.checkerboard(H, W), 1, 256, 16)
    n = (H - 2) * (W - 2)
    assert n % 2 == 0 and c[0, 0].tolist() == [n, 0, 1040400 * n]
    assert fr.sharpness(*c[0, 0])[()] == 1040400.0
    assert fr.focus(fr.checkerboard(H, W), 1, 255, 16)[0].sum() == 0             # every pixel has a 255 among its five


def test_blur_lowers_the_sharpness():
    r = fr.texture(97, 131, 11)
    p = np.pad(r.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="edge")
    blurred = (sum(p[dy:dy + 97, dx:dx + 131] for dy in range(3) for dx in range(3)) // 9).astype(np.uint8)
    s, b = (fr.sharpness(*fr.focus(x, 1, 220, 256)[0][0, 0])[()] for x in (r, blurred))
    print("sharpness: texture %.1f, its 3 x 3 box blur %.1f" % (s, b))
    assert b < s                                          # a trial of the rule: about 19 300 against about 380


# ---- wsi.focus_summary ----------------------------------------------------------------------------------------------------------------------
def test_focus_summary_on_hand_made_sums():
    n = np.asarray([[100, 10, 0], [50, 40, 0]], np.int64)
    s1 = np.asarray([[0, 10, 0], [-50, 0, 0]], np.int64)
    s2 = np.asarray([[40000, 1010, 0], [5050, 40, 0]], np.int64)
    sharp = wsi._sharpness(n, s1, s2)
    np.testing.assert_array_equal(sharp, [[400.0, 100.0, NAN], [100.0, 1.0, NAN]])
    np.testing.assert_array_equal(sharp, fr.sharpness(n, s1, s2))
    f = {"n": n, "s1": s1, "s2": s2, "sharpness": sharp}
    got = wsi.focus_summary(f)
    assert sorted(got) == ["evaluated_fraction"] and math.isnan(got["evaluated_fraction"])       # no threshold: no classification
    tissue = np.asarray([[200, 50, 30], [60, 60, 0]], np.int32)
    assert wsi.focus_summary(f, tissue)["evaluated_fraction"] == 200 / 400
    got = wsi.focus_summary(f, tissue, min_sharpness=100.0)
    assert sorted(got) == ["evaluated_fraction", "in_focus", "in_focus_fraction"]
    assert got["in_focus"].dtype == np.bool_ and got["in_focus"].tolist() == [[True, True, False], [True, False, False]]
    assert got["in_focus_fraction"] == 160 / 200
    got = wsi.focus_summary(f, None, min_sharpness=100.0, min_pixels=11)
    assert got["in_focus"].tolist() == [[True, False, False], [True, False, False]] and got["in_focus_fraction"] == 150 / 200
    assert wsi.focus_summary(f, None, min_sharpness=0.0)["in_focus"].tolist() == [[True, True, False], [True, True, False]]
    empty = {"n": 0 * n, "sharpness": np.full(n.shape, NAN)}
    got = wsi.focus_summary(empty, 0 * tissue, 1.0)
    assert math.isnan(got["evaluated_fraction"]) and math.isnan(got["in_focus_fraction"]) and not got["in_focus"].any()
    for bad in (dict(min_sharpness=-1.0), dict(min_sharpness=NAN), dict(min_sharpness=INF), dict(min_sharpness=True), dict(min_pixels=0),
                dict(min_pixels=1.5), dict(tissue=np.zeros((3, 2), np.int32)), dict(tissue=np.zeros((2, 3), np.float32)),
                dict(tissue=-np.ones((2, 3), np.int32))):
        with pytest.raises(ValueError):
            wsi.focus_summary(f, **bad)
    with pytest.raises(ValueError):
        wsi.focus_summary({"n": n.astype(np.float64), "sharpness": sharp})
    doc = " ".join(wsi.focus_summary.__doc__.split())
    assert "NO DEFAULT THRESHOLD IS OFFERED" in doc and "texture of the tissue and the strength of the stain" in doc


# ---- host argument checks: no device is touched ---------------------------------------------------------------------------------------------
def test_focus_map_rejects_bad_arguments_before_any_launch():
    r = np.full((64, 96, 3), 255, np.uint8)
    rows = np.zeros((2, 7), np.float32)
    for kw in (dict(cell=15), dict(cell=0), dict(cell=16.0), dict(cell=True), dict(shrink=3), dict(shrink=0), dict(bg_level=-1),
               dict(bg_level=257), dict(bg_level=2.5), dict(strip=2), dict(strip=0), dict(strip=16.0), dict(strip=True),
               dict(rows=np.zeros((2, 6), np.float32)), dict(rows=np.zeros(7, np.float32)), dict(rows=[1, 2, 3])):
        with pytest.raises(ValueError):
            wsi.focus_map(r, **kw)
    for bad in (np.zeros((64, 96), np.uint8), np.zeros((64, 96, 4), np.uint8), np.zeros((64, 96, 3), np.float32), np.zeros((0, 96, 3), np.uint8)):
        with pytest.raises(ValueError):
            wsi.focus_map(bad, rows)
    with pytest.raises(ValueError):
        wsi.focus_map(np.zeros((1, 96, 3), np.uint8), shrink=2)                      # no halved pixel
    big = lambda h, w: np.lib.stride_tricks.as_strided(np.zeros(3, np.uint8), (h, w, 3), (0, 0, 1))      # no memory is touched
    with pytest.raises(ValueError):
        wsi.focus_map(big((1 << 24) + 1, 1))
    with pytest.raises(ValueError):
        wsi.focus_map(big(1 << 22, 1 << 21), cell=1 << 20)                           # 2^43 pixels: s2 could pass int64


def test_a_slide_without_an_evaluated_pixel_gives_zeros_without_a_launch():
    rows = np.asarray([row(0, 0, 5, 5), row(NAN, 0, 5, 5)], np.float32)
    for shape, shrink in (((2, 40, 3), 1), ((40, 2, 3), 1), ((5, 40, 3), 2), ((1, 1, 3), 1)):
        got = wsi.focus_map(np.full(shape, 90, np.uint8), rows, cell=16, shrink=shrink)
        gy, gx, _ = wsi.tile_grid(shape[0] // shrink, shape[1] // shrink, 16)
        assert sorted(got) == ["box_sharpness", "boxes", "flags", "n", "s1", "s2", "sharpness"]
        for k in ("n", "s1", "s2"):
            assert got[k].dtype == np.int64 and got[k].shape == (gy, gx) and not got[k].any()
        assert np.isnan(got["sharpness"]).all() and got["boxes"].shape == (2, 3) and not got["boxes"].any() and got["flags"] == 0
        assert np.isnan(got["box_sharpness"]).all()
        assert sorted(wsi.focus_map(np.full(shape, 90, np.uint8), cell=16, shrink=shrink)) == ["n", "s1", "s2", "sharpness"]


def test_quantify_region_with_focus_rejects_bad_arguments_before_any_launch():
    r = np.full((64, 96, 3), 255, np.uint8)
    for kw in (dict(cell=8, probe_stride=8), dict(bg_level=300), dict(shrink=3), dict(min_sharpness=-1.0), dict(min_sharpness=NAN),
               dict(min_sharpness=True)):
        with pytest.raises(ValueError):
            wsi.quantify_region(None, r, focus=True, **kw)             # no model is touched before the checks
    with pytest.raises(ValueError):                                    # a threshold without the pass
        wsi.quantify_region(None, r, min_sharpness=100.0)


# ---- the ABI --------------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_entry_point():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "amyloid_yolo.h")) as f:
        header = f.read()
    assert "#define AY_ABI_VERSION 2\n" in header and "int ay_focus_u8(" in header and "THE FOCUS RULE" in header
    assert f"#define AY_FOCUS_MIN_CELL {fr.MIN_CELL}\n" in header and wsi.FOCUS_MIN_CELL == fr.MIN_CELL
    assert f"#define AY_FOCUS_FLAG_NONFINITE {fr.FLAG_NONFINITE}\n" in header and wsi.FOCUS_FLAG_NONFINITE == fr.FLAG_NONFINITE
    proto = header[header.index("int ay_focus_u8("):]
    proto = proto[:proto.index(");")]
    assert len(re.sub(r"/\*.*?\*/", "", proto).split(",")) == 18
    res, args = _lib._SIGS["ay_focus_u8"]
    assert res is C.c_int and len(args) == 18 and args[3] is C.c_size_t and "ay_focus_u8" in _lib.exported_symbols()
