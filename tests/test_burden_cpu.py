"""CPU: the restatement of THE BURDEN RULE and THE FIELD RULE (tests/burden_reference.py) on hand cases, a second formulation of the
field sums, and the argument checks of wsi.burden_map / densest_fields / quantify_region, which raise before any device work."""
import numpy as np
import pytest

import burden_reference as br
from amyloid_yolo_paper_amd.wsi import burden_map, densest_fields, quantify_region, tile_grid

NAN, INF = float("nan"), float("inf")


def row(cx, cy, conf=0.9, cls=0, w=10.0, h=10.0):
    return [cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, conf, 0.8, cls]


# ---- THE BURDEN RULE -------------------------------------------------------------------------------------------------------------------
def test_grid_is_the_tile_grid():
    for H, W, cell in ((1000, 777, 64), (1000, 777, 1), (1000, 777, 4096), (64, 128, 64), (65, 1, 64)):
        assert br.grid(H, W, cell) == tile_grid(H, W, cell, 0)[:2]


def test_centre_on_a_cell_border_and_inside():
    rows = [row(64.0, 10.0), row(63.5, 10.0), row(63.999, 128.0), row(0.0, 0.0)]
    counts, stats = br.burden_bin(rows, 200, 300, 64, 1, 0.0)
    assert counts.shape == (1, 4, 5)
    assert counts[0, 0, 1] == 1          # cx == 64 exactly: the cell that starts there
    assert counts[0, 0, 0] == 2          # 63.5 and the origin
    assert counts[0, 2, 0] == 1          # cy == 128: row 2
    assert counts.sum() == 4 and list(stats) == [4, 0, 0, 0]


def test_centres_outside_the_slide_go_to_border_cells():
    H, W, cell = 200, 300, 64
    rows = [row(-50.0, 100.0), row(100.0, -3.0), row(1e6, 100.0), row(100.0, 199.5), row(299.9, 250.0), row(-1.0, -1.0)]
    counts, stats = br.burden_bin(rows, H, W, cell, 1, 0.0)
    assert counts[0, 1, 0] == 1          # left of the slide
    assert counts[0, 0, 1] == 1          # above
    assert counts[0, 1, 4] == 1          # far right: the last column
    assert counts[0, 3, 1] == 1          # 199.5 -> pixel 199, the ragged last row
    assert counts[0, 3, 4] == 1          # beyond the bottom: clamped to pixel 199
    assert counts[0, 0, 0] == 1
    assert stats[0] == 6 and stats[1:].sum() == 0       # nothing is lost


def test_flagged_rows_and_the_flag_bits():
    C = 3
    bad_xy = [row(NAN, 5.0), row(5.0, INF), [-INF, 0.0, INF, 4.0, 0.9, 0.8, 0.0]]
    counts, stats = br.burden_bin(bad_xy, 100, 100, 10, C, 0.0)
    assert counts.sum() == 0 and list(stats) == [0, 0, 0, 0, 3, br.FLAG_NONFINITE]
    bad_cls = [row(5.0, 5.0, cls=-1), row(5.0, 5.0, cls=C), row(5.0, 5.0, cls=0.5), row(5.0, 5.0, cls=NAN)]
    counts, stats = br.burden_bin(bad_cls, 100, 100, 10, C, 0.0)
    assert counts.sum() == 0 and list(stats) == [0, 0, 0, 0, 4, br.FLAG_CLASS]
    counts, stats = br.burden_bin(bad_xy + bad_cls + [row(5.0, 5.0, cls=2), row(NAN, 5.0, cls=7, conf=NAN)], 100, 100, 10, C, 0.0)
    assert counts[2, 0, 0] == 1 and list(stats) == [0, 0, 1, 0, 8, br.FLAG_NONFINITE | br.FLAG_CLASS]
    # fp32 overflow of x1 + x2 is a centre that is not finite
    _, stats = br.burden_bin([[3e38, 0.0, 3e38, 4.0, 0.9, 0.8, 0.0]], 100, 100, 10, C, 0.0)
    assert stats[C + 1] == 1 and stats[C + 2] == br.FLAG_NONFINITE


def test_confidence_threshold():
    rows = [row(5.0, 5.0, conf=0.5), row(5.0, 5.0, conf=np.float32(0.5) - np.float32(1e-7)), row(5.0, 5.0, conf=NAN), row(5.0, 5.0, conf=0.7, cls=1)]
    counts, stats = br.burden_bin(rows, 100, 100, 10, 2, 0.5)
    assert counts[0, 0, 0] == 1 and counts[1, 0, 0] == 1          # conf == min_conf counts
    assert list(stats) == [1, 1, 2, 0, 0]                         # just below, and a NaN confidence, are below
    # a flagged row is flagged whatever its confidence
    _, stats = br.burden_bin([row(NAN, 5.0, conf=0.1)], 100, 100, 10, 2, 0.5)
    assert list(stats) == [0, 0, 0, 1, br.FLAG_NONFINITE]


@pytest.mark.parametrize("cell", [1, 64, 4096])
def test_invariants_on_random_rows(cell):
    H, W, C = 1000, 777, 3
    rows = br.random_rows(400, H, W, C, 11, True)
    counts, stats = br.burden_bin(rows, H, W, cell, C, 0.5)
    assert counts.shape == (C,) + br.grid(H, W, cell)
    for c in range(C):
        assert counts[c].sum() == stats[c]
    assert stats[:C].sum() + stats[C] + stats[C + 1] == len(rows)
    assert stats[C] >= 3 and stats[C + 1] >= 3 and stats[C + 2] == 3 and stats[:C].min() > 50      # the generator makes every kind
    assert 0.02 < (stats[C] + stats[C + 1]) / len(rows) < 0.1
    if cell == 4096:
        assert counts.shape == (C, 1, 1)


# ---- field sums -------------------------------------------------------------------------------------------------------------------------
def test_field_sums_two_formulations():
    rng = np.random.default_rng(5)
    for gy, gx, F in ((1, 1, 1), (5, 9, 1), (5, 9, 3), (9, 5, 5), (12, 31, 7), (8, 8, 8), (7, 40, 8), (40, 7, 8)):
        plane = rng.integers(0, 4097, (gy, gx)).astype(np.int32)
        a, b = br.field_sums_loops(plane, F), br.field_sums_sat(plane, F)
        np.testing.assert_array_equal(a, b)
        if gy >= F and gx >= F:
            assert a.shape == (gy - F + 1, gx - F + 1)
            for fy, fx in ((0, 0), (gy - F, gx - F), ((gy - F) // 2, (gx - F) // 3)):     # cell by cell, as the rule writes it
                assert a[fy, fx] == sum(int(plane[fy + dy, fx + dx]) for dy in range(F) for dx in range(F))
        else:
            assert a.size == 0


# ---- THE FIELD RULE -------------------------------------------------------------------------------------------------------------------
def plane(gy, gx, cells):
    p = np.zeros((1, gy, gx), np.int32)
    for (y, x), v in cells.items():
        p[0, y, x] = v
    return p


def test_tie_goes_to_the_lowest_index():
    counts = plane(6, 6, {(4, 4): 3, (0, 3): 3, (2, 0): 3})
    fields, n = br.field_select(counts, None, 1, 0, 3)
    assert n[0] == 3 and fields[0].tolist() == [[0, 3, 3, 0], [2, 0, 3, 0], [4, 4, 3, 0]]
    # with F = 2 several fields hold the same cell: the first of them in index order wins
    fields, n = br.field_select(plane(6, 6, {(3, 3): 5}), None, 2, 0, 1)
    assert fields[0, 0].tolist() == [2, 2, 5, 0]


def test_an_overlapping_runner_up_is_skipped():
    counts = plane(6, 8, {(1, 1): 5, (2, 2): 4, (1, 5): 2})
    fields, n = br.field_select(counts, None, 2, 0, 3)
    # the winner holds both (1,1) and (2,2): field (1,1), n = 9; every other field with (2,2) overlaps it
    assert fields[0, 0].tolist() == [1, 1, 9, 0]
    assert fields[0, 1].tolist() == [0, 4, 2, 0] and n[0] == 2 and fields[0, 2].tolist() == [-1] * 4
    assert br.suppression_acted(counts, None, 2, 0, fields, n) == 1
    # overlap is |dy| < F and |dx| < F: a field exactly F away is free
    counts = plane(2, 6, {(0, 0): 3, (0, 2): 2, (0, 1): 1})
    fields, n = br.field_select(counts, None, 2, 0, 3)
    assert fields[0, :2].tolist() == [[0, 0, 4, 0], [0, 2, 2, 0]] and n[0] == 2


def test_k_larger_than_what_fits_and_grids_without_a_field():
    counts = np.ones((1, 4, 4), np.int32)
    fields, n = br.field_select(counts, None, 2, 0, 9)
    assert n[0] == 4 and fields[0, :4, :2].tolist() == [[0, 0], [0, 2], [2, 0], [2, 2]] and (fields[0, 4:] == -1).all()
    fields, n = br.field_select(np.ones((2, 7, 40), np.int32), np.ones((7, 40), np.int32), 8, 0, 3)      # Gy < F
    assert n.tolist() == [0, 0] and (fields == -1).all()
    fields, n = br.field_select(np.ones((1, 8, 8), np.int32), None, 8, 0, 3)                           # F == Gy == Gx: one field
    assert n[0] == 1 and fields[0, 0].tolist() == [0, 0, 64, 0] and (fields[0, 1:] == -1).all()


def test_an_ineligible_field_holding_the_maximum():
    counts = plane(4, 8, {(1, 1): 9, (1, 6): 2})
    tissue = np.full((4, 8), 100, np.int32)
    tissue[0:3, 0:3] = 0                                           # no tissue under the maximum
    trace = {}
    fields, n = br.field_select(counts, tissue, 2, 400, 2, trace=trace)
    assert fields[0, 0].tolist() == [0, 5, 2, 400] and n[0] == 1 and trace["ineligible"] == 1
    tissue[2, 2] = 1                                               # field (1, 1) now has one tissue pixel
    fields, n = br.field_select(counts, tissue, 2, 1, 2)
    assert fields[0].tolist() == [[1, 1, 9, 1], [0, 5, 2, 400]] and n[0] == 2
    fields, n = br.field_select(counts, None, 2, 400, 2)           # without a tissue plane every field is eligible, t = 0
    assert fields[0, 0].tolist() == [0, 0, 9, 0] and n[0] == 2


def test_an_all_zero_class_finds_nothing():
    counts = np.zeros((2, 5, 5), np.int32)
    counts[1, 2, 2] = 1
    fields, n = br.field_select(counts, None, 2, 0, 3)
    assert n.tolist() == [0, 1] and (fields[0] == -1).all() and fields[1, 0].tolist() == [1, 1, 1, 0]


def test_selection_does_not_depend_on_the_sums_formulation():
    for gy, gx, F, K in br.FIELD_CASES[:5]:
        counts, tissue, need = br.field_case(gy, gx, F, K, 3)
        a = br.field_select(counts, tissue, F, need, K)
        b = br.field_select(counts, tissue, F, need, K, sums=br.field_sums_sat)
        np.testing.assert_array_equal(a[0], b[0])
        np.testing.assert_array_equal(a[1], b[1])


# ---- argument checks of the Python surface: ValueError before any device work ---------------------------------------------------------
def test_burden_map_rejects_bad_arguments():
    rows = np.zeros((4, 7), np.float32)
    for kw in (dict(cell=0), dict(cell=1.5), dict(cell=True), dict(num_classes=0), dict(num_classes=65), dict(num_classes=2.0)):
        with pytest.raises(ValueError):
            burden_map(rows, (100, 100), **{"num_classes": 2, **kw})
    for hw in ((0, 100), (100, -1), (100.0, 100)):
        with pytest.raises(ValueError):
            burden_map(rows, hw, num_classes=2)
    for bad in (np.zeros((4, 6), np.float32), np.zeros(7, np.float32), None):
        with pytest.raises(ValueError):
            burden_map(bad, (100, 100), num_classes=2)
    with pytest.raises(ValueError):
        burden_map(rows, (40000, 40000), cell=1, num_classes=2)      # 3.2e9 counters
    with pytest.raises(ValueError):
        burden_map(rows, (100, 100), num_classes=2, min_conf="high")


def test_densest_fields_rejects_bad_arguments():
    counts, tissue = np.zeros((2, 8, 9), np.int32), np.zeros((8, 9), np.int32)
    for kw in (dict(field=0), dict(field=46341), dict(field=2.0), dict(top_k=0), dict(top_k=65), dict(need_tissue=-1), dict(need_tissue=0.5),
               dict(tissue=np.zeros((9, 8), np.int32))):
        with pytest.raises(ValueError):
            densest_fields(counts, **{"tissue": tissue, **kw})
    for bad in (np.zeros((8, 9), np.int32), np.zeros((65, 8, 9), np.int32), np.zeros((0, 8, 9), np.int32), np.zeros((2, 0, 9), np.int32), None):
        with pytest.raises(ValueError):
            densest_fields(bad)


def test_quantify_region_rejects_bad_arguments():
    raster = np.full((64, 96, 3), 255, np.uint8)
    for kw in (dict(cell=0), dict(field=0), dict(top_k=0), dict(top_k=65), dict(cell=4096, field=12),      # 49152 > 46340
               dict(field_min_tissue=1.5), dict(field_min_tissue=-0.1), dict(field_min_tissue=NAN), dict(mpp=0.0), dict(mpp=-1.0), dict(mpp=NAN),
               dict(cell=40),                        # the default probe_stride 16 does not divide 40
               dict(cell=32, probe_stride=5), dict(cell=32, probe_stride=0), dict(min_conf="high")):
        with pytest.raises(ValueError):
            quantify_region(None, raster, **kw)      # no model is touched before the checks
    with pytest.raises(ValueError):
        quantify_region(None, np.zeros((64, 96), np.uint8))
