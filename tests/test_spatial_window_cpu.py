"""THE PAIR WINDOW RULE without a GPU: the restatement (tests/spatial_window_reference.py) against a second formulation and against
spatial_reference's rectangle, the cases of the GPU tests say something, and the host side of wsi.spatial_stats(window=...)."""
import numpy as np
import pytest

import spatial_reference as sr
import spatial_window_reference as wr
from amyloid_yolo_paper_amd import wsi


def test_window_bd_against_every_out_position_on_a_tiny_slide():
    H, W, cell, r_max = 44, 61, 16, 70                          # 3 x 4 cells, the last row and column cut to 12 and 13 px
    rng = np.random.default_rng(1)
    qx, qy = rng.integers(0, 4 * W, 150), rng.integers(0, 4 * H, 150)
    seen = set()
    for mask in (np.ones((3, 4), np.uint8), np.zeros((3, 4), np.uint8), np.array([[1, 1, 1, 1], [1, 0, 1, 1], [1, 1, 1, 1]], np.uint8),
                 np.array([[0, 1, 1, 0], [1, 1, 1, 1], [1, 1, 0, 1]], np.uint8), (rng.uniform(size=(3, 4)) < 0.6).astype(np.uint8)):
        got = wr.window_bd(qx, qy, mask, cell, H, W, r_max)
        np.testing.assert_array_equal(got, wr.window_bd_by_positions(qx, qy, mask, cell, H, W, r_max))
        assert got.min() >= -1 and got.max() <= r_max
        assert ((got == -1) == (mask[qy // 64, qx // 64] == 0)).all()
        seen |= set(got.tolist())
    assert {-1, 0, 1, r_max} <= seen and len(seen) > 40           # the cap, the OUT cells and the values between all occur
    assert wr.wbd_of([0, 1, 2, 25, 26, 70 * 70, 70 * 70 + 1, 10 ** 9], 70).tolist() == [-1, 0, 1, 4, 5, 69, 70, 70]


@pytest.mark.parametrize("H,W", [(384, 512), (390, 500)])
def test_an_all_in_mask_is_the_rectangle_with_bd_capped(H, W):
    rows = wr.ragged_rows(257, 31, H, W, 3)
    rq = sr.radii_q((3, 10.5, 40))
    for cell in (16, 32):
        mask = np.ones(wr.grid_of(H, W, cell), np.uint8)
        for border in (True, False):
            got = wr.pair_counts_window(rows, H, W, 3, 0.5, rq, mask, cell, None, border)
            want = sr.pair_counts(rows, H, W, 3, 0.5, rq, None, border)
            for k in (0, 1, 2, 4):
                assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), (cell, border, k)
            np.testing.assert_array_equal(got[3], np.where(want[3] >= 0, np.minimum(want[3], rq[-1]), -1))
            assert (want[3] > rq[-1]).any() and (want[3] == -1).any()
        roi = np.array([300, 200, 1500, 1100], np.int32)
        got, want = wr.pair_counts_window(rows, H, W, 3, 0.5, rq, mask, cell, roi), sr.pair_counts(rows, H, W, 3, 0.5, rq, roi)
        assert all(got[k].tobytes() == want[k].tobytes() for k in (0, 1, 2, 4))


@pytest.mark.parametrize("M", wr.SIZES)
def test_the_ragged_cases_are_not_idle(M):
    rows, rq, mask, res = wr.ragged_case(M)                     # (asserts check_not_idle for M >= 257)
    assert mask.shape == (49, 65) and 0.3 < mask.mean() < 0.8 and wr.SLIDE_H % wr.CELL and wr.SLIDE_W % wr.CELL
    assert len(rows) == M and res[3].shape == (M,) and res[4][:2].sum() + res[4][4] + res[4][5] == M
    loose = wr.ragged_case(M, border=False)[3]
    assert (loose[1] == loose[4][2:4, None]).all()               # without the border rule every row in an IN cell is a centre
    if M >= 257:
        with pytest.raises(AssertionError):                     # the conditions do bite: an all-IN mask fails them
            qx, qy, cls = wr.positions(rows, wr.SLIDE_H, wr.SLIDE_W, wr.CLASSES, 0.5)[:3]
            rect = wr.pair_counts_window(rows, wr.SLIDE_H, wr.SLIDE_W, wr.CLASSES, 0.5, rq, np.ones_like(mask), wr.CELL)
            rbd = wr.rect_bd(qx, qy, wr.SLIDE_H, wr.SLIDE_W)
            wr.check_not_idle(M, rect, rect, np.minimum(rbd, rq[-1]), rbd, cls, int(rq[-1]))


def test_window_from_tissue_on_cut_border_cells():
    H, W, cell = 40, 50, 16                                     # cells of 16 x 16, 16 x 2 (last column), 8 x 16 (last row), 8 x 2 (corner)
    full = np.array([[256, 256, 256, 32], [256, 256, 256, 32], [128, 128, 128, 16]])
    for frac in (0.0, 0.25, 0.5, 1.0):
        need = np.maximum(1, np.ceil(frac * full)).astype(np.int64)
        for t in (need, need - 1, np.zeros_like(need), full):
            t = t.astype(np.int32)
            got = wsi.window_from_tissue(t, (H, W), cell, frac)
            assert got.dtype == np.bool_ and got.shape == (3, 4)
            np.testing.assert_array_equal(got, wr.window_from_tissue(t, H, W, cell, frac))
        np.testing.assert_array_equal(wsi.window_from_tissue(need.astype(np.int32), (H, W), cell, frac), np.ones((3, 4), bool))
        np.testing.assert_array_equal(wsi.window_from_tissue((need - 1).astype(np.int32), (H, W), cell, frac), np.zeros((3, 4), bool))
    half = np.array([[128, 127, 200, 16], [0, 256, 128, 15], [64, 63, 1, 8]], np.int32)
    assert wsi.window_from_tissue(half, (H, W), cell).tolist() == [[True, False, True, True], [False, True, True, False], [True, False, False, True]]
    for bad in (lambda: wsi.window_from_tissue(half, (H, W), 15), lambda: wsi.window_from_tissue(half, (H, W), 32),
                lambda: wsi.window_from_tissue(half, (H, W), cell, 1.5), lambda: wsi.window_from_tissue(half, (H, W), cell, float("nan")),
                lambda: wsi.window_from_tissue(half.astype(np.float32), (H, W), cell), lambda: wsi.window_from_tissue(half, (H,), cell)):
        with pytest.raises(ValueError):
            bad()


def test_window_area_counts_positions_in_integers():
    H, W, cell = 40, 50, 16
    mask = np.array([[1, 0, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1]], np.uint8)
    assert wsi.window_area(np.ones((3, 4), bool), (H, W), cell) == float(H * W) == wr.window_area(np.ones((3, 4)), cell, H, W)
    assert wsi.window_area(mask, (H, W), cell) == wr.window_area(mask, cell, H, W) == 4 * 256 + 32 + 128 + 128 + 16
    for roi in ([10, 7, 150, 101], [64, 64, 127, 127], [0, 0, 0, 0], [130, 3, 199, 159], [64, 0, 70, 10]):
        assert wsi.window_area(mask, (H, W), cell, np.array(roi, np.int32)) == wr.window_area(mask, cell, H, W, roi), roi
    assert wsi.window_area(mask, (H, W), cell, [64, 0, 70, 10]) == 0.0 and wsi.window_area(mask, (H, W), cell, [0, 0, 0, 0]) == 1 / 16


def test_spatial_stats_checks_the_window_before_it_needs_a_device():
    """every refusal comes before the rows are looked at and before a device is asked for: this passes on a machine without one"""
    rows = np.zeros((3, 7), np.float32)
    ok = np.ones((3, 4), np.uint8)                              # the cells of 16 px of a 40 x 50 slide
    for kw in (dict(window=ok), dict(window_cell=16), dict(window=ok, window_cell=15), dict(window=ok, window_cell=16.0),
               dict(window=ok, window_cell=True), dict(window=ok[:2], window_cell=16), dict(window=ok.T, window_cell=16),
               dict(window=ok.astype(np.int32), window_cell=16), dict(window=ok.astype(np.float32), window_cell=16),
               dict(window=ok.reshape(-1), window_cell=16), dict(window=ok, window_cell=32)):
        with pytest.raises(ValueError, match="window"):
            wsi.spatial_stats(rows, (40, 50), (2, 4), 2, **kw)
    with pytest.raises(ValueError, match="2\\*\\*26"):
        wsi.spatial_stats(rows, (1 << 21, 1 << 21), (2, 4), 2, window=ok, window_cell=16)
    assert "window_from_tissue" in dir(wsi) and wsi.PAIR_WINDOW_MIN_CELL == 16 and wsi.PAIR_WINDOW_MAX_CELLS == 1 << 26
