"""Spatial statistics without a GPU: the restatement of THE PAIR RULE against its own second formulation, the host formulas on a
lattice one can count by hand, and the conversions and argument checks of wsi.spatial_stats / quantify_region(spatial_radii=...),
which raise before any device work."""
import math

import numpy as np
import pytest

import spatial_reference as sr
from amyloid_yolo_paper_amd import wsi

H, W = sr.SLIDE_H, sr.SLIDE_W


@pytest.mark.parametrize("M", [1, 2, 63, 65])
@pytest.mark.parametrize("border", [True, False])
def test_brute_force_equals_the_pair_loop(M, border):
    rows = sr.clustered_rows(M, 7 + M)
    rq = sr.radii_q(sr.RADII_PX)
    roi = None if M == 63 else sr.roi_q((300.0, 200.5, 3800.25, 2900.0), H, W)
    a, b = sr.pair_counts(rows, H, W, 3, 0.5, rq, roi, border), sr.pair_counts_loop(rows, H, W, 3, 0.5, rq, roi, border)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x, y)


def assert_same_outputs(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("M,border", [(M, True) for M in sr.SIZES] + [(M, False) for M in sr.SIZES if M <= 257])
def test_the_cell_grid_formulation_equals_the_brute_force_on_the_clustered_cases(M, border):
    """pair_counts_binned (the reference of the sizes all pairs are too many for) against pair_counts, every output, on the cases the
    GPU tests take"""
    rows, rq, want = sr.clustered_case(M, border)
    assert_same_outputs(sr.pair_counts_binned(rows, H, W, sr.CLASSES, 0.5, rq, None, border), want)
    if M == 257:                                                   # a window of the caller's; one radius (one cell side for all)
        roi = sr.roi_q((300.0, 200.5, 3800.25, 2900.0), H, W)
        assert_same_outputs(sr.pair_counts_binned(rows, H, W, 3, 0.5, rq, roi, border), sr.pair_counts(rows, H, W, 3, 0.5, rq, roi, border))
        assert_same_outputs(sr.pair_counts_binned(rows, H, W, 3, 0.5, rq[2:3], None, border), sr.pair_counts(rows, H, W, 3, 0.5, rq[2:3], None, border))


@pytest.mark.parametrize("border", [True, False])
def test_the_cell_grid_formulation_equals_the_brute_force_on_the_lattices(border):
    """pairs at exactly R_k (3-4-5 and 5-12-13 on a lattice 1 px apart), partners exactly on cell borders, duplicates at one position"""
    cases = [(sr.lattice_rows(9, 10.0, C=1, x0=60.0, y0=60.0), 200, 200, 1, sr.radii_q((10, 15))),
             (sr.lattice_rows(16, 1.0, C=2, side=6.0, x0=20.0, y0=24.0), 64, 64, 2, sr.radii_q((5, 13))),
             (sr.lattice_rows(16, 1.0, C=2, side=6.0, x0=20.0, y0=24.0), 64, 64, 2, sr.radii_q((4.75, 13))),
             (sr.lattice_rows(12, 8.0, C=2, x0=0.0, y0=8.0), 100, 100, 2, sr.radii_q((1, 3.5, 8))),     # 32 quarter pixels: the cell side
             (sr.points([[100.25, 50.5]] * 100, cls=np.arange(100) % 3), 200, 300, 3, sr.radii_q((0.25, 2)))]
    for rows, H_, W_, C_, rq in cases:
        want = sr.pair_counts(rows, H_, W_, C_, 0.0, rq, None, border)
        assert want[0].sum() > 0
        assert_same_outputs(sr.pair_counts_binned(rows, H_, W_, C_, 0.0, rq, None, border), want)


def test_the_clustered_cases_are_not_idle():
    for M in (257, 4097):
        rows, rq, res = sr.clustered_case(M)          # (check_not_idle runs inside)
        pairs, centres, nn, bd, stats = res
        assert pairs.dtype == np.int64 and centres.dtype == nn.dtype == bd.dtype == stats.dtype == np.int32
        assert stats[:3].sum() + stats[6] + stats[7] == M and stats[8] == 3


def test_pairs_are_monotone_in_k_and_symmetric_without_border():
    rows, rq, res = sr.clustered_case(257, border=False)
    pairs, centres = res[0], res[1]
    assert (np.diff(pairs, axis=2) >= 0).all()
    assert (centres == centres[:, :1]).all()                       # without the border rule every counted row is a centre at every k
    np.testing.assert_array_equal(pairs[:, :, -1], pairs[:, :, -1].T)
    assert (pairs[:, :, -1] > 0).all()
    with_border = sr.clustered_case(257)[2][0]                     # (the border rule only ever drops centres)
    assert (with_border <= pairs).all() and (with_border < pairs).any()


def test_lattice_by_hand():
    """a 9 x 9 lattice of one class, 10 px apart, on a 200 x 200 slide, radii 10 and 15 px: an inner point has 4 neighbours within
    10 px (equality counts) and 8 within 15 px (the diagonals are 14.14 px away)"""
    rows = sr.lattice_rows(9, 10.0, C=1, x0=60.0, y0=60.0)
    rq = sr.radii_q((10, 15))
    assert rq.tolist() == [40, 60]
    pairs, centres, nn, bd, stats = sr.pair_counts(rows, 200, 200, 1, 0.0, rq)
    # the points stand at 60 .. 140 px; the border distance is min(q, 799 - q) quarter pixels: 239 at the least -> all eligible
    assert centres.tolist() == [[81, 81]] and stats.tolist() == [81, 81, 0, 0, 0]
    n4 = 49 * 4 + 28 * 3 + 4 * 2              # inner, edge, corner points
    n8 = 49 * 8 + 28 * 5 + 4 * 3
    assert pairs.reshape(-1).tolist() == [n4, n8]
    assert (nn[:, 0, 0] == 1600).all() and bd.min() == 239
    assert nn[0, 0, 1] == 1 and nn[40, 0, 1] == 31                # ties: the lowest row index (right neighbour of 0; upper of the middle)
    s = sr.summaries(pairs, centres, stats[1:2], bd, nn, np.zeros(81, int), rq, 200.0 * 200.0, mpp=0.5)
    lam = 81 / 40000.0
    assert s["intensity"][0] == lam
    assert s["K"][0, 0].tolist() == [n4 / (81 * lam), n8 / (81 * lam)]
    assert s["L"][0, 0, 1] == math.sqrt(n8 / (81 * lam) / math.pi) and s["L_minus_r"][0, 0, 1] == s["L"][0, 0, 1] - 15.0
    assert s["g"][0, 0, 0] == s["K"][0, 0, 0] / (math.pi * 100.0)
    assert s["g"][0, 0, 1] == (s["K"][0, 0, 1] - s["K"][0, 0, 0]) / (math.pi * (225.0 - 100.0))
    assert s["G"][0, 0].tolist() == [1.0, 1.0]
    assert s["radii_um"].tolist() == [5.0, 7.5] and s["K_um2"][0, 0, 0] == s["K"][0, 0, 0] * 0.25
    # the product's host formulas say the same
    got = wsi.spatial_summaries(pairs, centres, stats[1:2], bd, nn, rq, 40000.0, 0.5, np.zeros(81, np.int64))
    for key in s:
        np.testing.assert_array_equal(got[key], s[key], err_msg=key)


def test_host_formulas_on_a_random_case_and_nan_where_nothing_is():
    rows, rq, (pairs, centres, nn, bd, stats) = sr.clustered_case(257)
    cls = sr.positions(rows, H, W, 3, 0.5)[2]
    want = sr.summaries(pairs, centres, stats[3:6], bd, nn, cls, rq, float(H * W))
    got = wsi.spatial_summaries(pairs, centres, stats[3:6], bd, nn, rq, float(H * W), None, cls)
    for key in want:
        np.testing.assert_allclose(got[key], want[key], rtol=1e-14, atol=0, err_msg=key)      # (vectorised against entry by entry)
        assert np.isfinite(want[key]).all()
    none = wsi.spatial_summaries(np.zeros((2, 2, 3)), np.zeros((2, 3)), np.zeros(2), np.zeros(0, np.int32), np.zeros((0, 2, 2), np.int32),
                                 [4, 8, 12], 100.0, None, np.zeros(0, np.int64))
    assert all(np.isnan(none[k]).all() for k in ("K", "L", "L_minus_r", "g", "G")) and (none["intensity"] == 0).all()
    assert np.isnan(wsi.spatial_summaries(pairs, centres, stats[3:6], bd, nn, rq, 0.0, None, cls)["K"]).all()     # no area


def test_radius_and_roi_conversion():
    assert wsi.spatial_radii_q([8, 16.3, 16.5, 8191.75]).tolist() == [32, 65, 66, 32767]
    assert wsi.spatial_radii_q(np.array([0.25])).tolist() == [1] and wsi.spatial_radii_q([1]).dtype == np.int32
    assert wsi.spatial_radii_q(sr.RADII_PX).tolist() == sr.radii_q(sr.RADII_PX).tolist()
    for bad in ([], [0.2], [8, 8], [8, 8.2], [16, 8], [8192], [float("nan")], [float("inf")], 8, "8", [[8, 16]], list(range(1, 34)), None):
        with pytest.raises(ValueError):
            wsi.spatial_radii_q(bad)
    assert wsi.spatial_roi_q(None, (10, 20)).tolist() == [0, 0, 79, 39]
    assert wsi.spatial_roi_q((0.1, 0.25, 5.3, 5.25), (10, 20)).tolist() == [1, 1, 21, 21]
    assert wsi.spatial_roi_q((-5, -5, 100, 100), (10, 20)).tolist() == [0, 0, 79, 39]
    assert wsi.spatial_roi_q((3, 4, 3, 4), (10, 20)).tolist() == [12, 16, 12, 16]              # one position
    for roi in ((0.1, 0.25, 5.3, 5.25), None, (-5, -5, 100, 100)):
        assert wsi.spatial_roi_q(roi, (10, 20)).tolist() == sr.roi_q(roi, 10, 20).tolist()
    for bad in ((5, 0, 4, 9), (0, 0.1, 9, 0.2), (30, 0, 40, 5), (0, 0, 1), (0, 0, float("nan"), 5), "roi"):
        with pytest.raises(ValueError):
            wsi.spatial_roi_q(bad, (10, 20))


def test_spatial_stats_rejects_bad_arguments_before_any_device_work():
    rows = np.zeros((4, 7), np.float32)
    ok = dict(rows=rows, slide_hw=(100, 100), radii=[4, 8])
    for kw in (dict(radii=[8, 8.1]), dict(radii=[]), dict(radii=[9000]), dict(slide_hw=(0, 100)), dict(slide_hw=(100, (1 << 21) + 1)),
               dict(slide_hw=(100.0, 100)), dict(slide_hw=100), dict(num_classes=0), dict(num_classes=9), dict(num_classes=True),
               dict(roi=(50, 50, 40, 60)), dict(roi=(0, 0, 1)), dict(area=-1.0), dict(area=float("nan")), dict(area=float("inf")),
               dict(mpp=0.0), dict(mpp=float("nan")), dict(rows=np.zeros((4, 6), np.float32)), dict(rows=None)):
        with pytest.raises(ValueError):
            wsi.spatial_stats(**{**ok, **kw})


def test_quantify_region_rejects_bad_spatial_radii_before_the_model_is_touched():
    raster = np.zeros((64, 96, 3), np.uint8)
    for radii in ([], [8, 8], [0.1], [9000], 8, [float("nan")]):
        with pytest.raises(ValueError):
            wsi.quantify_region(None, raster, spatial_radii=radii)      # no model is touched before the checks

    class NineClasses:
        class Layer:
            num_classes = 9
        yolo_layers = [Layer]

    with pytest.raises(ValueError, match="classes"):
        wsi.quantify_region(NineClasses, raster, spatial_radii=[8, 16])
