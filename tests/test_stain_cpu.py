"""THE STAIN RULE on the host (no GPU): the tables, the table's error bound against the exact exponential, the percentile and
fraction arithmetic of the histograms, the gains, and every argument the Python surface refuses.

Bounds.  The map's table is piecewise linear in 1/64-OD steps; against 10^-x its interpolation error is at most h^2 / 8 * max|f''| =
(ln 10 / 64)^2 / 8 * 256 / 255 = 1.63e-4 of full scale.  On top come a few fp32 roundings of values <= 4 * 64 and <= 1 (each below
1e-6 of full scale after the table's slope of at most ln 10 * 256 / 255 / 64 per unit of u): the tests assert 1.7e-4."""
import math

import numpy as np
import pytest

import stain_reference as sref
from amyloid_yolo_paper_amd import wsi
from amyloid_yolo_paper_amd.wsi import H_DAB, StainBasis, StainMap, StainStats

BOUND = 1.7e-4
ALL = np.arange(256, dtype=np.uint8)


def test_interpolation_bound_is_the_stated_one():
    assert (math.log(10) / 64) ** 2 / 8 * 256 / 255 == pytest.approx(1.63e-4, rel=5e-3) and 1.63e-4 < BOUND


def test_tables():
    t = sref.tables()
    assert t["od"][255] == 0 and t["T"][0] == 1 and all(v.dtype == np.float32 for v in t.values())
    assert [len(t[k]) for k in ("od", "D", "A", "T")] == [256, 9, 9, 257]
    assert (np.diff(t["od"]) < 0).all() and (np.diff(t["T"]) < 0).all()
    # the product's builder gives the same bits, for the identity and for gains
    for g in ((1.0, 1.0), (1.3, 0.7), (4.0, 0.25)):
        want, got = sref.tables(g), wsi.stain_tables(H_DAB, g)
        for k in want:
            assert np.asarray(getattr(got, k), np.float32).tobytes() == want[k].tobytes(), (g, k)
    assert np.array_equal(H_DAB.M, sref.basis())
    # with the default basis no uint8 pixel reaches bin 511
    grid = np.stack(np.meshgrid(ALL[::5], ALL[::5], ALL[::5], indexing="ij"), -1).reshape(-1, 3)
    c = sref.concentrations(grid, t)
    print("largest concentration with H_DAB on the grid:", c.max())
    assert c.max() < 4.55 and sref.bins(c).max() < 511


def test_identity_map_returns_every_grey_value():
    t = sref.tables()
    grey = np.repeat(ALL[:, None], 3, 1)
    x = sref.map_pixels(grey, t)
    err = np.abs(x.astype(np.float64) - ALL[:, None] / 255.0).max()
    print("identity map, largest deviation from v / 255:", err)
    assert err <= BOUND
    assert np.array_equal(sref.to_u8(x), grey)
    # and coloured pixels: each channel on its own against its byte
    px = np.random.default_rng(0).integers(0, 256, size=(20000, 3), dtype=np.uint8)
    x = sref.map_pixels(px, t)
    assert np.abs(x.astype(np.float64) - px / 255.0).max() <= BOUND and np.array_equal(sref.to_u8(x), px)


def test_map_with_gains_against_the_exact_exponential():
    px = np.random.default_rng(1).integers(0, 256, size=(100000, 3), dtype=np.uint8)
    for g in ((1.3, 0.7), (4.0, 0.25)):
        x = sref.map_pixels(px, sref.tables(g))
        err = np.abs(x.astype(np.float64) - sref.exact_map(px, g)).max()
        print("gains", g, "largest deviation from the float64 exact-exponential map:", err)
        assert err <= BOUND
    assert not np.array_equal(sref.to_u8(sref.map_pixels(px, sref.tables((1.3, 0.7)))), px)


def hist_of(bins0, bins1):
    h = np.zeros((2, 512), np.int64)
    for s, bs in enumerate((bins0, bins1)):
        for b, n in bs.items():
            h[s, b] = n
    return h


def test_strength_on_hand_made_histograms():
    # first bin, last bin
    s = StainStats(hist_of({0: 10}, {511: 10}), 10)
    assert s.strength(99.0) == (1 / 64, 512 / 64) == sref.strength(s.hist, 10, 99.0)
    # K on a bin edge: n = 100, bins 3 and 7 hold 50 each: p = 50 -> K = 50 is reached IN bin 3, p = 51 -> K = 51 in bin 7
    s = StainStats(hist_of({3: 50, 7: 50}, {3: 50, 7: 50}), 100)
    assert s.strength(50.0) == (4 / 64, 4 / 64) and s.strength(51.0) == (8 / 64, 8 / 64)
    assert s.strength(100.0) == (8 / 64, 8 / 64) and s.strength(1e-9) == (4 / 64, 4 / 64)      # K = max(1, ...) = 1
    for p in (50.0, 51.0, 99.0, 100.0, 0.5):
        assert s.strength(p) == sref.strength(s.hist, 100, p)
    # K = ceil(p n / 100) rounds up: n = 3, p = 34 -> K = 2
    s = StainStats(hist_of({1: 1, 5: 1, 9: 1}, {2: 3}), 3)
    assert s.strength(33.0) == (2 / 64, 3 / 64) and s.strength(34.0) == (6 / 64, 3 / 64) and s.strength(67.0) == (10 / 64, 3 / 64)
    with pytest.raises(ValueError):
        StainStats(hist_of({}, {}), 0).strength()
    with pytest.raises(ValueError):
        sref.strength(np.zeros((2, 512), np.int64), 0, 99.0)
    for p in (0.0, -1.0, 100.5, math.nan, math.inf):
        with pytest.raises(ValueError):
            s.strength(p)


def test_positive_fraction_bin_arithmetic():
    s = StainStats(hist_of({0: 100}, {0: 60, 9: 10, 10: 20, 400: 10}), 100)
    assert s.positive_fraction(1, 10 / 64) == (0.30, 10 / 64)
    assert s.positive_fraction(1, 0.15) == (0.30, 10 / 64)                  # round(9.6) = 10: the threshold moves to a bin edge
    assert s.positive_fraction(1, 0.147) == (0.40, 9 / 64)                  # round(9.408) = 9
    assert s.positive_fraction(1, 0.0) == (1.0, 0.0) and s.positive_fraction(0, 1 / 64) == (0.0, 1 / 64)
    assert s.positive_fraction(1, 401 / 64)[0] == 0.0 and s.positive_fraction(1, 100.0)[0] == 0.0
    for thres in (10 / 64, 0.15, 0.147, 0.0, 6.25):
        assert s.positive_fraction(1, thres) == sref.positive_fraction(s.hist, 100, 1, thres)
    assert math.isnan(StainStats(hist_of({}, {}), 0).positive_fraction(1, 0.15)[0])
    for bad in (-0.1, math.nan, math.inf):
        with pytest.raises(ValueError):
            s.positive_fraction(1, bad)
    with pytest.raises(ValueError):
        s.positive_fraction(2, 0.15)


def test_gains_are_clipped():
    s = StainStats(hist_of({63: 10}, {31: 10}), 10)            # strengths (1.0, 0.5)
    assert s.strength() == (1.0, 0.5)
    assert StainMap(s, (1.3, 0.35)).gains == (1.3, 0.7) == sref.gains((1.0, 0.5), (1.3, 0.35))
    assert StainMap(s, (100.0, 0.001)).gains == (4.0, 0.25)
    assert StainMap(s, (100.0, 0.001), max_gain=2.0).gains == (2.0, 0.5)
    assert StainMap(s, (3.0, 0.1), max_gain=1.0).gains == (1.0, 1.0)
    t = StainStats(hist_of({127: 10}, {15: 10}), 10)           # a StainStats as the target: its strengths (2.0, 0.25)
    m = StainMap(s, t)
    assert m.gains == (2.0, 0.5) and m.basis == H_DAB
    assert np.asarray(m.tables.A, np.float32).tobytes() == sref.tables((2.0, 0.5))["A"].tobytes()
    assert StainMap.identity().gains == (1.0, 1.0)
    assert StainMap.identity(StainBasis((1, 0, 0), (0, 1, 0))).basis != H_DAB


def test_bad_arguments_raise_before_any_launch():
    s = StainStats(hist_of({63: 10}, {31: 10}), 10)
    other = StainBasis((0.65, 0.70, 0.29), (0.07, 0.99, 0.11))                  # hematoxylin / eosin
    for p in (0.0, -5.0, 101.0, math.nan):
        with pytest.raises(ValueError):
            StainMap(s, (1.0, 1.0), p=p)
    for target in ((0.0, 1.0), (1.0, -1.0), (math.nan, 1.0), (math.inf, 1.0), (1.0,), (1.0, 1.0, 1.0), 3.0, None):
        with pytest.raises(ValueError):
            StainMap(s, target)
    for g in (0.5, 0.999, math.nan, math.inf, -2.0):
        with pytest.raises(ValueError):
            StainMap(s, (1.0, 1.0), max_gain=g)
    for a, b in (((1, 2, 3), (2, 4, 6)), ((0, 0, 0), (1, 0, 0)), ((1, 0, 0), (math.nan, 1, 0)), ((1, 0), (0, 1, 0)), ((1, 0, 0), (1, 0, 1e-9))):
        with pytest.raises(ValueError):
            StainBasis(a, b)
    with pytest.raises(ValueError):
        StainMap(s, (1.0, 1.0), basis=other)                                     # a basis that is not the source statistics'
    with pytest.raises(ValueError):
        StainMap(s, StainStats(s.hist, 10, other))                               # target statistics on another basis
    with pytest.raises(ValueError):
        StainMap((1.0, 0.5), (1.0, 1.0))                                         # the source is statistics, not strengths
    with pytest.raises(ValueError):
        StainMap(StainStats(hist_of({}, {}), 0), (1.0, 1.0))                     # no tissue
    with pytest.raises(ValueError):
        StainStats(hist_of({1: 3}, {1: 4}), 3)                                   # rows that do not sum to n_tissue
    raster = np.full((8, 8, 3), 200, np.uint8)
    with pytest.raises(ValueError):
        wsi.stain_stats(raster, bg_level=257)
    with pytest.raises(ValueError):
        wsi.stain_stats(raster, probe_stride=0)
    with pytest.raises(ValueError):
        wsi.stain_stats(raster, basis="H_DAB")
    with pytest.raises(ValueError):
        wsi.normalize_region(raster, stain=(1.0, 1.0))
    with pytest.raises(ValueError):
        wsi.detect_region(None, raster, stain=(1.0, 1.0))
    with pytest.raises(ValueError):
        wsi.RegionTileStream(raster, 8, 8, stain="identity")
    m = StainMap(s, (1.0, 1.0))
    with pytest.raises(ValueError):
        wsi.quantify_region(None, raster, stain_stats=s)                         # the two arguments go together
    with pytest.raises(ValueError):
        wsi.quantify_region(None, raster, dab_thres=0.15)
    with pytest.raises(ValueError):
        wsi.quantify_region(None, raster, stain_stats=s, dab_thres=-1.0)
    with pytest.raises(ValueError):
        wsi.quantify_region(None, raster, stain_stats=StainStats(s.hist, 10, other), dab_thres=0.15, stain=m)
