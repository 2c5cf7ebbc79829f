"""THE RELABEL RULE without a GPU: the keys' known answers, the label table of the product against the restatement's, the two
formulations of the restatement against one another, the host formulas of the envelope against plain loops, the argument checks of
wsi.spatial_envelope that need no device, and two statistical sanity cases on the restatement alone.

Yardstick: tests/spatial_envelope_reference.py."""
import os
import runpy
import sys

import numpy as np
import pytest

import spatial_envelope_reference as er
import spatial_reference as sr
import spatial_window_reference as swr
from amyloid_yolo_paper_amd import wsi


# ---- 1. the keys and the table --------------------------------------------------------------------------------------------------------
def test_known_answers_of_the_keys():
    assert [er.key_int(0, 1, t) for t in (0, 1)] == [0xe220a8397b1dcdaf, 0x2d0f28c7e7e786b2]
    assert er.key_int(7, 3, 2) == 0xd3a8307ee11bd937
    assert np.argsort(er.keys(0, 1, 8), kind="stable").tolist() == [7, 3, 1, 2, 5, 4, 6, 0]
    for seed, s, n in ((0, 1, 8), (7, 3, 5), ((1 << 64) - 1, 1023, 300), (0x0123456789ABCDEF, 99, 70)):
        want = [er.key_int(seed, s, t) for t in range(n)]
        assert [int(v) for v in er.keys(seed, s, n)] == want                      # uint64 arrays against Python integers
        got = wsi.relabel_keys(seed, s, n)
        assert got.dtype == np.uint64 and [int(v) for v in got] == want           # the product's


def labels_case(M=300, C=3, seed=5):
    rng = np.random.default_rng(seed)
    cls = rng.integers(0, C, M)
    cls[rng.uniform(size=M) < 0.1] = -1
    return cls


def test_every_column_keeps_the_class_totals_and_column_0_is_observed():
    cls = labels_case()
    tab = wsi.relabel_table(cls, 3, 40, 11)
    assert tab.dtype == np.uint8 and tab.shape == (300, 41)
    np.testing.assert_array_equal(tab, er.table(cls, 3, 40, 11))
    counted = cls >= 0
    np.testing.assert_array_equal(tab[counted, 0], cls[counted])
    assert (tab[~counted] == 255).all() and (~counted).sum() > 10                 # rows that are not counted get 255
    totals = np.bincount(cls[counted], minlength=3)
    for s in range(41):
        np.testing.assert_array_equal(np.bincount(tab[counted, s], minlength=3), totals)
    assert sum((tab[:, s] != tab[:, 0]).any() for s in range(1, 41)) == 40       # and every simulation moved some label
    assert len({tab[:, s].tobytes() for s in range(41)}) == 41


def test_seeds():
    cls = labels_case()
    a, b, again = wsi.relabel_table(cls, 3, 9, 1), wsi.relabel_table(cls, 3, 9, 2), wsi.relabel_table(cls, 3, 9, 1)
    assert a.tobytes() == again.tobytes() and (a[:, 1:] != b[:, 1:]).any() and (a[:, 0] == b[:, 0]).all()
    np.testing.assert_array_equal(wsi.relabel_table(cls, 3, 4, 1), a[:, :5])     # a column depends on (seed, s, t) alone
    big = wsi.relabel_table(cls, 3, 3, (1 << 64) - 1)
    np.testing.assert_array_equal(big, er.table(cls, 3, 3, (1 << 64) - 1))
    # labels outside 0 .. C-1 are rows that are not counted; an empty table and a table without counted rows are legal
    odd = wsi.relabel_table(np.array([0, 5, 1, -3, 1]), 2, 2, 0)
    assert (odd[[1, 3]] == 255).all() and sorted(odd[[0, 2, 4], 1].tolist()) == [0, 1, 1]
    assert wsi.relabel_table(np.zeros(0, np.int64), 2, 3, 0).shape == (0, 4)
    assert (wsi.relabel_table(np.full(4, -1), 2, 3, 0) == 255).all()
    for bad in (lambda: wsi.relabel_table(cls, 3, 0, 0), lambda: wsi.relabel_table(cls, 3, 1024, 0), lambda: wsi.relabel_table(cls, 3, 3, -1),
                lambda: wsi.relabel_table(cls, 3, 3, 1 << 64), lambda: wsi.relabel_table(cls, 9, 3, 0), lambda: wsi.relabel_table(cls.astype(float), 3, 3, 0)):
        with pytest.raises(ValueError):
            bad()


# ---- 2. the restatement's two formulations --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,S,border", [(1, 2, True), (2, 3, True), (40, 5, True), (64, 4, False)])
def test_the_two_formulations_agree(M, S, border):
    H, W, C = 320, 420, 3
    rows = sr.clustered_rows(M, 50 + M, C=C, bad=0.15)
    rows[:, :4] *= np.float32(0.1)                                                # the large slide's pattern on a small one: crowded
    rq = sr.radii_q((4, 10, 30, 90))
    cls = sr.positions(rows, H, W, C, 0.5)[2]
    tab = er.table(cls, C, S, 3)
    roi = sr.roi_q((60, 50, 350, 260), H, W)
    for r in (None, roi):
        got = er.sim_counts(rows, H, W, C, 0.5, rq, tab, r, border)
        want = er.sim_counts_by_definition(rows, H, W, C, 0.5, rq, tab, r, border)
        for g, w in zip(got[:3], want):
            np.testing.assert_array_equal(g, w)
        plain = sr.pair_counts(rows, H, W, C, 0.5, rq, r, border)                 # column 0 is the plain rule
        np.testing.assert_array_equal(got[0][0], plain[0]), np.testing.assert_array_equal(got[1][0], plain[1])
        np.testing.assert_array_equal(got[3], plain[3]), np.testing.assert_array_equal(got[4], plain[4])
    if M >= 40:
        assert got[0].sum() > 0 and (got[0][1:] != got[0][0]).any()


def test_the_two_formulations_agree_with_a_mask_and_with_bad_table_values():
    H, W, C, cell = 200, 260, 2, 16
    rng = np.random.default_rng(8)
    rows = er.square_points(np.round(rng.uniform(5, [255, 195], (60, 2)) * 4) / 4, rng.integers(0, 2, 60))
    rows[5, 6], rows[9, 4] = 7, 0.1                                               # a flagged row and one below
    mask = swr.blob_mask(*swr.grid_of(H, W, cell), seed=3, holes=2)
    rq = sr.radii_q((5, 12, 40))
    cls = sr.positions(rows, H, W, C, 0.5)[2]
    tab = er.table(cls, C, 4, 21)
    tab[[5, 9]] = (3, 0, 1, 200, 2)                                               # garbage on rows that are not counted
    tab[12, 2], tab[30, 2], tab[31, 4] = 2, 255, 9                                # values >= C on counted rows, in simulations 2 and 4
    for m in (None, mask):
        got = er.sim_counts(rows, H, W, C, 0.5, rq, tab, None, True, m, cell)
        want = er.sim_counts_by_definition(rows, H, W, C, 0.5, rq, tab, None, True, m, cell)
        for g, w in zip(got[:3], want):
            np.testing.assert_array_equal(g, w)
        assert got[4][2 * C + 2] & er.FLAG_LABEL and got[0].sum() > 0
        assert got[2][2].sum() == got[2][0].sum() - 2 or m is not None            # two rows fewer inside in simulation 2 (rectangle)
    clean = er.table(cls, C, 4, 21)
    assert not er.sim_counts(rows, H, W, C, 0.5, rq, clean)[4][2 * C + 2] & er.FLAG_LABEL


# ---- 3. the product's host formulas against the loops ---------------------------------------------------------------------------------
def assert_envelope(got, want):
    for key in ("K_sim", "L_minus_r_sim", "K_lo", "K_hi", "L_lo", "L_hi", "outside", "T", "p_mad"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)           # NaN positions included
    for key in ("K_mean", "L_mean"):
        np.testing.assert_allclose(got[key], want[key], rtol=1e-13, atol=0, err_msg=key)


@pytest.mark.parametrize("rank", [1, 2, 4])
def test_envelope_summaries_against_the_loops(rank):
    H, W, C = 480, 630, 3
    rows = sr.clustered_rows(150, 9, C=C)
    rows[:, :4] *= np.float32(0.15)
    rq = sr.radii_q((4, 10, 30, 90))
    cls = sr.positions(rows, H, W, C, 0.5)[2]
    cls2 = np.where(cls == 2, -1, cls)                                            # class 2 without rows: NaN rows and columns
    rows[cls == 2, 4] = 0.0
    sp, sc, si, _, _ = er.sim_counts(rows, H, W, C, 0.5, rq, er.table(cls2, C, 9, 4))
    want = er.envelope_loops(sp, sc, si, rq, 123456.0, rank)
    got = wsi.envelope_summaries(sp, sc, si, rq, 123456.0, rank)
    assert_envelope(got, want)
    assert np.isnan(want["p_mad"][2]).all() and np.isfinite(want["p_mad"][:2, :2]).all() and np.isnan(want["K_lo"]).any()
    assert (want["K_lo"][:2, :2] <= want["K_hi"][:2, :2]).all() and (want["K_lo"][:2, :2] < want["K_hi"][:2, :2]).any()
    zero = wsi.envelope_summaries(sp, sc, si, rq, 0.0, rank)                     # no area: NaN everywhere, nothing outside
    assert np.isnan(zero["K_sim"]).all() and np.isnan(zero["p_mad"]).all() and not zero["outside"].any()
    assert_envelope(zero, er.envelope_loops(sp, sc, si, rq, 0.0, rank))


# ---- 4. argument checks that need no device -------------------------------------------------------------------------------------------
def test_spatial_envelope_refuses_bad_arguments_before_any_launch():
    rows = np.zeros((3, 7), np.float32)
    ok = dict(rows=rows, slide_hw=(100, 100), radii=(4, 8))
    for kw in (dict(num_classes=1), dict(num_classes=9), dict(n_sim=0), dict(n_sim=1024), dict(n_sim=9.0), dict(rank=0), dict(n_sim=99, rank=50),
               dict(n_sim=1, rank=2), dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5), dict(seed=True)):
        with pytest.raises(ValueError, match="spatial_envelope"):
            wsi.spatial_envelope(**{**ok, **kw})
    with pytest.raises(ValueError):
        wsi.spatial_envelope(rows, (100, 100), (8, 4))                            # everything spatial_stats refuses
    with pytest.raises(ValueError):
        wsi.spatial_envelope(rows, (100, 100), (4, 8), window=np.ones((7, 7), bool))
    assert wsi.PAIR_RELABEL_MAX_SIMS == 1024 and wsi.PAIR_RELABEL_FLAG_LABEL == 4


def test_quantify_region_refuses_an_envelope_without_radii():
    raster = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(ValueError, match="spatial_envelope needs spatial_radii"):
        wsi.quantify_region(None, raster, cell=16, field=1, top_k=1, spatial_envelope=19)
    for kw in (dict(spatial_envelope=0), dict(spatial_envelope=19, spatial_rank=10), dict(spatial_envelope=19, spatial_seed=-1)):
        with pytest.raises(ValueError, match="quantify_region"):
            wsi.quantify_region(None, raster, cell=16, field=1, top_k=1, spatial_radii=(4, 8), **kw)


# ---- 5. does the test say what it should: two patterns on the restatement alone --------------------------------------------------------
RADII = (8, 16, 32, 64)


def test_attraction_is_found():
    """two class-1 points next to every class-0 point: the cross K lies above every simulation at every radius, and so does the K of
    either class with itself (a class is then no random subset of all points)"""
    res = er.envelope(er.attraction_rows(), 1024, 1024, 2, RADII, 99, 0)
    np.testing.assert_array_equal(res["p_mad"], np.full((2, 2), 1 / 100))
    assert res["outside"][0, 1].all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_labels_are_not(seed):
    res = er.envelope(er.random_label_rows(), 1024, 1024, 2, RADII, 99, seed)
    assert (res["p_mad"] > 0.05).all(), res["p_mad"]
    assert not res["outside"].any()


# ---- 6. the cost script -----------------------------------------------------------------------------------------------------------------
def test_the_cost_script_shows_its_help_without_a_device(monkeypatch, capsys):
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts", "cost_spatial_envelope.py")
    assert "import harness" in open(path).read()
    monkeypatch.setattr(sys, "argv", [path, "--help"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(path, run_name="__main__")
    assert e.value.code == 0 and "usage:" in capsys.readouterr().out
