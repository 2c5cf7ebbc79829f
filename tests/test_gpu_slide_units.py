"""The second work unit of a workgroup (-m gpu).  Every slide-level kernel caps its grid and lets a workgroup (a wavefront in the box
walk, a group of 16 lanes in the pair search) loop over what is left, carrying LDS tables, pending counters, registers and barriers
from one trip to the next; the neighbouring test modules run every such loop body once per workgroup.  Here each input is the smallest
that reaches the second trip (and, for the LDS histograms, the flush in the middle of a run), and every test first asserts from
tests/slide_units_reference.py -- the launch geometry restated -- that it does.  Every comparison is exact (integers, bytes) against the
NumPy references of the neighbouring modules; every call runs twice into fresh outputs with guard words behind them.

Deliberately not here:
  * launches that are not capped (the seam merge, the slide match's bin / scatter / match, the pair count and scatter);
  * n_xc >= 2 TOGETHER with more than 2 048 units for the load and histogram kernels: rasters of 200 MB to 1.6 GB.  n_xc = 2 is
    covered at one trip by the "rows longer than a work unit" tests of test_gpu_load / test_gpu_stain / test_gpu_stain_basis;
  * the block loop of the views cut (region_tiles_views_u8_kernel, cap 2^20 workgroups: more than a million 32 x 32 blocks) and the
    row loop of view_votes_kernel, whose LDS state is per chunk of detections, not per trip.
The stateless element loops of ay_cut.h, ay_ingest.hip and ay_views.hip (cap 8 192 x 256 threads): checked, and NOT passed by the tests
that were there -- test_gpu_parity's 2 x 1024^2 ingest is exactly 8 192 x 256 elements, one trip; the cut kernels run at S <= 128 and
ay_unview_rows on a few hundred rows -- so section 10 below holds one exact case per loop at the smallest size that passes the cap."""
import time

import numpy as np
import pytest
import torch

import focus_reference as fr
import load_reference as lr
import segment_reference as sg
import slide_units_reference as su
import spatial_reference as sp
import stain_basis_reference as br
import stain_reference as sref
import tissue_reference as tr
import views_reference as vr
from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.datasets import ingest_tiles_device
from amyloid_yolo_paper_amd.views import unview_rows_device
from amyloid_yolo_paper_amd.wsi import StainMap, pair_counts_device, segment_boxes
from oracle.ingest_oracle import ingest
from test_gpu_stain import placed

pytestmark = pytest.mark.gpu

GUARD = 16
IDENTITY = StainMap.identity()                    # kept alive: its params tensor is what the calls read
TABLES = sref.tables()
BQ = br.beta_q()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def basis_params(dev):
    return wsi._params_to_device(wsi.basis_tables(), dev)


def guarded(dev, n, dtype=torch.int64, fill=0):
    """n words of `fill` with GUARD words of -7 behind them"""
    t = torch.full((n + GUARD,), -7, device=dev, dtype=dtype)
    t[:n] = fill
    return t


def strides(r):
    """(base, pad) of the tight stride (byte loads) and of the next multiple of 16 bytes (16-byte loads)"""
    assert (3 * r.shape[1]) % 16
    return (0, 0), (0, 16 - (3 * r.shape[1]) % 16)


def twice(dev, n, call, what, dtype=torch.int64, fill=0):
    """call(out) twice into fresh guarded outputs: the same bytes, the guard words untouched -> the n words"""
    runs = []
    for _ in range(2):
        out = guarded(dev, n, dtype, fill)
        assert call(out) == 0, what
        runs.append(out.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes(), what
    assert (runs[0][n:] == -7).all(), what
    return runs[0][:n].astype(np.int64)


# ---- 1. load cells ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_load_cells_on_the_second_and_third_unit_of_a_workgroup(dev, shrink):
    """37 pixels x 70 331 rows: 4 396 units for 2 048 workgroups; cell 24 against bands of 16: a unit lies in one or two cell rows, and
    both rows of the LDS table are used and zeroed again trip after trip"""
    H, W, cell = su.STRIP_H, su.STRIP_W, 24
    _, n_xc, units, blocks = su.slide_units(W, shrink, H, *su.LOAD)
    assert n_xc == 1 and su.trips(units, blocks) == (2, 3) and cell % 16
    r = su.strip_raster(shrink)
    assert r.shape[:2] == su.source_shape(H, W, shrink)
    t0 = time.perf_counter()
    want, _, _ = lr.load(r, shrink, su.BG, TABLES, 1, sg.THRES_BIN, cell)
    print(f"load reference {time.perf_counter() - t0:.2f} s")
    assert 0 < want[:, :, 1].sum() < want[:, :, 0].sum() < H * W and (want[:, :, 0] > 0).all()
    for base, pad in strides(r):
        buf, stride = placed(dev, r, base, pad)
        got = twice(dev, want.size, lambda out: _lib.lib().ay_stain_load_u8(
            ptr(buf), r.shape[0], r.shape[1], stride, shrink, 0, 0, H, W, su.BG, ptr(IDENTITY.params), 1, sg.THRES_BIN, cell, ptr(out), None, 0,
            None, None, _lib.stream_ptr()), (shrink, pad))
        assert np.array_equal(got.reshape(want.shape), want), (shrink, pad)


# ---- 2. histogram, moments, direction histogram --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_histogram_passes_on_the_second_and_third_unit_of_a_workgroup(dev, basis_params, shrink):
    """the same raster: the LDS histograms and the lane's count, the moments' registers, carried over two or three units"""
    H, W = su.STRIP_H, su.STRIP_W
    _, n_xc, units, blocks = su.slide_units(W, shrink, H, *su.HIST)
    assert n_xc == 1 and su.trips(units, blocks) == (2, 3) and su.trips(units, blocks)[1] < su.HIST_FLUSH
    r = su.strip_raster(shrink)
    t0 = time.perf_counter()
    want_h = sref.hist(r, shrink, su.BG, TABLES)
    t1 = time.perf_counter()
    want_m = br.moments(r, shrink, su.BG, BQ)
    eq1, eq2, _ = br.plane(want_m)
    want_d = br.direction_hist(r, shrink, su.BG, BQ, eq1, eq2)
    print(f"hist reference {t1 - t0:.2f} s, moments and direction reference {time.perf_counter() - t1:.2f} s")
    assert 0 < want_h[1024] < H * W and 0 < want_m[1] < want_m[0] == want_h[1024] and want_d[513] == want_m[1] and (want_d[:512] > 0).sum() > 100
    L, s = _lib.lib(), _lib.stream_ptr()
    plane = [int(v) for v in eq1] + [int(v) for v in eq2]
    for base, pad in strides(r):
        buf, stride = placed(dev, r, base, pad)
        head = (ptr(buf), r.shape[0], r.shape[1], stride, shrink, su.BG)
        got = twice(dev, 1025, lambda out: L.ay_stain_hist_u8(*head, ptr(IDENTITY.params), ptr(out), s), ("hist", shrink, pad))
        assert np.array_equal(got, want_h), ("hist", shrink, pad)
        got = twice(dev, 11, lambda out: L.ay_stain_moments_u8(*head, BQ, ptr(basis_params), ptr(out), s), ("moments", shrink, pad))
        assert np.array_equal(got, want_m), ("moments", shrink, pad)
        got = twice(dev, 514, lambda out: L.ay_stain_direction_hist_u8(*head, BQ, *plane, ptr(basis_params), ptr(out), s), ("direction", shrink, pad))
        assert np.array_equal(got, want_d), ("direction", shrink, pad)


# ---- 3. the flush in the middle of a run -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def column(dev):
    """the 201 MB column, resident once for both tests"""
    col = su.flush_column()[0]
    d = torch.from_numpy(col.reshape(-1)).to(dev)                 # (flush_column leaves the column writable: no copy on the host)
    assert d.data_ptr() % 16 == 0
    yield d
    del d
    torch.cuda.empty_cache()


def flush_geometry():
    _, n_xc, units, blocks = su.slide_units(1, 1, su.FLUSH_H, *su.HIST)
    lo, hi = su.trips(units, blocks)
    # every workgroup flushes after its unit 2 048 and has at least one unit left, and none flushes twice before its end
    assert n_xc == 1 and blocks == su.CAP and lo - su.HIST_FLUSH >= 1 and hi - su.HIST_FLUSH <= 2 and hi < 2 * su.HIST_FLUSH


def test_histogram_flush_in_the_middle_of_a_run(dev, column):
    """one pixel x 67 141 776 rows (3-byte rows, byte loads): 2 048 x 2 048 + 2 048 + 9 units, so every workgroup reaches pending ==
    HIST_FLUSH once, flushes, zeroes, and counts one or two more units into the zeroed bins"""
    flush_geometry()
    _, block, reps, rem = su.flush_column()
    want = reps * sref.hist(block, 1, su.BG, TABLES) + sref.hist(block[:rem], 1, su.BG, TABLES)
    tissue = reps * int(tr.tissue(block, 1, su.BG).sum()) + int(tr.tissue(block[:rem], 1, su.BG).sum())
    assert 0 < tissue < su.FLUSH_H and tissue > 2 ** 25
    t0 = time.perf_counter()
    got = twice(dev, 1025, lambda out: _lib.lib().ay_stain_hist_u8(ptr(column), su.FLUSH_H, 1, 3, 1, su.BG, ptr(IDENTITY.params), ptr(out),
                                                                     _lib.stream_ptr()), "flush")
    print(f"two histogram runs {time.perf_counter() - t0:.2f} s")
    assert got[1024] == tissue == got[:512].sum() == got[512:1024].sum()            # the total word is the tissue pixel count
    assert np.array_equal(got, want)


def test_direction_histogram_flush_in_the_middle_of_a_run(dev, basis_params, column):
    flush_geometry()
    _, block, reps, rem = su.flush_column()
    eq1, eq2, _ = br.plane(br.moments(block, 1, su.BG, BQ))
    want = reps * br.direction_hist(block, 1, su.BG, BQ, eq1, eq2) + br.direction_hist(block[:rem], 1, su.BG, BQ, eq1, eq2)
    selected = reps * len(br.selected(block, 1, su.BG, BQ)[1]) + len(br.selected(block[:rem], 1, su.BG, BQ)[1])
    assert 0 < selected and (want[:512] > 0).sum() > 50
    plane = [int(v) for v in eq1] + [int(v) for v in eq2]
    got = twice(dev, 514, lambda out: _lib.lib().ay_stain_direction_hist_u8(ptr(column), su.FLUSH_H, 1, 3, 1, su.BG, BQ, *plane, ptr(basis_params),
                                                                              ptr(out), _lib.stream_ptr()), "flush")
    assert got[513] == selected == got[:513].sum()                                  # the total word is the selected pixel count
    assert np.array_equal(got, want)


# ---- 4. focus cells ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,shrink", [("a", 1), ("a", 2), ("b", 1), ("c", 1)])
def test_focus_cells_on_the_second_unit_of_a_workgroup(dev, case, shrink):
    """(a) 40 x 140 667, cell 48: 4 396 units one across; the cell row changes inside the rows of a lane in two units of three, so the
    spill path and all three rows of the LDS table run trip after trip.  (b) 520 x 32 967: two units across (32 items, 1 item) and
    2 062 units; 2 048 is even, so the units of ONE workgroup are equally wide.  (c) 1 030 x 22 089: three units across (32, 32, 1
    items); 2 048 is no multiple of 3, so for two workgroups in three the second unit has another width than the first (32 then 1, 1 then
    32): the lanes behind wq, the halo columns and the table's used part change between the trips."""
    W, H, cell = {"a": su.FOCUS_A, "b": su.FOCUS_B, "c": su.FOCUS_C}[case]
    nq, n_xc, units, blocks = su.focus_units(W, shrink, H)
    assert n_xc == {"a": 1, "b": 2, "c": 3}[case] and su.trips(units, blocks)[1] >= 2 and (case != "a" or su.trips(units, blocks) == (2, 3))
    if case == "c":
        assert all(su.unit_wq(u, n_xc, nq, 32) != su.unit_wq(u + su.CAP, n_xc, nq, 32) or u % 3 == 1 for u in range(units - su.CAP))
        assert {su.unit_wq(u, n_xc, nq, 32) for u in range(su.CAP, units)} == {1, 32}
    r = su.focus_raster(case, shrink)
    assert r.shape[:2] == su.source_shape(H, W, shrink)
    t0 = time.perf_counter()
    want, _, _ = fr.focus(r, shrink, su.BG, cell)
    print(f"focus reference {time.perf_counter() - t0:.2f} s")
    assert 0 < want[:, :, 0].sum() < (H - 2) * (W - 2) and (want[:, :, 1] < 0).any() and (want[:, :, 1] > 0).any() and (want[:, :, 0] > 0).mean() > 0.9
    for base, pad in strides(r):
        buf, stride = placed(dev, r, base, pad)
        got = twice(dev, want.size, lambda out: _lib.lib().ay_focus_u8(
            ptr(buf), r.shape[0], r.shape[1], stride, shrink, 0, H, W, 0, H, su.BG, cell, ptr(out), None, 0, None, None, _lib.stream_ptr()),
                    (case, shrink, pad))
        assert np.array_equal(got.reshape(want.shape), want), (case, shrink, pad)


# ---- 5. tile tissue ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
@pytest.mark.parametrize("side,tile,step", su.TISSUE_CASES)
def test_tile_tissue_on_the_second_unit_of_a_workgroup(dev, side, tile, step, shrink):
    """15 876 and 8 464 units for 8 192 workgroups; with tile 24 and step 16 every unit adds to two or four tiles, and units without a
    tile `continue` between the trips"""
    m, _, _, _, units, blocks = su.tissue_units(side, side, tile, step)
    assert units > blocks == su.TISSUE_CAP and su.trips(units, blocks) == (1, 2) and m == (2 if tile != step else 1)
    r = su.tissue_raster(side, shrink)
    assert r.shape[:2] == su.source_shape(side, side, shrink)
    ty, tx, st = tr.grid(side, side, tile, tile - step)
    assert st == step
    t0 = time.perf_counter()
    want = tr.tissue_counts(r, tile, shrink, tile - step, su.BG)
    print(f"tissue reference {time.perf_counter() - t0:.2f} s")
    assert want.shape == (ty, tx) and 0 < want.min() and want.max() < tile * tile
    for base, pad in strides(r):
        buf, stride = placed(dev, r, base, pad)
        got = twice(dev, ty * tx, lambda out: _lib.lib().ay_tile_tissue_u8(ptr(buf), r.shape[0], r.shape[1], stride, shrink, tile, step, ty, tx,
                                                                            su.BG, ptr(out), _lib.stream_ptr()), (side, shrink, pad),
                    dtype=torch.int32, fill=-3)                       # the call zeroes what it counts into
        assert np.array_equal(got.reshape(ty, tx), want), (side, shrink, pad)


# ---- 6. the box walk -----------------------------------------------------------------------------------------------------------------------
def box_geometry(M, k):
    assert su.box_walk_waves(M) == su.BOX_CAP and su.trips(M, su.BOX_CAP) == (2, 3) and k + 2 * su.BOX_CAP < M


def test_load_boxes_on_the_second_and_third_box_of_a_wavefront(dev):
    """2 x 8 192 + 77 boxes for 8 192 wavefronts; one wavefront's three boxes are a NaN row, an empty row and a row off the slide
    (`continue`, `continue`, `continue`), its neighbour's an inverted row and two ordinary boxes; one call, and three uneven strips"""
    r, rows, k = su.box_case()
    H, W = su.BOX_HW
    M = len(rows)
    box_geometry(M, k)
    d_rows = torch.from_numpy(np.array(rows)).to(dev)
    rd = torch.from_numpy(np.array(r)).to(dev)
    t0 = time.perf_counter()
    _, want, want_f = lr.load(r, 1, su.BG, TABLES, 1, sg.THRES_BIN, 24, rows)
    print(f"load box reference {time.perf_counter() - t0:.2f} s")
    three = [k, k + su.BOX_CAP, k + 2 * su.BOX_CAP]
    assert want_f[0] == lr.FLAG_NONFINITE and (want[three] == 0).all() and (want[k + 1] == 0).all() and (want[[k + 1 + su.BOX_CAP, k + 1 + 2 * su.BOX_CAP], 0] > 0).all()
    assert 0 < want[:, 2].sum() < want[:, 1].sum() < want[:, 0].sum() and np.array_equal(want[:, 0], lr.owned_pixels(rows, H, W))
    for cuts in ((), (13, 14)):
        bounds = [0, *cuts, H]
        runs = []
        for _ in range(2):
            boxes, flags = guarded(dev, M * 4), torch.tensor([0, -7], device=dev, dtype=torch.int32)
            for a, b in zip(bounds[:-1], bounds[1:]):
                assert _lib.lib().ay_stain_load_u8(ptr(rd[a:b]), b - a, W, W * 3, 1, a, 0, H, W, su.BG, ptr(IDENTITY.params), 1, sg.THRES_BIN, 24,
                                                   None, ptr(d_rows), M, ptr(boxes), ptr(flags), _lib.stream_ptr()) == 0
            runs.append(boxes.cpu().numpy())
            assert flags.tolist() == [lr.FLAG_NONFINITE, -7]
        assert runs[0].tobytes() == runs[1].tobytes() and (runs[0][M * 4:] == -7).all(), cuts
        bad = np.flatnonzero((runs[0][:M * 4].reshape(M, 4) != want).any(1))
        assert len(bad) == 0, (cuts, bad[:8], bad // su.BOX_CAP)


def test_focus_boxes_on_the_second_and_third_box_of_a_wavefront(dev):
    r, rows, k = su.box_case()
    H, W = su.BOX_HW
    M = len(rows)
    box_geometry(M, k)
    d_rows = torch.from_numpy(np.array(rows)).to(dev)
    rd = torch.from_numpy(np.array(r)).to(dev)
    t0 = time.perf_counter()
    _, want, want_f = fr.focus(r, 1, su.BG, 24, rows)
    print(f"focus box reference {time.perf_counter() - t0:.2f} s")
    assert want_f[0] == fr.FLAG_NONFINITE and (want[[k, k + su.BOX_CAP, k + 2 * su.BOX_CAP, k + 1]] == 0).all() and (want[:, 0] > 0).sum() > 0.5 * M
    for ranges in (((0, H),), ((0, 13), (13, 14), (14, H))):
        runs = []
        for _ in range(2):
            boxes, flags = guarded(dev, M * 3), torch.tensor([0, -7], device=dev, dtype=torch.int32)
            for a, b in ranges:
                lo, hi = max(a, 1) - 1, min(b, H - 1)               # the rows the call needs
                assert _lib.lib().ay_focus_u8(ptr(rd[lo:hi + 1]), hi + 1 - lo, W, W * 3, 1, lo, H, W, a, b, su.BG, 24, None, ptr(d_rows), M,
                                              ptr(boxes), ptr(flags), _lib.stream_ptr()) == 0
            runs.append(boxes.cpu().numpy())
            assert flags.tolist() == [fr.FLAG_NONFINITE, -7]
        assert runs[0].tobytes() == runs[1].tobytes() and (runs[0][M * 3:] == -7).all(), ranges
        bad = np.flatnonzero((runs[0][:M * 3].reshape(M, 3) != want).any(1))
        assert len(bad) == 0, (ranges, bad[:8], bad // su.BOX_CAP)


# ---- 7. the segmenter ----------------------------------------------------------------------------------------------------------------------
def segment_geometry():
    assert su.segment_blocks(su.SEG_M) == su.SEG_CAP and su.trips(su.SEG_M, su.SEG_CAP) == (2, 3)
    counts = su.segment_successions(su.segment_want()[0])
    assert min(counts.values()) >= 10, counts                        # (test_slide_units_cpu.py prints them)


def test_segments_of_the_second_and_third_box_of_a_workgroup(dev):
    """2 x 2 048 + 37 rows for 2 048 workgroups, ordered so that what one box leaves in LDS -- `best`, `acc`, the planes beyond the next
    window's words and rows, `parent` -- would show in the next: a large component before a window without a positive pixel, a wide
    window before a narrow short one, a window before each status row, and windows of either instance alternating (so that both
    instances skip and take rows in turn).  One call on the rows [0, 280) of the slide: windows that reach further are NOT_RESIDENT."""
    segment_geometry()
    r, rows = su.segment_raster(), su.segment_rows()
    t0 = time.perf_counter()
    want, want_flags, _, _ = su.segment_want()
    print(f"segment reference {time.perf_counter() - t0:.2f} s")
    M = len(rows)
    region = np.ascontiguousarray(r[:su.SEG_SHORT])
    d_rows = torch.from_numpy(np.array(rows)).to(dev)
    for base, pad in ((0, 0), (5, 7)):
        buf, stride = placed(dev, region, base, pad)
        runs = []
        for _ in range(2):
            out = torch.full((M * sg.COLS + GUARD,), -7, device=dev, dtype=torch.int32)      # never zeroed: a call writes every word it owns
            flags = torch.tensor([0, -7], device=dev, dtype=torch.int32)
            check(_lib.lib().ay_box_segments_u8(ptr(buf), su.SEG_SHORT, su.SEG_W, stride, 1, 0, 0, su.SEG_H, su.SEG_W, 0, su.SEG_H, sg.BG,
                                                ptr(IDENTITY.params), 1, sg.THRES_BIN, sg.CORE_BIN, su.SEG_MARGIN, 1, ptr(d_rows), M, ptr(out),
                                                ptr(flags), _lib.stream_ptr()), "ay_box_segments_u8")
            runs.append(out.cpu().numpy())
            assert flags.tolist() == [want_flags, -7]
        assert runs[0].tobytes() == runs[1].tobytes() and (runs[0][M * sg.COLS:] == -7).all(), (base, pad)
        got = runs[0][:M * sg.COLS].reshape(M, sg.COLS).astype(np.int64)
        bad = np.flatnonzero((got != want).any(1))
        assert len(bad) == 0, (base, pad, len(bad), bad[:8], got[bad[:2]], want[bad[:2]])


def test_segment_boxes_in_strips_of_255_rows(dev):
    """the same rows through wsi.segment_boxes with strip=255: 46 calls, each owning one owner row, so that the owner-row `continue`
    falls between the boxes of one workgroup, before and behind the boxes it takes"""
    segment_geometry()
    _, _, want, want_flags = su.segment_want()
    got = segment_boxes(np.array(su.segment_raster()), np.array(su.segment_rows()), margin=su.SEG_MARGIN, thres=sg.THRES_BIN / 64.0,
                        core_thres=sg.CORE_BIN / 64.0, bg_level=sg.BG, strip=255)
    assert got["strips"][1] == len(sg.strip_plan(su.SEG_H, 255)) == 46 and got["strips"][0] >= 30
    bad = np.flatnonzero((got["segments"].astype(np.int64) != want).any(1))
    assert len(bad) == 0 and got["flags"] == want_flags, (len(bad), bad[:8], got["segments"][bad[:2]], want[bad[:2]])


# ---- 8. the pair search --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pair_want():
    rows, rq = su.pair_rows(), sp.radii_q(su.PAIR_RADII_PX)
    t0 = time.perf_counter()
    want = {border: sp.pair_counts_binned(rows, sp.SLIDE_H, sp.SLIDE_W, su.PAIR_CLASSES, 0.5, rq, None, border) for border in (True, False)}
    print(f"pair reference (both border settings) {time.perf_counter() - t0:.2f} s")
    return rows, rq, want


@pytest.mark.parametrize("border", [True, False])
def test_pair_search_on_the_second_and_third_centre_of_a_group(dev, pair_want, border):
    """71 000 rows, more than 2 x 32 768 + 500 of them counted, for the 32 768 groups of 16 lanes of the capped search launch: a group's
    wtab and wnn are zeroed behind a centre and used again; flagged rows and rows below the threshold are mixed in"""
    rows, rq, want = pair_want
    C_ = su.PAIR_CLASSES
    pairs, centres, nn, bd, stats = want[border]
    counted = int(stats[:C_].sum())
    assert su.pair_groups(len(rows)) == su.PAIR_CAP and su.trips(counted, su.PAIR_CAP)[0] >= 2 and counted >= 2 * su.PAIR_CAP + 500
    assert len(rq) == 4 and stats[2 * C_] > 0 and stats[2 * C_ + 1] > 0 and (pairs > 0).all()
    assert all((nn[:, b, 1] >= 0).any() and (nn[bd >= 0, b, 1] < 0).any() for b in range(C_))          # hits and misses in every class
    assert (centres[:, 0] > centres[:, -1]).all() if border else (centres == centres[:, :1]).all()
    t = torch.from_numpy(np.array(rows)).to(dev)
    runs = []
    for _ in range(2):
        out = pair_counts_device(t, (sp.SLIDE_H, sp.SLIDE_W), rq, C_, 0.5, None, border)
        torch.cuda.synchronize()
        runs.append(tuple(out[k].cpu().numpy() for k in ("pairs", "centres", "nn", "bd", "stats")))
    for name, a, b, w in zip(("pairs", "centres", "nn", "bd", "stats"), runs[0], runs[1], want[border]):
        assert a.tobytes() == b.tobytes(), name
        assert a.dtype == w.dtype and a.shape == w.shape, name
        np.testing.assert_array_equal(a, w, err_msg=f"{name} border={border}")


# ---- 9. stain apply ------------------------------------------------------------------------------------------------------------------------
def test_apply_kernel_beyond_its_grid_cap(dev):
    """1 500 x 1 500 pixels for 8 192 x 256 threads: 152 848 pixels are second trips"""
    n = su.APPLY_SIDE
    assert su.element_threads(n * n) == su.ELEMENT_CAP < n * n
    r = su.content(n, n, 900)
    gains = (1.3, 0.7)
    h = np.zeros((2, 512), np.int64)
    h[:, 63] = 1
    m = StainMap(wsi.StainStats(h, 1), gains, max_gain=4.0)           # exactly these gains: source strengths (1, 1)
    assert m.gains == gains
    t0 = time.perf_counter()
    want = sref.apply(r, 1, sref.tables(gains))
    print(f"apply reference {time.perf_counter() - t0:.2f} s")
    assert (want != r).mean() > 0.25
    for base, pad, opad in ((0, 0, 0), (5, 7, 11)):
        buf, stride = placed(dev, r, base, pad)
        ostride = n * 3 + opad
        runs = []
        for _ in range(2):
            out = torch.full((n * ostride + GUARD,), 99, dtype=torch.uint8, device=dev)
            check(_lib.lib().ay_stain_apply_u8(ptr(buf), n, n, stride, 1, ptr(m.params), ptr(out), ostride, _lib.stream_ptr()), "ay_stain_apply_u8")
            runs.append(out.cpu().numpy())
        assert runs[0].tobytes() == runs[1].tobytes()
        rows = np.lib.stride_tricks.as_strided(runs[0], (n, ostride), (ostride, 1))
        assert np.array_equal(rows[:, :n * 3].reshape(n, n, 3), want), (base, pad, opad)
        assert (rows[:, n * 3:] == 99).all() and (runs[0][n * ostride:] == 99).all()        # row padding and what lies behind: untouched


# ---- 10. the stateless element loops of the cut, the ingest and the unview kernels -----------------------------------------------------------
@pytest.mark.parametrize("S_,shift", [(968, 0), (483, 1)], ids=["S968 vec4", "S483 scalar"])
def test_cut_kernel_beyond_its_grid_cap(dev, S_, shift):
    """nine tiles of 32 pixels cut to S: 9 x 968 x 968 / 4 vectors and 9 x 483 x 483 floats both pass 8 192 x 256 by less than a percent"""
    n, tile = 9, 32
    assert su.element_threads(n * S_ * S_ // (4 if shift == 0 else 1)) == su.ELEMENT_CAP < n * S_ * (S_ // (4 if shift == 0 else 1))
    assert n * S_ * (S_ // (4 if shift == 0 else 1)) < 1.01 * su.ELEMENT_CAP and (S_ % 4 == 0) == (shift == 0)
    r = su.content(70, 100, 901)
    origins = [(0, 0), (32, 0), (64, 0), (0, 32), (32, 32), (80, 32), (1, 2), (-3, 50), (60, -5)]
    want = []
    for x, y in origins:                                            # a 255-padded crop, then the oracle's nearest resize
        t = np.full((tile, tile, 3), 255, np.uint8)
        c = r[max(y, 0):max(y + tile, 0), max(x, 0):max(x + tile, 0)]
        t[max(-y, 0):max(-y, 0) + c.shape[0], max(-x, 0):max(-x, 0) + c.shape[1]] = c
        want.append(ingest(t, S_))
    want = torch.stack(want)
    rd = torch.from_numpy(np.array(r)).to(dev)
    o = torch.tensor(origins, dtype=torch.int32, device=dev)
    total = want.numel()
    runs = []
    for _ in range(2):
        buf = torch.full((GUARD + shift + total + GUARD,), -7.0, device=dev)
        assert buf.data_ptr() % 16 == 0
        check(_lib.lib().ay_ingest_region_tiles_list_u8(ptr(rd), 70, 100, 300, 1, tile, ptr(o), n, S_, ptr(buf[GUARD + shift:]), _lib.stream_ptr()),
              "ay_ingest_region_tiles_list_u8")
        runs.append(buf.cpu())
    assert torch.equal(runs[0], runs[1])
    got = runs[0]
    assert (got[:GUARD + shift] == -7.0).all() and (got[GUARD + shift + total:] == -7.0).all()
    assert torch.equal(got[GUARD + shift:GUARD + shift + total].view_as(want), want)


def test_ingest_kernel_beyond_its_grid_cap(dev):
    """three tiles to 837 x 837: 3 x 837^2 = 2 101 707 elements, 4 555 more than 8 192 x 256"""
    B, S_ = 3, 837
    assert su.element_threads(B * S_ * S_) == su.ELEMENT_CAP < B * S_ * S_ and B * (S_ - 1) ** 2 <= su.ELEMENT_CAP
    tiles = np.stack([su.content(37, 53, 910 + b) for b in range(B)])
    runs = [ingest_tiles_device(tiles, S_).cpu() for _ in range(2)]
    assert torch.equal(runs[0], runs[1])
    for b in range(B):
        assert torch.equal(runs[0][b], ingest(tiles[b], S_)), b


def test_unview_rows_beyond_its_grid_cap(dev):
    """16 images (two of every view) of 131 100 rows: 2 097 600 rows, 448 more than 8 192 x 256"""
    views, n_images, N, K = tuple(range(8)), 16, 131100, 6
    assert su.element_threads(n_images * N) == su.ELEMENT_CAP < n_images * N
    rng = np.random.default_rng(920)
    pred = rng.uniform(-100.0, 520.0, (n_images, N, K)).astype(np.float32)
    want = vr.unview_rows(pred, views, 416)
    runs = []
    for _ in range(2):
        buf = torch.full((pred.size + GUARD,), -7.0, device=dev)
        t = buf[:pred.size].view(n_images, N, K)
        t.copy_(torch.from_numpy(pred))
        assert unview_rows_device(t, views, 416) is t
        runs.append(buf.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes() and (runs[0][pred.size:] == -7.0).all()
    assert runs[0][:pred.size].reshape(pred.shape).tobytes() == want.tobytes()
