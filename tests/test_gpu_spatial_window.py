"""Spatial statistics inside a tissue-shaped window (-m gpu): ay_pair_counts_window through wsi.pair_counts_device(window=...),
wsi.spatial_stats(window=...) and quantify_region(spatial_window=True).  Every output -- pairs, centres, nn, bd, stats -- is compared
byte for byte: THE PAIR WINDOW RULE is THE PAIR RULE's two fp32 operations and integers after them.

Yardstick: tests/spatial_window_reference.py (the distance to every OUT cell by brute force, the pairs by brute force)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spatial_reference as sr
import spatial_window_reference as wr
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ptr
from amyloid_yolo_paper_amd.wsi import pair_counts_device, quantify_region, spatial_stats, window_from_tissue

pytestmark = pytest.mark.gpu

H, W, NC, CELL = wr.SLIDE_H, wr.SLIDE_W, wr.CLASSES, wr.CELL
NAMES = ("pairs", "centres", "nn", "bd", "stats")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def run(dev, rows, H_, W_, C_, min_conf, rq, mask=None, cell=0, roi=None, border=True, cell_side=0):
    t = torch.from_numpy(np.array(rows, np.float32)).reshape(-1, 7).to(dev)      # (a copy: the shared cases are read-only)
    m = None if mask is None else torch.from_numpy(np.array(mask, np.uint8)).to(dev)
    out = pair_counts_device(t, (H_, W_), rq, C_, min_conf, roi, border, cell_side, m, cell)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in NAMES)


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
        assert g.tobytes() == w.tobytes(), (what, name)


def against_the_reference(dev, rows, H_, W_, C_, min_conf, rq, mask, cell, roi=None, border=True, cell_side=0, what=""):
    want = wr.pair_counts_window(rows, H_, W_, C_, min_conf, rq, mask, cell, roi, border)
    assert_same(run(dev, rows, H_, W_, C_, min_conf, rq, mask, cell, roi, border, cell_side), want, what)
    return want


# ---- 1. an all-IN mask is the rectangle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Hs,Ws", [(384, 512), (390, 500)])
@pytest.mark.parametrize("cell", [16, 32])
def test_an_all_in_mask_equals_the_plain_call_with_bd_capped(dev, Hs, Ws, cell):
    rows = wr.ragged_rows(257, 31, Hs, Ws, 3)
    rq = sr.radii_q((3, 10.5, 40))
    mask = np.ones(wr.grid_of(Hs, Ws, cell), np.uint8)
    for border in (True, False):
        plain = run(dev, rows, Hs, Ws, 3, 0.5, rq, border=border)
        got = run(dev, rows, Hs, Ws, 3, 0.5, rq, mask, cell, border=border)
        assert (plain[3] > rq[-1]).any() and plain[0][:, :, -1].min() > 0
        capped = np.where(plain[3] >= 0, np.minimum(plain[3], rq[-1]), -1).astype(np.int32)
        assert_same(got, (plain[0], plain[1], plain[2], capped, plain[4]), f"all IN, cell {cell}, border={border}")
    assert_same(got, wr.pair_counts_window(rows, Hs, Ws, 3, 0.5, rq, mask, cell, None, False), "all IN against the restatement")


# ---- 2. a ragged mask ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("border", [True, False])
@pytest.mark.parametrize("M", wr.SIZES)
def test_ragged_case_against_the_restatement(dev, M, border):
    rows, rq, mask, want = wr.ragged_case(M, border)           # (check_not_idle ran on the restatement for M >= 257)
    assert_same(run(dev, rows, H, W, NC, 0.5, rq, mask, CELL, border=border), want, f"M={M} border={border}")


# ---- 3. equality on a diagonal ------------------------------------------------------------------------------------------------------------
def test_a_radius_equal_to_the_distance_is_not_eligible(dev):
    """one OUT cell (gy 10, gx 12: x 768 .. 831, y 640 .. 703 quarter pixels) in an all-IN mask on a 390 x 500 slide (cut last cells).
    Rows whose nearest OUT position is offset by exactly (3n, 4n), n = 5, or (5m, 12m), m = 4, from each corner of the cell, by a
    pure dx or dy of 25 and 52 from its edges, and by 25 and 52 from the slide's right and lower border, which lie beyond cut cells:
    d2out = 25^2 or 52^2, so R = 25 (52) is NOT eligible and R - 1 is"""
    Hs, Ws, cell = 390, 500, 16
    mask = np.ones(wr.grid_of(Hs, Ws, cell), np.uint8)
    mask[10, 12] = 0
    rq = np.array([24, 25, 51, 52], np.int32)
    q, want_bd = [], []
    for cx, sx in ((768, -1), (831, 1)):
        for cy, sy in ((640, -1), (703, 1)):
            for dx, dy, d in ((15, 20, 24), (20, 15, 24), (20, 48, 51), (48, 20, 51)):
                q.append((cx + sx * dx, cy + sy * dy)), want_bd.append(d)
    for d in (25, 52):
        q += [(768 - d, 650), (831 + d, 700), (800, 640 - d), (769, 703 + d), (2000 - d, 300), (300, 1560 - d), (d - 1, 1000), (1500, d - 1)]
        want_bd += [d - 1] * 8
    n_exact = len(q)
    q += [(x + 8, y + 4) for x, y in q] + [(800, 670), (767, 639), (832, 680)]          # partners; a row in the OUT cell, one off its corner, one beside it
    rows = sr.points(np.array(q, np.float64) / 4.0, cls=np.arange(len(q)) % 2)
    for border in (True, False):
        want = against_the_reference(dev, rows, Hs, Ws, 2, 0.0, rq, mask, cell, None, border, what=f"diagonal border={border}")
    want = wr.pair_counts_window(rows, Hs, Ws, 2, 0.0, rq, mask, cell)
    assert want[3][:n_exact].tolist() == want_bd                 # wbd = R - 1 where d2out == R^2
    assert want[3][-3:].tolist() == [-1, 1, 0] and want[0].sum() > 0      # d2out 0, 2 and 1
    plain = sr.pair_counts(rows, Hs, Ws, 2, 0.0, rq)
    assert want[1].sum() < plain[1].sum()
    qx, qy = sr.positions(rows, Hs, Ws, 2, 0.0)[:2]
    d2 = wr.d2_out(qx, qy, mask, cell, Hs, Ws)
    assert sorted(set(d2[:n_exact].tolist())) == [25 * 25, 52 * 52]


# ---- 4. degenerate grids ------------------------------------------------------------------------------------------------------------------
def test_degenerate_grids(dev):
    rq = sr.radii_q((2, 7.25, 30))
    for Hs, Ws, cell, masks in ((100, 20, 32, ([[1], [0], [1], [1]], [[1], [1], [1], [1]], [[0], [1], [0], [1]])),          # Gx == 1
                                (20, 100, 32, ([[1, 0, 1, 1]], [[1, 1, 1, 1]], [[0, 1, 1, 0]])),                            # Gy == 1
                                (30, 30, 32, ([[1]], [[0]])), (16, 16, 16, ([[1]],)), (1, 1, 16, ([[1]],))):               # one cell
        rows = wr.ragged_rows(120, 40 + Hs, Hs, Ws, 2)
        rows[:, :4] = np.round(rows[:, :4] / np.float32(3))     # (the generator spreads its clusters over 50 px: pull them together)
        for mask in masks:
            mask = np.array(mask, np.uint8)
            for border in (True, False):
                against_the_reference(dev, rows, Hs, Ws, 2, 0.5, rq, mask, cell, None, border, what=f"{Hs} x {Ws} mask {mask.tolist()} border={border}")
    Hs, Ws, cell = 200, 300, 16                                 # 13 x 19 cells, the last row 8 px and the last column 12 px
    rows = wr.ragged_rows(400, 77, Hs, Ws, 2)
    qx, qy, cls = sr.positions(rows, Hs, Ws, 2, 0.5)[:3]
    assert ((qx == 0) | (qx == 4 * Ws - 1) | (qy == 0) | (qy == 4 * Hs - 1))[cls >= 0].sum() >= 10      # centres outside the slide, clamped
    stripes = np.ones((13, 19), np.uint8)
    stripes[1::2] = 0
    holes = np.ones((13, 19), np.uint8)
    holes[[0, 5, 12, 12, 7], [0, 9, 18, 3, 18]] = 0             # columns 1, 2, 4 .. are all IN: the slide's edges are their only OUT rows
    columns = np.ones((13, 19), np.uint8)
    columns[:, 1::2] = 0
    for name, mask in (("alternating rows", stripes), ("alternating columns", columns), ("a few holes", holes), ("all OUT", np.zeros((13, 19), np.uint8))):
        for border in (True, False):
            want = against_the_reference(dev, rows, Hs, Ws, 2, 0.5, rq, mask, cell, None, border, what=f"{name} border={border}")
        pairs, centres, nn, bd, stats = want
        if name == "all OUT":
            assert centres.sum() == 0 and pairs.sum() == 0 and stats[2:4].sum() == 0 and (bd == -1).all() and (nn[:, :, 1] >= 0).sum() > 300
        else:
            assert centres[:, 0].min() > 0 and set(bd[(cls >= 0) & ((qx == 0) | (qy == 0))].tolist()) <= {-1, 0}
            in_cell = mask[qy // (4 * cell), qx // (4 * cell)] != 0
            out_partner = (cls >= 0) & ~in_cell
            assert out_partner.sum() >= 5 and np.isin(nn[(cls >= 0) & in_cell][:, :, 1], np.flatnonzero(out_partner)).any()   # OUT rows are partners


def test_tall_masks_cross_the_64_row_words(dev):
    """the kernels keep 64 mask rows of a column in one word: 200 and 321 mask rows (4 and 6 words), OUT cells at the words' first and
    last rows and columns that are IN for several words, with radii of 3, 40 and 130 cells so that a search ends inside a word, in the
    next one, two words on, and at its reach with an OUT cell beyond it"""
    cell = 16
    for Gy, Gx, rad_px, seed in ((200, 10, (20, 50.5), 1), (200, 10, (30, 640), 2), (321, 7, (100, 2080), 3), (321, 7, (9, 48), 4)):
        Hs, Ws = cell * Gy - 5, cell * Gx - 3                   # cut last cells
        rng = np.random.default_rng(seed)
        mask = np.ones((Gy, Gx), np.uint8)
        mask[[0, 63, 64, 127, 128, 199], [0, 1, 2, 3, 4, 5]] = 0
        mask[rng.integers(0, Gy, 6), rng.integers(0, Gx, 6)] = 0
        mask[70:75, 6] = 0
        if Gy > 300:
            mask[[255, 256, 320], [0, 3, 6]] = 0
        xy = rng.uniform([-8, -8], [Ws + 8, Hs + 8], (500, 2))
        rows = sr.points(np.round(xy * 4) / 4, cls=np.arange(500) % 2)
        rq = sr.radii_q(rad_px)
        for border in (True, False):
            want = against_the_reference(dev, rows, Hs, Ws, 2, 0.0, rq, mask, cell, None, border, what=f"{Gy} mask rows, radii {rad_px}, border={border}")
        assert len(set(want[3].tolist())) > 50 and want[1].min() >= 0 and (want[3] == -1).any()
        assert (want[3] == rq[-1]).any() == (rad_px[-1] < 100)  # the small radii reach no OUT position from some rows, the large from none


# ---- 5. mask AND ROI ----------------------------------------------------------------------------------------------------------------------
def test_mask_and_roi(dev):
    rows, rq, mask, masked = wr.ragged_case(257)
    roi = np.array([900, 700, 3100, 2500], np.int32)             # cuts through IN cells
    for border in (True, False):
        want = against_the_reference(dev, rows, H, W, NC, 0.5, rq, mask, CELL, roi, border, what=f"roi border={border}")
    rect = sr.pair_counts(rows, H, W, NC, 0.5, rq, roi)
    both = (want[3] >= 0)
    np.testing.assert_array_equal(want[3][both], np.minimum(rect[3], masked[3])[both])         # bd is the minimum of the two
    assert (rect[3][both] < masked[3][both]).any() and (rect[3][both] > masked[3][both]).any()
    assert 0 < want[4][2:4].sum() < min(rect[4][2:4].sum(), masked[4][2:4].sum())
    glass = np.array([0, 0, 4 * W - 1, 100], np.int32)           # the two top mask rows (32 px) are OUT: an ROI wholly over OUT cells
    assert not mask[:2].any()
    want = against_the_reference(dev, rows, H, W, NC, 0.5, rq, mask, CELL, glass, True, what="roi over OUT cells")
    assert want[1].sum() == 0 and want[4][2:4].sum() == 0 and sr.pair_counts(rows, H, W, NC, 0.5, rq, glass)[4][2:4].sum() > 0


# ---- 6. the limits ------------------------------------------------------------------------------------------------------------------------
def test_the_largest_radius_on_1025_x_1025_cells(dev):
    """16 400 x 16 400 px on 16-px cells, R_{B-1} = 32 767, 32 radii, C = 8.  A position is further than R from the slide's border
    only within 32 767 .. 32 832, so every row of interest stands there.
    First mask, two OUT cells: one row's d2out is R^2 + 1 = 19 661^2 + 26 213^2 (eligible at R: wbd = R) and another's is
    R^2 - 32 = 22 436^2 + 23 881^2 (not eligible: wbd = R - 1).  R^2 itself is no sum of two non-zero squares (32 767 = 7 x 31 x 151,
    all 3 mod 4), so d2out == R^2 exactly is only reached along an axis: the second mask, one OUT cell at the left border in the
    row's own cell row, 32 767 to its left, with neighbours at 32 768 (a capped offset) and at (32 767, 1)."""
    side, cell, R = 16400, 16, 32767
    rq = np.concatenate([np.arange(1, 31) * 1000, [R - 1, R]]).astype(np.int32)
    rng = np.random.default_rng(9)
    filler = np.round(rng.uniform(0, 4 * side, (56, 2)))
    mask = np.ones((1025, 1025), np.uint8)
    mask[138, 161] = mask[922, 820] = 0
    q = np.concatenate([[(32803, 32776), (32819, 32795), (32767, 32820), (32800, 32800)], filler])
    rows = sr.points(q / 4.0, cls=np.arange(len(q)) % 8)
    qx, qy = sr.positions(rows, side, side, 8, 0.0)[:2]
    assert (qx[:4].tolist(), qy[:4].tolist()) == ([32803, 32819, 32767, 32800], [32776, 32795, 32820, 32800])
    d2 = wr.d2_out(qx, qy, mask, cell, side, side)
    assert d2[:3].tolist()[:2] == [R * R - 32, R * R + 1] and d2[2] > R * R and 22436 ** 2 + 23881 ** 2 == R * R - 32 and 19661 ** 2 + 26213 ** 2 == R * R + 1
    for border in (True, False):
        want = against_the_reference(dev, rows, side, side, 8, 0.0, rq, mask, cell, None, border, what=f"limits border={border}")
    want = wr.pair_counts_window(rows, side, side, 8, 0.0, rq, mask, cell)
    assert want[3][:4].tolist() == [R - 1, R, R, R] and want[1][:, -1].sum() == 3 and want[1][:, -2].sum() == 4 and want[0][:, :, -1].sum() > 0
    axis = np.ones((1025, 1025), np.uint8)
    axis[512, 0] = 0                                             # y 32 768 .. 32 831, x 0 .. 63
    q = np.concatenate([[(32830, 32800), (32831, 32800), (32830, 32832), (32832, 32790)], filler])
    rows = sr.points(q / 4.0, cls=np.arange(len(q)) % 8)
    want = against_the_reference(dev, rows, side, side, 8, 0.0, rq, axis, cell, None, True, what="limits, along an axis")
    qx, qy = sr.positions(rows, side, side, 8, 0.0)[:2]
    assert wr.d2_out(qx, qy, axis, cell, side, side)[:4].tolist() == [R * R, 32768 ** 2, R * R + 1, 32768 ** 2]
    assert want[3][:4].tolist() == [R - 1, R, R, R]


# ---- 7. independence and contract ---------------------------------------------------------------------------------------------------------
def test_the_cell_side_does_not_show_and_two_runs_agree(dev):
    rows, rq, mask, want = wr.ragged_case(1025)
    r_max = int(rq[-1])
    for side in (0, r_max, 2 * r_max + 1, 4 * W + 5, 0):
        assert_same(run(dev, rows, H, W, NC, 0.5, rq, mask, CELL, cell_side=side), want, f"cell side {side}")
    none = np.zeros((0, 7), np.float32)
    got = run(dev, none, H, W, NC, 0.5, rq, mask, CELL)
    assert_same(got, wr.pair_counts_window(none, H, W, NC, 0.5, rq, mask, CELL), "M = 0")
    assert got[0].sum() == 0 and got[2].shape == (0, NC, 2)


I32P = C.POINTER(C.c_int32)


class Buffers:
    def __init__(self, dev, M, C_, B):
        self.pairs = torch.empty(C_, C_, B, device=dev, dtype=torch.int64)
        self.centres = torch.empty(C_, B, device=dev, dtype=torch.int32)
        self.nn = torch.empty(M, C_, 2, device=dev, dtype=torch.int32)
        self.bd = torch.empty(M, device=dev, dtype=torch.int32)
        self.stats = torch.empty(2 * C_ + 3, device=dev, dtype=torch.int32)

    def all(self):
        return self.pairs, self.centres, self.nn, self.bd, self.stats

    def numpy(self):
        return tuple(t.cpu().numpy() for t in self.all())


def call(L, rows, M, C_, H_, W_, rq, mask, cell, o, ws, nbytes, border=1, side=0):
    rq = np.ascontiguousarray(rq, np.int32)
    return L.ay_pair_counts_window(ptr(rows), M, C_, H_, W_, C.c_float(0.5), rq.ctypes.data_as(I32P), len(rq), None, border, side,
                                   None if mask is None else ptr(mask), cell, ptr(o.pairs), ptr(o.centres), ptr(o.nn), ptr(o.bd), ptr(o.stats), ptr(ws),
                                   nbytes, _lib.stream_ptr())


def test_refused_arguments_return_minus_one_with_a_message(dev):
    L = _lib.lib()
    rows = torch.zeros(4, 7, device=dev)
    o = Buffers(dev, 4, 2, 3)
    rq = [8, 16, 32]
    mask = torch.ones(7, 7, device=dev, dtype=torch.uint8)
    need = int(L.ay_pair_counts_window_workspace_bytes(4, 100, 100, 32, 0, 16))
    assert need > int(L.ay_pair_counts_workspace_bytes(4, 100, 100, 32, 0)) > 0
    ws = torch.zeros(need + 256, device=dev, dtype=torch.uint8)
    assert call(L, rows, 4, 2, 100, 100, rq, mask, 16, o, ws, need) == 0
    big = 1 << 21                                                # 2^21 / 16 = 2^17 cells a side: 2^34 cells
    for f, word in ((lambda: call(L, rows, 4, 2, 100, 100, rq, mask, 15, o, ws, need), b"mask_cell"),
                    (lambda: call(L, rows, 4, 2, 100, 100, rq, None, 16, o, ws, need), b"null mask"),
                    (lambda: call(L, rows, 4, 2, big, big, rq, mask, 16, o, ws, need), b"2^26"),
                    (lambda: call(L, rows, 4, 2, 100, 100, rq, mask, 16, o, ws, need - 256), b"workspace"),
                    (lambda: call(L, rows, 4, 2, 100, 100, rq, mask, 16, o, ws, need, side=31), b"cell_side")):
        assert f() == -1
        assert word in L.ay_last_error() and b"ay_pair_counts_window" in L.ay_last_error(), (word, L.ay_last_error())
    assert L.ay_pair_counts_window_workspace_bytes(4, 100, 100, 32, 0, 15) == 0 and L.ay_pair_counts_window_workspace_bytes(4, big, big, 32, 0, 16) == 0
    assert L.ay_pair_counts_window_workspace_bytes(4, 131072, 131072, 32, 0, 16) > (1 << 26) // 8    # 8192 x 8192: exactly 2^26 cells are taken, a bit each
    assert L.ay_pair_counts_window_workspace_bytes(4, 131072 + 1, 131072, 32, 0, 16) == 0
    torch.cuda.synchronize()


# ---- 8. capture ---------------------------------------------------------------------------------------------------------------------------
def test_hip_graph_of_the_call_replays_on_new_rows_and_a_new_mask(dev):
    """ay_pair_counts_window captured on a side stream and replayed on other rows and another mask: kernel launches only, and its
    own kernels reset the outputs and rewrite every word of the workspace they read"""
    M = 1025
    L = _lib.lib()
    rq = wr.radii_q(wr.RADII_PX)
    grid = wr.grid_of(H, W, CELL)
    inputs = [(wr.ragged_rows(M, 90 + k), wr.blob_mask(*grid, seed=20 + k, holes=4 + k)) for k in range(3)]
    wants = [wr.pair_counts_window(r, H, W, NC, 0.5, rq, m, CELL) for r, m in inputs]
    assert len({w[1].tobytes() for w in wants}) == 3 and all((w[1] > 0).all() for w in wants)
    rows, mask = torch.from_numpy(inputs[0][0]).to(dev), torch.from_numpy(inputs[0][1]).to(dev)
    o = Buffers(dev, M, NC, len(rq))
    need = int(L.ay_pair_counts_window_workspace_bytes(M, H, W, int(rq[-1]), 0, CELL))
    ws = torch.empty(need, device=dev, dtype=torch.uint8)

    def step():
        assert call(L, rows, M, NC, H, W, rq, mask, CELL, o, ws, need) == 0, L.ay_last_error()

    step()                                                            # eager once (loads the code objects)
    torch.cuda.synchronize()
    assert_same(o.numpy(), wants[0], "eager")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    for k in (1, 2, 0, 1):
        for t in o.all():                                             # the graph's own kernels must reset the outputs
            t.fill_(77)
        ws.fill_(0x5A)
        rows.copy_(torch.from_numpy(inputs[k][0]))
        mask.copy_(torch.from_numpy(inputs[k][1]))
        g.replay()
        torch.cuda.synchronize()
        assert_same(o.numpy(), wants[k], f"replay on input {k}")


# ---- 9. spatial_stats(window=) ------------------------------------------------------------------------------------------------------------
def test_spatial_stats_with_a_window(dev):
    rows, rq, mask, (pairs, centres, nn, bd, stats) = wr.ragged_case(257)
    rows, mask = rows.copy(), mask.copy()                       # (the shared case is read-only)
    cls = sr.positions(rows, H, W, NC, 0.5)[2]
    area = wr.window_area(mask, CELL, H, W)
    assert 0 < area < H * W
    for window in (mask, mask.astype(bool), torch.from_numpy(mask).to(dev), torch.from_numpy(mask.astype(bool)).to(dev), mask * np.uint8(255)):
        got = spatial_stats(rows, (H, W), wr.RADII_PX, NC, 0.5, mpp=0.5, window=window, window_cell=CELL)
        assert_same(tuple(got[k] for k in ("pairs", "centres", "nn", "bd")), (pairs, centres, nn, bd))
        np.testing.assert_array_equal(got["counted"], stats[:2])
        np.testing.assert_array_equal(got["inside"], stats[2:4])
        assert got["window_area"] == area and got["area"] == area
        want = sr.summaries(pairs, centres, stats[2:4], bd, nn, cls, rq, area, 0.5)
        for key in want:
            np.testing.assert_allclose(got[key], want[key], rtol=1e-14, atol=0, err_msg=key)
    assert np.isfinite(got["K"]).all()
    roi = (100.0, 90.5, 800.25, 700.0)                          # a window and an area of the caller's
    got = spatial_stats(torch.from_numpy(rows).to(dev), (H, W), wr.RADII_PX, NC, 0.5, roi=roi, border=False, area=3.0e5, window=mask, window_cell=CELL)
    want = wr.pair_counts_window(rows, H, W, NC, 0.5, rq, mask, CELL, sr.roi_q(roi, H, W), False)
    assert_same(tuple(got[k] for k in ("pairs", "centres", "nn", "bd")), want[:4])
    assert got["area"] == 3.0e5 and got["window_area"] == wr.window_area(mask, CELL, H, W, sr.roi_q(roi, H, W)) < area
    np.testing.assert_array_equal(got["intensity"], want[4][2:4] / 3.0e5)
    plain = spatial_stats(rows, (H, W), wr.RADII_PX, NC, 0.5)
    assert "window_area" not in plain and set(got) == set(plain) | {"window_area"}
    for kw in (dict(window=mask), dict(window_cell=CELL), dict(window=mask, window_cell=15), dict(window=mask[:-1], window_cell=CELL),
               dict(window=mask.astype(np.int32), window_cell=CELL), dict(window=torch.from_numpy(mask).to(dev)[:, :-1], window_cell=CELL),
               dict(window=mask, window_cell=32)):
        with pytest.raises(ValueError, match="window"):
            spatial_stats(rows, (H, W), wr.RADII_PX, NC, 0.5, **kw)


# ---- 10. end to end -----------------------------------------------------------------------------------------------------------------------
def test_quantify_region_with_a_spatial_window(tmp_cfg_dir, dev):
    from test_gpu_burden import OVERLAP, S, TILE, small_model, synthetic_raster
    m = small_model(tmp_cfg_dir, dev)
    raster = synthetic_raster()
    RH, RW = raster.shape[:2]
    cell = 32
    kw = dict(tile=TILE, img_size=S, conf_thres=0.5, nms_thres=0.4, batch_size=4, overlap=OVERLAP, cell=cell, field=3, top_k=4)
    radii = (8, 24.5, 64)
    plain = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, **kw)
    off = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, spatial_window=False, **kw)
    assert set(off) == set(plain) and "spatial_window" not in plain and set(off["spatial"]) == set(plain["spatial"])
    for key, v in plain["spatial"].items():                     # spatial_window=False: the keys and the bytes it had
        np.testing.assert_array_equal(off["spatial"][key], v, err_msg=key)
    # the raster is nearly all tissue: at the default probe stride a cell holds 512, 768 or 1024 estimated tissue pixels of 1024, so
    # three quarters of a cell is the bound at which the mask has both kinds of cell
    got = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, spatial_window=True, spatial_min_tissue=0.75, **kw)
    assert set(got) == set(plain) | {"spatial_window"}
    rows, mask = got["rows"], got["spatial_window"]
    assert torch.equal(rows, plain["rows"]) and len(rows) >= 12
    assert mask.dtype == np.bool_ and mask.shape == got["tissue"].shape and mask.any() and not mask.all()
    np.testing.assert_array_equal(mask, wr.window_from_tissue(got["tissue"], RH, RW, cell, 0.75))
    np.testing.assert_array_equal(mask, window_from_tissue(got["tissue"], (RH, RW), cell, 0.75))
    want = spatial_stats(rows, (RH, RW), radii, 3, 0.0, mpp=0.5, window=mask, window_cell=cell)
    assert set(got["spatial"]) == set(want) == set(plain["spatial"]) | {"window_area"}
    for key, v in want.items():
        np.testing.assert_array_equal(got["spatial"][key], v, err_msg=key)
    ref = wr.pair_counts_window(rows.numpy(), RH, RW, 3, 0.0, sr.radii_q(radii), mask, cell)
    assert_same(tuple(got["spatial"][k] for k in ("pairs", "centres", "nn", "bd")), ref[:4], "end to end")
    np.testing.assert_array_equal(got["spatial"]["inside"], ref[4][3:6])
    assert got["spatial"]["area"] == got["spatial"]["window_area"] == wr.window_area(mask, cell, RH, RW) < RH * RW
    assert (got["spatial"]["centres"] <= plain["spatial"]["centres"]).all()
    assert (got["spatial"]["centres"].sum(1) < plain["spatial"]["centres"].sum(1)).any()       # a class lost eligible centres to the mask
    for bad in (dict(spatial_window=True), dict(spatial_radii=radii, spatial_window=True, spatial_min_tissue=1.5)):
        with pytest.raises(ValueError, match="spatial"):
            quantify_region(m, raster, **{**kw, **bad})
    with pytest.raises(ValueError, match="window_cell"):
        quantify_region(m, raster, spatial_radii=radii, spatial_window=True, **{**kw, "cell": 8, "probe_stride": 8})
