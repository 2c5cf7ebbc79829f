"""Spatial statistics (-m gpu): ay_pair_counts through wsi.pair_counts_device, wsi.spatial_stats and quantify_region(spatial_radii=...).
Every output -- pairs, centres, nn, bd, stats -- is compared byte for byte: THE PAIR RULE is two fp32 operations that both sides
compute alike and integers after them.

Yardstick: tests/spatial_reference.py (the rule by brute force over all pairs in NumPy, and as a Python loop over every pair)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spatial_reference as sr
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ptr
from amyloid_yolo_paper_amd.wsi import detect_region, pair_counts_device, quantify_region, spatial_stats

pytestmark = pytest.mark.gpu

H, W, NC = sr.SLIDE_H, sr.SLIDE_W, sr.CLASSES
NAMES = ("pairs", "centres", "nn", "bd", "stats")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def run(dev, rows, H_, W_, C_, min_conf, rq, roi=None, border=True, cell_side=0):
    t = torch.from_numpy(np.array(rows, np.float32)).reshape(-1, 7).to(dev)      # (a copy: the shared cases are read-only)
    out = pair_counts_device(t, (H_, W_), rq, C_, min_conf, roi, border, cell_side)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in NAMES)


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
        assert g.tobytes() == w.tobytes(), (what, name)


def against_the_reference(dev, rows, H_, W_, C_, min_conf, rq, roi=None, border=True, cell_side=0, what=""):
    want = sr.pair_counts(rows, H_, W_, C_, min_conf, rq, roi, border)
    assert_same(run(dev, rows, H_, W_, C_, min_conf, rq, roi, border, cell_side), want, what)
    return want


# ---- 1. sizes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", sr.SIZES)
def test_clustered_case_against_the_restatement(dev, M):
    rows, rq, want = sr.clustered_case(M)                      # (check_not_idle ran on the restatement for M >= 257)
    assert_same(run(dev, rows, H, W, NC, 0.5, rq), want, f"M={M}")
    if M <= 257:
        rows, rq, want = sr.clustered_case(M, border=False)
        assert_same(run(dev, rows, H, W, NC, 0.5, rq, None, False), want, f"M={M} without border")


def test_spatial_stats_returns_the_raw_outputs_and_the_host_formulas(dev):
    rows, rq, (pairs, centres, nn, bd, stats) = sr.clustered_case(257)
    rows = rows.copy()                                          # (the shared case is read-only)
    cls = sr.positions(rows, H, W, NC, 0.5)[2]
    for src in (rows, torch.from_numpy(rows).to(dev)):
        got = spatial_stats(src, (H, W), sr.RADII_PX, NC, 0.5, mpp=0.5)
        assert_same(tuple(got[k] for k in ("pairs", "centres", "nn", "bd")), (pairs, centres, nn, bd))
        np.testing.assert_array_equal(got["counted"], stats[:3])
        np.testing.assert_array_equal(got["inside"], stats[3:6])
        assert (got["below"], got["flagged"], got["flags"]) == tuple(int(v) for v in stats[6:])
        assert got["radii"].tolist() == [float(r) for r in sr.RADII_PX] and got["area"] == float(H * W)
        np.testing.assert_array_equal(got["nn_index"], nn[:, :, 1])
        d2 = nn[:, :, 0].astype(np.float64)
        np.testing.assert_array_equal(got["nn_distance"], np.where(d2 >= 0, np.sqrt(np.abs(d2)) / 4.0, np.nan))
        want = sr.summaries(pairs, centres, stats[3:6], bd, nn, cls, rq, float(H * W), 0.5)
        for key in want:
            np.testing.assert_allclose(got[key], want[key], rtol=1e-14, atol=0, err_msg=key)
    # a window and an area of the caller's
    roi = (300.0, 200.5, 3800.25, 2900.0)
    got = spatial_stats(rows, (H, W), sr.RADII_PX, NC, 0.5, roi=roi, border=False, area=5.0e6)
    want = sr.pair_counts(rows, H, W, NC, 0.5, rq, sr.roi_q(roi, H, W), False)
    assert_same(tuple(got[k] for k in ("pairs", "centres", "nn", "bd")), want[:4])
    assert got["roi_q"].tolist() == [1200, 802, 15201, 11600] and got["area"] == 5.0e6
    np.testing.assert_array_equal(got["intensity"], want[4][3:6] / 5.0e6)


# ---- 2. equality, duplicates ----------------------------------------------------------------------------------------------------------
def test_pairs_at_exactly_the_radius_count(dev):
    """a 16 x 16 integer lattice 1 px apart, radii 5 and 13 px: 3-4-5 and 5-12-13 pairs lie at exactly R_k"""
    rows = sr.lattice_rows(16, 1.0, C=2, side=6.0, x0=20.0, y0=24.0)
    qx, qy, _, _, _, _ = sr.positions(rows, 64, 64, 2, 0.0)
    d2 = (qx[:, None] - qx[None, :]) ** 2 + (qy[:, None] - qy[None, :]) ** 2
    assert (d2 == 20 * 20).sum() >= 100 and (d2 == 52 * 52).sum() >= 100                       # the case says something
    at = against_the_reference(dev, rows, 64, 64, 2, 0.0, sr.radii_q((5, 13)), None, False, what="at the radius")
    short = against_the_reference(dev, rows, 64, 64, 2, 0.0, sr.radii_q((4.75, 13)), None, False, what="a quarter pixel shorter")
    assert at[0][:, :, 0].sum() - short[0][:, :, 0].sum() == ((d2 > 19 * 19) & (d2 <= 20 * 20)).sum()
    against_the_reference(dev, rows, 64, 64, 2, 0.0, sr.radii_q((5, 13)), None, True, what="at the radius, border")


def test_duplicates_at_one_position(dev):
    rows = sr.points([[100.25, 50.5]] * 100, cls=np.arange(100) % 3)
    want = against_the_reference(dev, rows, 200, 300, 3, 0.0, sr.radii_q((0.25, 2)), what="duplicates")
    pairs, _, nn, _, _ = want
    assert pairs[0, 0, 0] == 34 * 33 and pairs[0, 1, 0] == 34 * 33 and pairs[1, 2, 1] == 33 * 33
    assert (nn[:, :, 0] == 0).all()
    assert nn[0].tolist() == [[0, 3], [0, 1], [0, 2]] and nn[1].tolist() == [[0, 0], [0, 4], [0, 2]]    # the lowest index, never itself


# ---- 3. cell geometry -----------------------------------------------------------------------------------------------------------------
def test_cell_edges_slide_borders_and_centres_outside(dev):
    Hs, Ws = 300, 500                                                   # 1200 x 2000 quarter pixels: no multiple of the 32-wide cell
    rq = sr.radii_q((1, 3.5, 8))
    assert rq[-1] == 32
    xs = [(32 * k + d) / 4.0 for k in (1, 2, 3, 20, 62) for d in (-1, 0, 1)]
    ys = [(32 * k + d) / 4.0 for k in (1, 2, 17, 37) for d in (-1, 0, 1)]
    pts = [(x, y) for x in xs for y in ys]
    pts += [(0, y) for y in ys] + [(Ws - 0.25, y) for y in ys] + [(x, 0) for x in xs] + [(x, Hs - 0.25) for x in xs]       # the four borders
    pts += [(-10, 8), (-10, 9), (Ws + 10, 8.25), (Ws + 3, 9), (8, -7), (8.5, -70), (9, Hs + 5), (12, Hs + 50), (-5, -5), (Ws + 5, Hs + 5)]
    rows = sr.points(pts, cls=np.arange(len(pts)) % 2)
    for border in (True, False):
        want = against_the_reference(dev, rows, Hs, Ws, 2, 0.0, rq, None, border, what=f"cell edges border={border}")
    assert want[0].min() > 0
    for side in (32, 33, 100, 5000):
        against_the_reference(dev, rows, Hs, Ws, 2, 0.0, rq, None, True, side, what=f"cell side {side}")


def test_tiny_slides(dev):
    rows = sr.points([(1, 1), (3.25, 2), (4.75, 6.5), (0, 0), (9, 9), (2, 2)], cls=[0, 1, 0, 1, 0, 1])
    against_the_reference(dev, rows, 7, 5, 2, 0.0, sr.radii_q((2, 8)), what="a slide smaller than r_max")
    rows = sr.points([(0, 0), (0.25, 0.5), (0.75, 0.75), (0.5, 0), (5, 5), (0.75, 0.75)], cls=[0, 0, 1, 1, 0, 1])
    want = against_the_reference(dev, rows, 1, 1, 2, 0.0, sr.radii_q((0.25, 0.5, 1)), None, False, what="H = W = 1")
    assert (want[0][:, :, -1] > 0).all() and want[4][:2].sum() == 6            # the centre at (5, 5) stands at the corner position
    against_the_reference(dev, rows, 1, 1, 2, 0.0, sr.radii_q((0.25, 0.5, 1)), None, True, what="H = W = 1, border")


def test_a_dense_cell(dev):
    """all 3000 rows inside one 256-px cell: every wavefront walks the same long run, every atomic of the scatter hits one word"""
    rng = np.random.default_rng(5)
    xy = np.round(rng.uniform([1024 + 1, 1280 + 1], [1280 - 1, 1536 - 1], (3000, 2)) * 8) / 8
    rows = sr.points(xy, cls=rng.integers(0, 3, 3000))
    rq = sr.radii_q(sr.RADII_PX)
    want = against_the_reference(dev, rows, H, W, NC, 0.0, rq, what="a dense cell")
    assert want[0].min() > 0 and want[1][:, -1].min() > 900


# ---- 4. the window --------------------------------------------------------------------------------------------------------------------
def test_roi_and_border(dev):
    rq = sr.radii_q((2, 5, 10))                                          # 8, 20, 40 quarter pixels
    roi = np.array([400, 200, 1200, 900], np.int32)
    pts = [(200.0, 140.0)]
    for R in (8, 20, 40):
        for off in (R, R - 1, R + 1, 0, -1):                             # bd == R_k, R_k - 1, ..., on the border, one position outside
            pts += [((400 + off) / 4, 140.0), ((1200 - off) / 4, 141.0), (200.0, (200 + off) / 4), (201.0, (900 - off) / 4)]
    rng = np.random.default_rng(11)
    pts += [tuple(p) for p in np.round(rng.uniform([80, 30], [320, 250], (300, 2)) * 4) / 4]
    rows = sr.points(pts, cls=np.arange(len(pts)) % 2)
    for border in (True, False):
        want = against_the_reference(dev, rows, 400, 600, 2, 0.0, rq, roi, border, what=f"roi border={border}")
        pairs, centres, nn, bd, stats = want
        assert set((8, 7, 9, 20, 19, 21, 40, 39, 41, 0, -1)) <= set(bd.tolist())
        assert (stats[2:4] < stats[0:2]).all()                          # rows outside the window are counted, but not inside
        assert ((nn[:, :, 1] >= 0).any(1) & (bd < 0)).any()             # a row outside the window still has its nearest neighbours
    whole = np.array([0, 0, 4 * 600 - 1, 4 * 400 - 1], np.int32)
    assert_same(run(dev, rows, 400, 600, 2, 0.0, rq, None), run(dev, rows, 400, 600, 2, 0.0, rq, whole), "roi=None against the whole slide")
    one = np.array([800, 560, 800, 560], np.int32)                       # one position: (200, 140) px
    want = against_the_reference(dev, rows, 400, 600, 2, 0.0, rq, one, False, what="a window of one position")
    assert want[4][2:4].sum() >= 1 and want[1].sum() >= 1
    against_the_reference(dev, rows, 400, 600, 2, 0.0, rq, one, True, what="a window of one position, border")


@pytest.mark.parametrize("M", [257, 4097])
def test_the_cell_side_does_not_show(dev, M):
    rows, rq, want = sr.clustered_case(M)
    r_max = int(rq[-1])
    for side in (r_max, 2 * r_max, 7 * r_max + 3, 4 * W + 5):
        assert_same(run(dev, rows, H, W, NC, 0.5, rq, None, True, side), want, f"cell side {side}")


def test_many_cells(dev):
    """small radii on the large slide: grids of 3 072 (the call's own), 196 608 (96 whole chunks of the three-level scan) and 185 381
    cells (a last chunk that is not full)"""
    rows = sr.clustered_case(4097)[0]
    rq = sr.radii_q((2, 4, 8))
    want = sr.pair_counts(rows, H, W, NC, 0.5, rq)
    assert (want[0][:, :, -1] > 0).all() and want[1].min() > 0
    for side in (0, 32, 33):
        assert_same(run(dev, rows, H, W, NC, 0.5, rq, None, True, side), want, f"many cells, cell side {side}")


def test_row_order(dev):
    rows, rq, want = sr.clustered_case(257)
    perm = np.random.default_rng(3).permutation(257)
    shuffled = rows[perm]
    got = run(dev, shuffled, H, W, NC, 0.5, rq)
    for k in (0, 1, 4):                                                  # pairs, centres, stats: unchanged
        assert got[k].tobytes() == want[k].tobytes()
    np.testing.assert_array_equal(got[3], want[3][perm])                 # bd and the nn distances: permuted
    np.testing.assert_array_equal(got[2][:, :, 0], want[2][perm][:, :, 0])
    again = sr.pair_counts(shuffled, H, W, NC, 0.5, rq)
    sr.check_not_idle(257, again)
    assert_same(got, again, "shuffled")                                 # the indices: against the restatement


# ---- 5. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits(dev):
    rq = sr.radii_q(sr.RADII_PX)
    got = run(dev, np.zeros((0, 7), np.float32), H, W, NC, 0.5, rq)
    assert_same(got, sr.pair_counts(np.zeros((0, 7), np.float32), H, W, NC, 0.5, rq), "M = 0")
    assert got[0].sum() == 0 and got[2].shape == (0, 3, 2)
    rows = sr.clustered_case(257)[0]
    want = against_the_reference(dev, rows, H, W, 5, 0.5, rq, what="a class without rows")      # (the generator's bad label 3 is a class here)
    assert want[4][4] == 0 and want[0][4].sum() == 0 and want[0][:, 4].sum() == 0 and (want[2][:, 4] == -1).all()
    against_the_reference(dev, rows, H, W, 1, 0.5, sr.radii_q((64,)), what="C = 1, B = 1")
    many = sr.clustered_rows(1200, 17, C=8)
    want = against_the_reference(dev, many, H, W, 8, 0.5, sr.radii_q(40 + 8 * np.arange(32)), what="C = 8, B = 32")
    sr.check_not_idle(1200, want)
    assert want[0].shape == (8, 8, 32) and (np.diff(want[1], axis=1) < 0).any()


def test_the_largest_radius_on_the_largest_slide(dev):
    side = 1 << 21
    base = 1000000.0
    pts = [(base, base), (base + 8191.75, base), (base + 8192.0, base + 1), (base, base + 8191.75), (base + 5000, base + 6000.25),
           (side - 0.25, side - 0.25), (side - 8192.0, side - 0.25), (side + 100.0, side - 8191.75), (0, 0), (8191.75, 0)]
    rows = sr.points(pts, cls=[0, 1, 0, 1, 0, 1, 0, 1, 0, 1])
    qx = sr.positions(rows, side, side, 2, 0.0)[0]
    assert (np.abs(qx[:, None] - qx[None, :]) == 32767).any() and qx.max() == 4 * side - 1
    rq = np.array([1, 30000, 32767], np.int32)
    for border in (True, False):
        want = against_the_reference(dev, rows, side, side, 2, 0.0, rq, None, border, what=f"R = 32767 border={border}")
    assert (want[2][:, :, 0] == 32767 * 32767).any()                     # a nearest neighbour at exactly the largest radius


# ---- 6. launch behaviour --------------------------------------------------------------------------------------------------------------
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


def call(L, rows, M, C_, H_, W_, rq, roi, border, side, o, ws, nbytes):
    rq = np.ascontiguousarray(rq, np.int32)
    roi_arg = None if roi is None else np.ascontiguousarray(roi, np.int32).ctypes.data_as(I32P)
    return L.ay_pair_counts(ptr(rows), M, C_, H_, W_, C.c_float(0.5), rq.ctypes.data_as(I32P), len(rq), roi_arg, border, side, ptr(o.pairs),
                            ptr(o.centres), ptr(o.nn), ptr(o.bd), ptr(o.stats), ptr(ws), nbytes, _lib.stream_ptr())


def test_bad_arguments_return_minus_one_with_a_message(dev):
    L = _lib.lib()
    rows = torch.zeros(4, 7, device=dev)
    o = Buffers(dev, 4, 8, 32)
    rq = [8, 16, 32]
    need = int(L.ay_pair_counts_workspace_bytes(4, 100, 100, 32, 0))
    assert need > 0
    ws = torch.zeros(need + 256, device=dev, dtype=torch.uint8)

    def go(M=4, C_=2, H_=100, W_=100, r=rq, roi=None, side=0, nbytes=need, w=ws):
        return call(L, rows, M, C_, H_, W_, r, roi, 1, side, o, w, nbytes)

    assert go() == 0
    for f, word in ((lambda: go(M=-1), b"n_rows"), (lambda: go(C_=0), b"num_classes"), (lambda: go(C_=9), b"num_classes"),
                    (lambda: go(H_=0), b"slide"), (lambda: go(W_=(1 << 21) + 1), b"slide"), (lambda: go(r=[]), b"n_radii"),
                    (lambda: go(r=list(range(1, 34))), b"n_radii"), (lambda: go(r=[8, 8]), b"radii"), (lambda: go(r=[16, 8]), b"radii"),
                    (lambda: go(r=[0, 8]), b"radii"), (lambda: go(r=[8, 32768]), b"radii"), (lambda: go(roi=[50, 0, 49, 10]), b"roi"),
                    (lambda: go(roi=[0, 11, 49, 10]), b"roi"), (lambda: go(side=31), b"cell_side"), (lambda: go(nbytes=need - 256), b"workspace"),
                    (lambda: go(w=ws[4:]), b"aligned")):
        assert f() == -1
        assert word in L.ay_last_error(), (word, L.ay_last_error())
    assert L.ay_pair_counts_workspace_bytes(4, 100, 100, 32, 31) == 0 and L.ay_pair_counts_workspace_bytes(4, 0, 100, 32, 0) == 0
    torch.cuda.synchronize()


def test_two_runs_give_the_same_bytes(dev):
    rows, rq, want = sr.clustered_case(4097)
    a, b = run(dev, rows, H, W, NC, 0.5, rq), run(dev, rows, H, W, NC, 0.5, rq)
    assert_same(a, b, "two runs")
    assert_same(a, want, "two runs against the restatement")


def test_hip_graph_of_the_call_replays_on_new_rows(dev):
    """ay_pair_counts captured on a side stream and replayed on other rows: kernel launches only, and its own kernels reset the outputs"""
    M = 1025
    L = _lib.lib()
    rq = sr.radii_q(sr.RADII_PX)
    inputs = [sr.clustered_rows(M, 70 + k) for k in range(3)]
    wants = [sr.pair_counts(r, H, W, NC, 0.5, rq) for r in inputs]
    for w in wants:
        sr.check_not_idle(M, w)
    rows = torch.from_numpy(inputs[0]).to(dev)
    o = Buffers(dev, M, NC, len(rq))
    need = int(L.ay_pair_counts_workspace_bytes(M, H, W, int(rq[-1]), 0))
    ws = torch.empty(need, device=dev, dtype=torch.uint8)

    def step():
        assert call(L, rows, M, NC, H, W, rq, None, 1, 0, o, ws, need) == 0, L.ay_last_error()

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
        rows.copy_(torch.from_numpy(inputs[k]))
        g.replay()
        torch.cuda.synchronize()
        assert_same(o.numpy(), wants[k], f"replay on input {k}")


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------
def test_quantify_region_with_spatial_radii(tmp_cfg_dir, dev):
    from test_gpu_burden import OVERLAP, S, TILE, small_model, synthetic_raster
    m = small_model(tmp_cfg_dir, dev)
    raster = synthetic_raster()
    RH, RW = raster.shape[:2]
    kw = dict(tile=TILE, img_size=S, conf_thres=0.5, nms_thres=0.4, batch_size=4, overlap=OVERLAP, cell=32, field=3, top_k=4)
    radii = (8, 24.5, 64)
    plain = quantify_region(m, raster, mpp=0.5, **kw)
    got = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, **kw)
    assert "spatial" not in plain and set(got) == set(plain) | {"spatial"}            # without the argument: the keys it had
    rows = got["rows"]
    assert torch.equal(rows, plain["rows"]) and len(rows) >= 12
    want = spatial_stats(rows, (RH, RW), radii, 3, 0.0, area=int(got["tissue"].sum()), mpp=0.5)
    assert set(got["spatial"]) == set(want)
    for key, v in want.items():
        np.testing.assert_array_equal(got["spatial"][key], v, err_msg=key)
    ref = sr.pair_counts(rows.numpy(), RH, RW, 3, 0.0, sr.radii_q(radii))
    assert_same(tuple(got["spatial"][k] for k in ("pairs", "centres", "nn", "bd")), ref[:4], "end to end")
    assert ref[0].sum() > 0 and got["spatial"]["area"] == float(got["tissue"].sum()) and np.isfinite(got["spatial"]["K"]).any()
