"""Amyloid load (-m gpu): ay_stain_load_u8, wsi.stain_load, wsi.quantify_region(load=True).  Every comparison is exact: integers, or
bytes.  Yardstick: tests/load_reference.py (THE LOAD RULE restated in NumPy on stain_reference's and tissue_reference's pixel classes);
the histogram's tail (wsi.stain_stats) and the tissue map (wsi.tissue_counts) for the totals."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import load_reference as lr
import stain_reference as sref
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import StainMap, quantify_region, stain_load, stain_stats, tissue_counts
from test_gpu_seam import BATCH, CONF, NMS, S, TILE, build_model, region_raster
from test_gpu_stain import hist_rasters, placed
from test_gpu_tissue import dark_and_bright

pytestmark = pytest.mark.gpu

GUARD = 16
CELLS = (lr.MIN_CELL, 24, 37, 128, 400)            # 400: larger than either region, and than the slide around it
THRES = (0, 10, 40, 512)
PLACEMENTS = ((0, 0), (0, 7), (5, 0), (5, 7))      # (base, pad): test_gpu_stain's, both load paths
ORIGIN, MARGIN = (13, 29), (21, 40)                # the region inside a larger slide: cell borders fall mid-band and mid-item
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def guarded(dev, n):
    """n zeroed int64 words with GUARD words of -7 behind them"""
    t = torch.full((n + GUARD,), -7, device=dev, dtype=torch.int64)
    t[:n] = 0
    return t


def device_load(dev, params, r, shrink, bg, stain, j, cell, origin, slide, base, pad, cells, rows=None, boxes=None, flags=None):
    buf, stride = placed(dev, r, base, pad)
    M = 0 if rows is None else int(rows.shape[0])
    return _lib.lib().ay_stain_load_u8(ptr(buf), r.shape[0], r.shape[1], stride, shrink, origin[0], origin[1], slide[0], slide[1], bg,
                                       ptr(params), stain, j, cell, ptr(cells), ptr(rows), M, ptr(boxes), ptr(flags), _lib.stream_ptr())


# ---- 1. the cell pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(97, 131), (200, 304)], ids=str)
def test_cell_pass_against_the_reference(dev, shape):
    """Crossed in full: raster x shrink x bg_level x placement x origin x thres_bin, 576 combinations per shape: every kernel instance
    and load path on every kind of data, at both origins, with every threshold.  The two launch parameters left, (stain, cell), ten
    pairs, rotate through those combinations three at a time (3 and 10 share no factor, and the 96 draws of one raster, shrink and
    level shift the next by 6).  What the rotation reaches is asserted at the end, not assumed: every pair with every threshold at
    each origin, at each pad and on each load path, and a case with 0 < positive < tissue for both thresholds that can make one on
    every (load path, shrink, origin).  Per run: two runs with the same bytes, guard words, and a second call on another raster
    that adds."""
    params, t = StainMap.identity().params, sref.tables()
    all_pairs = set(itertools.product((0, 1), CELLS))
    pairs = itertools.cycle(sorted(all_pairs))
    assert (3 * 304) % 16 == 0 and (3 * 131 + 7) % 16 == 0        # base 0 with these strides takes the 16-byte loads (test_gpu_stain)
    by_origin, by_pad, by_path, some_positive = {}, {}, {}, set()
    for name, r in hist_rasters(*shape).items():
        other = np.ascontiguousarray(r[::-1, ::-1] // 2 + 40)                       # the "next strip": other pixels, other bins
        for shrink, bg in itertools.product((1, 2), (0, 170, 256)):
            H, W = shape[0] // shrink, shape[1] // shrink
            cls = {(k, s): lr.classes(x, shrink, bg, t, s) for k, x in (("r", r), ("other", other)) for s in (0, 1)}
            for (base, pad), inside, j in itertools.product(PLACEMENTS, (False, True), THRES):
                origin = ORIGIN if inside else (0, 0)
                slide = (H + ORIGIN[0] + MARGIN[0], W + ORIGIN[1] + MARGIN[1]) if inside else (H, W)
                wide = base == 0 and (3 * shape[1] + pad) % 16 == 0
                for _ in range(3):
                    stain, cell = next(pairs)
                    by_origin.setdefault((j, inside), set()).add((stain, cell))
                    by_pad.setdefault((j, pad), set()).add((stain, cell))
                    by_path.setdefault((j, wide), set()).add((stain, cell))
                    want, _, _ = lr.new_outputs(slide[0], slide[1], cell, 0)
                    lr.add_classes(*cls[("r", stain)], origin[0], origin[1], slide[0], slide[1], j, cell, want, None, None, None)
                    want2 = want.copy()
                    lr.add_classes(*cls[("other", stain)], origin[0], origin[1], slide[0], slide[1], j, cell, want2, None, None, None)
                    what = (name, shrink, bg, base, pad, origin, j, stain, cell)
                    if bg == 256:
                        assert want[:, :, 0].sum() == H * W, what
                    if bg == 0 or j == 512:
                        assert want[:, :, 1:].sum() == 0, what
                    if 0 < want[:, :, 1].sum() < want[:, :, 0].sum():
                        some_positive.add((j, wide, shrink, inside))
                    n = want.size
                    runs = []
                    for _ in range(2):
                        cells = guarded(dev, n)
                        assert device_load(dev, params, r, shrink, bg, stain, j, cell, origin, slide, base, pad, cells) == 0
                        runs.append(cells.cpu().numpy())
                    assert runs[0].tobytes() == runs[1].tobytes(), what                # two runs, the same bytes
                    assert (runs[0][n:] == -7).all(), what                             # guard words behind the cells untouched
                    assert np.array_equal(runs[0][:n].reshape(want.shape), want), what
                    assert device_load(dev, params, other, shrink, bg, stain, j, cell, origin, slide, base, pad, cells) == 0
                    got = cells.cpu().numpy()                                          # a second call adds
                    assert np.array_equal(got[:n].reshape(want.shape), want2) and (got[n:] == -7).all(), what
    # what the rotation reached
    assert set(by_origin) == set(itertools.product(THRES, (False, True))) and all(v == all_pairs for v in by_origin.values())
    assert set(by_pad) == set(itertools.product(THRES, (0, 7))) and all(v == all_pairs for v in by_pad.values())
    assert set(by_path) == set(itertools.product(THRES, (False, True))) and all(v == all_pairs for v in by_path.values())
    assert some_positive == set(itertools.product((10, 40), (False, True), (1, 2), (False, True)))


@pytest.mark.parametrize("shrink", [1, 2])
def test_cell_pass_on_rows_longer_than_a_work_unit(dev, shrink):
    """a work unit holds 256 48-byte items of 16 rows, 4096 pixels (2048 halved): rows of 33 001 pixels are walked in nine units, 19
    rows in two bands"""
    params, t = StainMap.identity().params, sref.tables()
    r = dark_and_bright(21, 19, 33001)
    H, W = 19 // shrink, 33001 // shrink
    assert W > 4 * 4096
    cls = lr.classes(r, shrink, 170, t, 1)
    for origin, slide in (((0, 0), (H, W)), ((7, 29), (H + 30, W + 100))):
        want, _, _ = lr.new_outputs(slide[0], slide[1], 64, 0)
        lr.add_classes(*cls, origin[0], origin[1], slide[0], slide[1], 10, 64, want, None, None, None)
        assert 0 < want[:, :, 1].sum() < want[:, :, 0].sum() < H * W
        for base, pad in ((0, 5), (5, 7)):                        # 99 003 + 5 is a multiple of 16: the 16-byte loads
            cells = guarded(dev, want.size)
            assert device_load(dev, params, r, shrink, 170, 1, 10, 64, origin, slide, base, pad, cells) == 0
            got = cells.cpu().numpy()
            assert np.array_equal(got[:want.size].reshape(want.shape), want) and (got[want.size:] == -7).all(), (origin, base, pad)


# ---- 2. the box pass ------------------------------------------------------------------------------------------------------------------
def hand_rows(H, W):
    row = lambda x1, y1, x2, y2: [x1, y1, x2, y2, 0.9, 0.9, 0.0]
    return np.asarray([row(10.5, 10.5, 11.5, 11.5), row(10.5, 10.5, 10.5, 30.0), row(0.0, 0.0, W, H), row(-7.3, -1e9, 4.5, 2.49),
                       row(W - 2.5, H - 1.5, 1e9, 3e38), row(30.0, 40.0, 20.0, 50.0), row(20.0, 50.0, 30.0, 40.0), row(NAN, 1.0, 5.0, 5.0),
                       row(1.0, 1.0, INF, 5.0), row(1.0, -INF, 5.0, 5.0), row(3.2, 12.6, 40.0, 14.4), row(W + 5.0, 3.0, W + 9.0, 8.0)], np.float32)


@pytest.mark.parametrize("shrink", [1, 2])
def test_box_pass_on_one_region_and_on_three_uneven_strips(dev, shrink):
    params, t = StainMap.identity().params, sref.tables()
    rasters = hist_rasters(97, 131)
    r = rasters["random"]
    H, W = 97 // shrink, 131 // shrink
    rows = np.concatenate([hand_rows(H, W), lr.random_boxes(200, H, W, 17 + shrink, cuts=(13, 14))])
    M = len(rows)
    d_rows = torch.from_numpy(rows).to(dev)
    for stain, j, cell in ((1, 10, 24), (0, 40, 16)):
        want_c, want_b, want_f = lr.load(r, shrink, 170, t, stain, j, cell, rows)
        assert want_f[0] == lr.FLAG_NONFINITE and 0 < want_b[:, 2].sum() < want_b[:, 1].sum() < want_b[:, 0].sum()
        assert (want_b[:, 0] > 0).sum() > 150 and np.array_equal(want_b[:, 0], lr.owned_pixels(rows, H, W))     # the closed form
        for cuts in ((), (13, 14)):                                # one region; rows 0..13, 13..14, 14..H of the (halved) slide
            bounds = [0, *cuts, H]
            for with_cells in (True, False):
                cells, boxes = guarded(dev, want_c.size), guarded(dev, M * 4)
                flags = torch.tensor([0, -7], device=dev, dtype=torch.int32)
                for a, b in zip(bounds[:-1], bounds[1:]):
                    assert device_load(dev, params, r[a * shrink:b * shrink], shrink, 170, stain, j, cell, (a, 0), (H, W), 0, 0,
                                       cells if with_cells else None, d_rows, boxes, flags) == 0
                got_b, got_c = boxes.cpu().numpy(), cells.cpu().numpy()
                assert np.array_equal(got_b[:M * 4].reshape(M, 4), want_b) and (got_b[M * 4:] == -7).all(), (stain, cuts, with_cells)
                assert flags.tolist() == [lr.FLAG_NONFINITE, -7]
                assert np.array_equal(got_c[:want_c.size].reshape(want_c.shape), want_c if with_cells else 0 * want_c)
                assert (got_c[want_c.size:] == -7).all()
    # n_rows == 0 with NULL rows, boxes and flags: legal, and only the cells are written
    cells = guarded(dev, want_c.size)
    assert _lib.lib().ay_stain_load_u8(ptr(torch.from_numpy(r).to(dev)), 97, 131, 131 * 3, shrink, 0, 0, H, W, 170, ptr(params), 0, 40, 16,
                                       ptr(cells), None, 0, None, None, _lib.stream_ptr()) == 0
    assert np.array_equal(cells.cpu().numpy()[:want_c.size].reshape(want_c.shape), want_c)
    # one colour, one box over all of it: every lane adds into one box, every pixel into one bin
    one = rasters["one colour"]
    whole = np.asarray([[0, 0, W, H, 1, 1, 0], [-5, -5, W + 5, H + 5, 1, 1, 1]], np.float32)
    _, want_b, _ = lr.load(one, shrink, 170, t, 1, 10, 128, whole)
    assert (want_b[:, 0] == W * H).all() and (want_b[:, 2] == W * H).all() and want_b[0, 3] % (W * H) == 0
    boxes, flags = guarded(dev, 8), torch.zeros(1, device=dev, dtype=torch.int32)
    assert device_load(dev, params, one, shrink, 170, 1, 10, 128, (0, 0), (H, W), 5, 7, None, torch.from_numpy(whole).to(dev), boxes, flags) == 0
    got = boxes.cpu().numpy()
    assert np.array_equal(got[:8].reshape(2, 4), want_b) and (got[8:] == -7).all() and int(flags.item()) == 0


# ---- 3. a captured HIP graph ----------------------------------------------------------------------------------------------------------
def test_hip_graph_of_one_call_replays_on_other_rows(dev):
    """one call with cells and boxes captured on one stream (no side branches) and replayed onto re-zeroed outputs: launches only"""
    params, t = StainMap.identity().params, sref.tables()
    r = dark_and_bright(31, 97, 131)
    H, W, M, cell = 97, 131, 120, 24
    inputs = [lr.random_boxes(M, H, W, 70 + k) for k in range(3)]
    rd = torch.from_numpy(r).to(dev)
    rows = torch.from_numpy(inputs[0]).to(dev)
    gy, gx = lr.grid(H, W, cell)
    cells = torch.zeros(gy, gx, 3, device=dev, dtype=torch.int64)
    boxes = torch.zeros(M, 4, device=dev, dtype=torch.int64)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def step():
        check(_lib.lib().ay_stain_load_u8(ptr(rd), H, W, W * 3, 1, 0, 0, H, W, 170, ptr(params), 1, 10, cell, ptr(cells), ptr(rows), M,
                                          ptr(boxes), ptr(flags), _lib.stream_ptr()), "ay_stain_load_u8")

    step()                                                            # eager once (loads the code objects)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    for k in (1, 2, 0, 1):
        for out in (cells, boxes, flags):                             # the call adds: the caller zeroes
            out.zero_()
        rows.copy_(torch.from_numpy(inputs[k]))
        g.replay()
        torch.cuda.synchronize()
        want_c, want_b, want_f = lr.load(r, 1, 170, t, 1, 10, cell, inputs[k])
        assert 0 < want_b[:, 2].sum() < want_b[:, 1].sum()
        np.testing.assert_array_equal(cells.cpu().numpy(), want_c)
        np.testing.assert_array_equal(boxes.cpu().numpy(), want_b)
        assert int(flags.item()) == int(want_f[0]) == 0


# ---- 4. bad arguments through the C ABI -----------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one_and_leave_the_outputs_alone(dev):
    L, params, sp = _lib.lib(), StainMap.identity().params, _lib.stream_ptr()
    rd = torch.full((32, 32, 3), 90, dtype=torch.uint8, device=dev)
    rows = torch.tensor([[0, 0, 32, 32, 1, 1, 0]], dtype=torch.float32, device=dev)
    cells = torch.full((2 * 2 * 3 + 1,), 77, dtype=torch.int64, device=dev)
    boxes = torch.full((4 + 1,), 77, dtype=torch.int64, device=dev)
    flags = torch.full((1,), 77, dtype=torch.int32, device=dev)
    good = dict(region=ptr(rd), h=32, w=32, stride=96, shrink=1, oy=0, ox=0, sh=32, sw=32, bg=220, params=ptr(params), stain=1, j=10, cell=16,
                cells=ptr(cells), rows=ptr(rows), n=1, boxes=ptr(boxes), flags=ptr(flags))
    call = lambda **kw: L.ay_stain_load_u8(*{**good, **kw}.values(), sp)
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    for bad in (dict(region=None), dict(params=None), dict(h=0), dict(w=0), dict(stride=95), dict(shrink=0), dict(shrink=3), dict(bg=-1),
                dict(bg=257), dict(stain=-1), dict(stain=2), dict(j=-1), dict(j=513), dict(cell=lr.MIN_CELL - 1), dict(cell=0),
                dict(cell=lr.MIN_CELL - 1, cells=None), dict(oy=-1), dict(ox=-1), dict(oy=1), dict(ox=1), dict(sh=31), dict(sw=31),
                dict(sh=0), dict(sw=(1 << 24) + 1), dict(sh=(1 << 24) + 1), dict(shrink=2, sh=15), dict(n=-1), dict(rows=None),
                dict(boxes=None), dict(flags=None), dict(cells=odd(cells)), dict(boxes=odd(boxes))):
        assert call(**bad) == -1, bad
        assert _lib.lib().ay_last_error()
    torch.cuda.synchronize()
    assert (cells == 77).all() and (boxes == 77).all() and (flags == 77).all()
    assert call(h=1, shrink=2, sh=1) == 0                            # no halved image: AY_OK, nothing to add
    torch.cuda.synchronize()
    assert (cells == 77).all() and (boxes == 77).all() and (flags == 77).all()
    # the good call is good; at (5, 7) of a 37 x 39 slide (one cell of 64) the box [0, 32) x [0, 32) owns 25 x 27 pixels of the region
    assert call() == 0 and call(shrink=2, sh=16, sw=16) == 0 and call(oy=5, ox=7, sh=37, sw=39, cell=64) == 0
    assert boxes[0].item() == 77 + 32 * 32 + 16 * 16 + 25 * 27 and flags.item() == 77 and cells[-1].item() == 77
    assert cells[0].item() == 77 + 16 * 16 + 16 * 16 + 32 * 32       # tissue of cell (0, 0): every pixel is tissue (90 < 220)


# ---- 5. wsi.stain_load ----------------------------------------------------------------------------------------------------------------
def check_load(got, raster, shrink, bg, stain, thres, cell, rows):
    t = sref.tables()
    j = lr.thres_bin(thres)
    want_c, want_b, want_f = lr.load(raster, shrink, bg, t, stain, j, cell, rows)
    assert 0 < want_c[:, :, 1].sum() < want_c[:, :, 0].sum()
    for i, k in enumerate(("tissue", "positive", "bin_sum")):
        assert got[k].dtype == np.int64 and np.array_equal(got[k], want_c[:, :, i]), k
    assert got["thres"] == j / 64.0 and got["total_load"] == want_c[:, :, 1].sum() / want_c[:, :, 0].sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        np.testing.assert_array_equal(got["load"], want_c[:, :, 1] / np.where(want_c[:, :, 0] > 0, want_c[:, :, 0], np.nan))
    if rows is None:
        assert sorted(got) == ["bin_sum", "load", "positive", "thres", "tissue", "total_load"]
    else:
        assert got["boxes"].dtype == np.int64 and np.array_equal(got["boxes"], want_b) and got["flags"] == int(want_f[0])
    return want_c, want_b


def test_stain_load_through_the_stream(dev):
    raster = region_raster()
    H, W = raster.shape[:2]
    rows = np.concatenate([hand_rows(H, W), lr.random_boxes(150, H, W, 5)])
    got = stain_load(raster, rows, cell=32)
    want, want_b = check_load(got, raster, 1, 220, 1, 0.15, 32, rows)
    assert np.isnan(got["load"]).sum() == (want[:, :, 0] == 0).sum() and (want_b[:, 2] > 0).sum() >= 10
    # the histogram's tail and the tissue map say the same, exactly
    assert stain_stats(raster, probe_stride=1).positive_fraction(1, 0.15)[0] == got["positive"].sum() / got["tissue"].sum() == got["total_load"]
    assert np.array_equal(got["tissue"], tissue_counts(raster, 32))
    # rows on the device; a non-contiguous view of a wider raster; no rows
    on_dev = stain_load(raster, torch.from_numpy(rows).to(dev), cell=32)
    assert all(np.array_equal(on_dev[k], got[k], equal_nan=True) for k in ("tissue", "positive", "bin_sum", "load", "boxes"))
    wide = np.concatenate([raster, 255 - raster], 1)
    view = wide[:, 5:5 + W]
    assert not view.flags["C_CONTIGUOUS"]
    check_load(stain_load(view, None, cell=48, thres=0.62, stain=0, bg_level=200), np.ascontiguousarray(view), 1, 200, 0, 0.62, 48, None)
    # shrink 2 on a tall raster: two strips accumulate, boxes across the cut at halved row 1536
    tall = dark_and_bright(9, 3301, 45)
    rows2 = np.concatenate([lr.random_boxes(60, 1650, 22, 6, cuts=(1536,)), np.asarray([[0, 0, 22, 1650, 1, 1, 0]], np.float32)])
    _, want_b = check_load(stain_load(tall, rows2, cell=16, shrink=2, bg_level=200, thres=0.3), tall, 2, 200, 1, 0.3, 16, rows2)
    assert (want_b[:, 2] > 0).sum() >= 10
    assert stain_load(tall, np.zeros((0, 7), np.float32), cell=64)["boxes"].shape == (0, 4)


# ---- 6. quantify_region(load=True) ----------------------------------------------------------------------------------------------------
def test_quantify_region_with_load(tmp_cfg_dir, dev):
    model = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    F, K, cell = 3, 4, 32
    kw = dict(cell=cell, field=F, top_k=K, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    base = quantify_region(model, raster, **kw)
    assert sorted(base) == sorted(["rows", "counts", "tissue", "fields", "n_found", "totals", "below", "flagged", "flags"])
    got = quantify_region(model, raster, dab_thres=0.15, load=True, **kw)
    new = ["load_tissue", "load_positive", "load_map", "total_load", "box_load", "field_load"]
    assert sorted(got) == sorted(list(base) + new)
    assert torch.equal(got["rows"], base["rows"]) and np.array_equal(got["fields"], base["fields"]) and len(got["rows"]) >= 12
    ld = stain_load(raster, got["rows"], cell=cell, thres=0.15)
    want_c, _ = check_load(ld, raster, 1, 220, 1, 0.15, cell, got["rows"].numpy())
    assert np.array_equal(got["box_load"], ld["boxes"]) and got["box_load"].shape == (len(got["rows"]), 4)
    assert np.array_equal(got["load_tissue"], want_c[:, :, 0]) and np.array_equal(got["load_positive"], want_c[:, :, 1])
    assert np.array_equal(got["load_map"], ld["load"], equal_nan=True) and got["total_load"] == ld["total_load"]
    fl = np.full((3, K), np.nan)                                     # the host sum over the cells of every picked field
    for c in range(3):
        for k in range(int(got["n_found"][c])):
            y, x = got["fields"][c, k, :2] // cell
            tissue = int(want_c[y:y + F, x:x + F, 0].sum())
            if tissue:
                fl[c, k] = int(want_c[y:y + F, x:x + F, 1].sum()) / tissue
    assert got["n_found"].sum() >= 1 and np.isfinite(fl).sum() >= 1
    np.testing.assert_array_equal(got["field_load"], fl)
    # with the statistics as well: both sets of keys, and the two loads agree exactly
    stats = stain_stats(raster, probe_stride=1)
    both = quantify_region(model, raster, stain_stats=stats, dab_thres=0.15, load=True, **kw)
    assert sorted(both) == sorted(list(base) + new + ["dab_positive_fraction", "dab_thres"])
    assert both["dab_positive_fraction"] == both["total_load"] == got["total_load"] and both["dab_thres"] == 10 / 64
