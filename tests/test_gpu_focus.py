"""Focus map (-m gpu): ay_focus_u8, wsi.focus_map, wsi.quantify_region(focus=True).  Every comparison is exact: integers, or bytes.
Yardstick: tests/focus_reference.py, THE FOCUS RULE restated in NumPy int64."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import focus_reference as fr
import load_reference as lr
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import focus_map, quantify_region
from test_gpu_seam import BATCH, CONF, NMS, S, TILE, build_model, region_raster
from test_gpu_stain import placed

pytestmark = pytest.mark.gpu

GUARD = 16
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


def aligned_pad(width):
    """the pad that makes rows of `width` pixels a multiple of 16 bytes apart (never 0, so that the tight stride is another case)"""
    assert (3 * width) % 16
    return 16 - (3 * width) % 16


def device_focus(dev, region, shrink, origin_y, slide, own, bg, cell, base, pad, cells, rows=None, boxes=None, flags=None):
    """one call on `region` (source rows), which holds rows origin_y .. of the (halved) slide (H, W)"""
    buf, stride = placed(dev, region, base, pad)
    M = 0 if rows is None else int(rows.shape[0])
    return _lib.lib().ay_focus_u8(ptr(buf), region.shape[0], region.shape[1], stride, shrink, origin_y, slide[0], slide[1], own[0], own[1], bg,
                                  cell, ptr(cells), ptr(rows), M, ptr(boxes), ptr(flags), _lib.stream_ptr())


def whole(dev, r, shrink, bg, cell, base, pad, rows=None):
    """the slide in one call that owns every row -> cells [Gy, Gx, 3] (and boxes, flags), guard words checked"""
    H, W = r.shape[0] // shrink, r.shape[1] // shrink
    gy, gx = fr.grid(H, W, cell)
    n = gy * gx * 3
    cells = guarded(dev, n)
    M = 0 if rows is None else len(rows)
    boxes, flags = guarded(dev, M * 3), torch.tensor([0, -7], device=dev, dtype=torch.int32)
    assert device_focus(dev, r, shrink, 0, (H, W), (0, H), bg, cell, base, pad, cells, None if rows is None else torch.from_numpy(rows).to(dev),
                        boxes if M else None, flags if M else None) == 0
    got, got_b = cells.cpu().numpy(), boxes.cpu().numpy()
    assert (got[n:] == -7).all() and (got_b[M * 3:] == -7).all() and flags[1].item() == -7
    return got[:n].reshape(gy, gx, 3), got_b[:M * 3].reshape(M, 3), int(flags[0].item())


# ---- 1. the cell pass -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_cell_pass_against_the_reference(dev, shrink):
    """97 x 131 pixels of the (halved) slide (195 x 263 source pixels for shrink 2: both odd), glass punched in; the tight stride is
    no multiple of 16 (byte loads), the padded one is (16-byte loads); both must give the reference's sums"""
    shape = (97, 131) if shrink == 1 else (195, 263)
    r = fr.glass_blobs(fr.texture(*shape, 7, 20, 256), 8, n=10, radius=(2, 6 * shrink + 4))
    seen = set()
    for bg, cell in itertools.product((0, 220, 256), (16, 40)):
        want, _, _ = fr.focus(r, shrink, bg, cell)
        if bg == 0:
            assert want.sum() == 0
        if bg == 256:
            assert want[:, :, 0].sum() == 95 * 129
        if bg == 220:
            assert 1000 < want[:, :, 0].sum() < 95 * 129 - 500 and (want[:, :, 1] < 0).any() and (want[:, :, 1] > 0).any()
        for base, pad in ((0, 0), (0, aligned_pad(shape[1])), (3, 5)):
            runs = [whole(dev, r, shrink, bg, cell, base, pad)[0] for _ in range(2)]
            assert runs[0].tobytes() == runs[1].tobytes(), (bg, cell, base, pad)             # two runs, the same bytes
            assert np.array_equal(runs[0], want), (bg, cell, base, pad)
            seen.add((base == 0 and (3 * shape[1] + pad) % 16 == 0))
    assert seen == {False, True}


@pytest.mark.parametrize("shape,shrink", [((40, 4200), 1), ((40, 4300), 2)], ids=str)
def test_cell_pass_on_rows_longer_than_a_work_unit(dev, shape, shrink):
    """a work unit spans 32 items of 48 bytes, 512 pixels (256 halved): these rows are walked in nine units, and the stencil reads
    across every border between them; 40 (20) rows are two bands"""
    r = fr.glass_blobs(fr.texture(*shape, 9, 20, 256), 10, n=40, radius=(2, 9))
    H, W = shape[0] // shrink, shape[1] // shrink
    assert W > 8 * 512 // shrink
    for cell in (16, 100):
        want, _, _ = fr.focus(r, shrink, 220, cell)
        gx = want.shape[1]
        assert (want[:, :, 0] > 0).sum() > 0.5 * want.shape[0] * gx and 0 < want[:, :, 0].sum() < (H - 2) * (W - 2)
        for base, pad in ((0, 0), (0, aligned_pad(shape[1]))):
            assert np.array_equal(whole(dev, r, shrink, 220, cell, base, pad)[0], want), (cell, base, pad)


def test_sums_beyond_32_bits(dev):
    """64 x 4200 pixels that alternate between 0 and 255, all tissue at bg_level 256, in two cells of 4096 columns: every Laplacian is
    +-1020, s2 = 62 * 4198 * 1 040 400 = 270 791 150 400 and the first cell alone holds 2^37.9: no 32-bit accumulator can carry it"""
    r = fr.checkerboard(64, 4200)
    want, _, _ = fr.focus(r, 1, 256, 4096)
    assert want.shape == (1, 2, 3) and want[:, :, 2].sum() == 270791150400 and want[:, :, 0].sum() == 62 * 4198 and want[:, :, 1].sum() == 0
    assert want[0, 0, 2] == 62 * 4095 * 1040400 > 1 << 37
    for base, pad in ((0, 0), (0, aligned_pad(4200))):
        assert np.array_equal(whole(dev, r, 1, 256, 4096, base, pad)[0], want), (base, pad)
    rows = np.asarray([[0, 0, 4200, 64, 1, 1, 0]], np.float32)                     # one box over all of it: the same on one wavefront
    _, got_b, _ = whole(dev, r, 1, 256, 4096, 0, 0, rows)
    assert got_b.tolist() == [[62 * 4198, 0, 270791150400]]


# ---- 2. ownership ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_two_calls_on_the_rows_each_needs_give_the_whole_image(dev, shrink):
    shape = (41, 75) if shrink == 1 else (83, 151)
    r = fr.glass_blobs(fr.texture(*shape, 12, 20, 256), 13, n=6, radius=(2, 4 * shrink + 2))
    H, W = shape[0] // shrink, shape[1] // shrink
    want, _, _ = fr.focus(r, shrink, 220, 16)
    assert want[:, :, 0].sum() > 500
    noise = np.random.default_rng(14).integers(0, 256, size=r.shape, dtype=np.uint8)
    for k, (base, pad) in itertools.product((1, 2, 15, 16, 17, H - 2), ((0, 0), (0, aligned_pad(shape[1])))):
        cells = guarded(dev, want.size)
        first = np.zeros(want.size + GUARD, np.int64)
        for a, b in ((0, k), (k, H)):
            lo, hi = max(a, 1) - 1, min(b, H - 1)            # the rows the call needs: lo .. hi
            region = r[lo * shrink:(hi + 1) * shrink] if max(a, 1) < min(b, H - 1) else r[:shrink]       # nothing owned: any region
            origin = lo if max(a, 1) < min(b, H - 1) else 0
            assert device_focus(dev, region, shrink, origin, (H, W), (a, b), 220, 16, base, pad, cells) == 0, (k, a, b)
            if a == 0:
                first = cells.cpu().numpy()
        got = cells.cpu().numpy()
        assert np.array_equal(got[:want.size].reshape(want.shape), want) and (got[want.size:] == -7).all(), (k, base, pad)
        assert k == 1 or (0 < first[:want.size].sum() and not np.array_equal(first, got))          # both calls had a share
        # the same two calls on the whole raster, every row outside own_y0 - 1 .. own_y1 overwritten: the same bytes
        cells = guarded(dev, want.size)
        for a, b in ((0, k), (k, H)):
            dirty = noise.copy()
            dirty[max(a - 1, 0) * shrink:(b + 1) * shrink] = r[max(a - 1, 0) * shrink:(b + 1) * shrink]
            assert device_focus(dev, dirty, shrink, 0, (H, W), (a, b), 220, 16, base, pad, cells) == 0
        assert cells.cpu().numpy().tobytes() == got.tobytes(), (k, base, pad)


def test_a_call_adds(dev):
    r = fr.glass_blobs(fr.texture(50, 67, 15, 20, 256), 16, n=5)
    rows = lr.random_boxes(50, 50, 67, 17)
    want_c, want_b, _ = fr.focus(r, 1, 220, 24, rows)
    assert want_b[:, 0].sum() > 0 and (want_c[:, :, 1] != 0).any()
    cells, boxes = guarded(dev, want_c.size), guarded(dev, want_b.size)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)
    d_rows = torch.from_numpy(rows).to(dev)
    for times in (1, 2):
        assert device_focus(dev, r, 1, 0, (50, 67), (0, 50), 220, 24, 0, 0, cells, d_rows, boxes, flags) == 0
        got_c, got_b = cells.cpu().numpy(), boxes.cpu().numpy()
        assert np.array_equal(got_c[:want_c.size].reshape(want_c.shape), times * want_c) and (got_c[want_c.size:] == -7).all()
        assert np.array_equal(got_b[:want_b.size].reshape(want_b.shape), times * want_b) and (got_b[want_b.size:] == -7).all()


# ---- 3. the box pass ------------------------------------------------------------------------------------------------------------------
def hand_rows(H, W):
    row = lambda x1, y1, x2, y2: [x1, y1, x2, y2, 0.9, 0.9, 0.0]
    return np.asarray([row(10.5, 10.5, 11.5, 11.5), row(10.5, 10.5, 10.5, 30.0), row(0.0, 0.0, W, H), row(-7.3, -1e9, 4.5, 2.49),
                       row(W - 2.5, H - 1.5, 1e9, 3e38), row(30.0, 40.0, 20.0, 50.0), row(20.0, 50.0, 30.0, 40.0), row(NAN, 1.0, 5.0, 5.0),
                       row(1.0, 1.0, INF, 5.0), row(1.0, -INF, 5.0, 5.0), row(3.2, 12.6, 40.0, 14.4), row(W + 5.0, 3.0, W + 9.0, 8.0),
                       row(10.49, 10.51, 11.51, 11.49), row(2.0, 5.0, 30.0, 25.0)], np.float32)


@pytest.mark.parametrize("shrink", [1, 2])
def test_box_pass_on_one_region_and_on_three_uneven_ranges(dev, shrink):
    """fractional edges, boxes off the slide, empty and inverted boxes, boxes across the splits at rows 13 and 14, a NaN row and two
    inf rows (flagged, zeros); on one call and on three calls that own rows 0 .. 12, 13 and 14 .. of regions that hold what each needs"""
    shape = (97, 131) if shrink == 1 else (195, 263)
    r = fr.glass_blobs(fr.texture(*shape, 18, 20, 256), 19, n=8, radius=(2, 5 * shrink + 2))
    H, W = 97, 131
    rows = np.concatenate([hand_rows(H, W), lr.random_boxes(200, H, W, 20 + shrink, cuts=(13, 14))])
    M = len(rows)
    d_rows = torch.from_numpy(rows).to(dev)
    want_c, want_b, want_f = fr.focus(r, shrink, 220, 24, rows)
    assert want_f[0] == fr.FLAG_NONFINITE and (want_b[:, 0] > 0).sum() > 150 and (want_b[7:10] == 0).all() and (want_b[[1, 5, 6, 11, 12]] == 0).all()
    assert want_b[2].tolist() == want_c.sum((0, 1)).tolist() and 0 < want_b[13, 0] <= 28 * 20         # the slide; a box of 28 x 20 pixels
    for ranges in (((0, H),), ((0, 13), (13, 14), (14, H))):
        for with_cells in (True, False):
            cells, boxes = guarded(dev, want_c.size), guarded(dev, M * 3)
            flags = torch.tensor([0, -7], device=dev, dtype=torch.int32)
            for a, b in ranges:
                lo, hi = max(a, 1) - 1, min(b, H - 1)
                assert device_focus(dev, r[lo * shrink:(hi + 1) * shrink], shrink, lo, (H, W), (a, b), 220, 24, 0, 0,
                                    cells if with_cells else None, d_rows, boxes, flags) == 0
            got_b, got_c = boxes.cpu().numpy(), cells.cpu().numpy()
            assert np.array_equal(got_b[:M * 3].reshape(M, 3), want_b) and (got_b[M * 3:] == -7).all(), (ranges, with_cells)
            assert flags.tolist() == [fr.FLAG_NONFINITE, -7]
            assert np.array_equal(got_c[:want_c.size].reshape(want_c.shape), want_c if with_cells else 0 * want_c)
            assert (got_c[want_c.size:] == -7).all()
    # n_rows == 0 with NULL rows, boxes and flags: legal, and only the cells are written
    assert np.array_equal(whole(dev, r, shrink, 220, 24, 0, 0)[0], want_c)


# ---- 4. a captured HIP graph ----------------------------------------------------------------------------------------------------------
def test_hip_graph_of_one_call_replays_on_other_bytes(dev):
    """one call with cells and boxes captured on one stream (no side branches) and replayed onto re-zeroed outputs: launches only"""
    H, W, M, cell = 97, 131, 120, 24
    rasters = [fr.glass_blobs(fr.texture(H, W, 30 + k, 20, 256), 40 + k) for k in range(3)]
    inputs = [lr.random_boxes(M, H, W, 70 + k) for k in range(3)]
    rd = torch.from_numpy(rasters[0]).to(dev)
    rows = torch.from_numpy(inputs[0]).to(dev)
    gy, gx = fr.grid(H, W, cell)
    cells = torch.zeros(gy, gx, 3, device=dev, dtype=torch.int64)
    boxes = torch.zeros(M, 3, device=dev, dtype=torch.int64)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def step():
        check(_lib.lib().ay_focus_u8(ptr(rd), H, W, W * 3, 1, 0, H, W, 0, H, 220, cell, ptr(cells), ptr(rows), M, ptr(boxes), ptr(flags),
                                     _lib.stream_ptr()), "ay_focus_u8")

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
        rd.copy_(torch.from_numpy(rasters[k]))
        g.replay()
        torch.cuda.synchronize()
        want_c, want_b, want_f = fr.focus(rasters[k], 1, 220, cell, inputs[k])
        assert want_b[:, 0].sum() > 0
        np.testing.assert_array_equal(cells.cpu().numpy(), want_c)
        np.testing.assert_array_equal(boxes.cpu().numpy(), want_b)
        assert int(flags.item()) == int(want_f[0]) == 0


# ---- 5. bad arguments through the C ABI -----------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one_and_leave_the_outputs_alone(dev):
    L, sp = _lib.lib(), _lib.stream_ptr()
    rd = torch.full((32, 32, 3), 90, dtype=torch.uint8, device=dev)
    rows = torch.tensor([[0, 0, 32, 32, 1, 1, 0]], dtype=torch.float32, device=dev)
    cells = torch.full((3 * 2 * 3 + 1,), 77, dtype=torch.int64, device=dev)      # the largest grid below: 40 x 32 in cells of 16
    boxes = torch.full((3 + 1,), 77, dtype=torch.int64, device=dev)
    flags = torch.full((1,), 77, dtype=torch.int32, device=dev)
    good = dict(region=ptr(rd), h=32, w=32, stride=96, shrink=1, oy=0, sh=32, sw=32, y0=0, y1=32, bg=220, cell=16, cells=ptr(cells),
                rows=ptr(rows), n=1, boxes=ptr(boxes), flags=ptr(flags))
    call = lambda **kw: L.ay_focus_u8(*{**good, **kw}.values(), sp)
    odd = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    for bad in (dict(region=None), dict(h=0), dict(w=0), dict(stride=95), dict(shrink=0), dict(shrink=3), dict(bg=-1), dict(bg=257),
                dict(cell=fr.MIN_CELL - 1), dict(cell=0), dict(cell=fr.MIN_CELL - 1, cells=None), dict(oy=-1), dict(oy=1), dict(sh=31),
                dict(sw=31), dict(sw=33), dict(sh=0), dict(sh=(1 << 24) + 1), dict(sw=(1 << 24) + 1), dict(shrink=2, sh=16), dict(n=-1),
                dict(rows=None), dict(boxes=None), dict(flags=None), dict(cells=odd(cells)), dict(boxes=odd(boxes)), dict(y0=-1),
                dict(y0=5, y1=4), dict(y1=33), dict(sh=40, y1=40),
                # a needed halo row that is not resident: below (rows 0 .. 32 of a region that holds 0 .. 31) and above (row 7 of 8 .. 39)
                dict(sh=40, y1=32), dict(sh=40, y1=33), dict(sh=40, oy=8, y0=8, y1=39), dict(sh=40, oy=8, y0=0, y1=20)):
        assert call(**bad) == -1, bad
        assert _lib.lib().ay_last_error()
    torch.cuda.synchronize()
    assert (cells == 77).all() and (boxes == 77).all() and (flags == 77).all()
    # nothing owned: AY_OK, nothing to add, and no row is needed (a range outside 1 .. H - 2, an empty range)
    assert call(y0=0, y1=1) == 0 and call(y0=31, y1=32) == 0 and call(y0=9, y1=9) == 0 and call(sh=40, oy=8, y0=39, y1=40) == 0
    torch.cuda.synchronize()
    assert (cells == 77).all() and (boxes == 77).all() and (flags == 77).all()
    # the good calls: all 30 x 30 evaluated pixels are flat (lap 0); rows 9 .. 38 of a 40-row slide from a region at row 8; the halved image
    assert call() == 0 and call(sh=40, oy=8, y0=9, y1=40) == 0 and call(sh=40, y1=31) == 0
    assert call(shrink=2, sh=16, sw=16, y1=16) == 0
    torch.cuda.synchronize()
    assert boxes.tolist() == [77 + 30 * 30 + 30 * 23 + 30 * 30 + 14 * 14, 77, 77, 77] and flags.item() == 77 and cells[-1].item() == 77
    assert cells[0].item() == 77 + 15 * 15 + 15 * 7 + 15 * 15 + 14 * 14     # cell (0, 0) of each of the four calls


# ---- 6. wsi.focus_map -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_focus_map_gives_the_reference_on_any_strip_height(dev, shrink):
    shape = (97, 131) if shrink == 1 else (195, 263)
    r = fr.glass_blobs(fr.texture(*shape, 50, 20, 256), 51, n=10, radius=(2, 6 * shrink + 4))
    H, W = 97, 131
    rows = np.concatenate([hand_rows(H, W), lr.random_boxes(100, H, W, 52, cuts=(15, 16, 30))])
    want_c, want_b, want_f = fr.focus(r, shrink, 220, 40, rows)
    assert (want_b[:, 0] > 0).sum() > 60
    first = None
    for strip in (3, 17, H, 1536):
        got = focus_map(r, rows, cell=40, shrink=shrink, strip=strip)
        assert sorted(got) == ["box_sharpness", "boxes", "flags", "n", "s1", "s2", "sharpness"]
        for i, k in enumerate(("n", "s1", "s2")):
            assert got[k].dtype == np.int64 and np.array_equal(got[k], want_c[:, :, i]), (strip, k)
        assert got["boxes"].dtype == np.int64 and np.array_equal(got["boxes"], want_b) and got["flags"] == int(want_f[0]) == 1
        np.testing.assert_array_equal(got["sharpness"], fr.sharpness(want_c[:, :, 0], want_c[:, :, 1], want_c[:, :, 2]))
        np.testing.assert_array_equal(got["box_sharpness"], fr.sharpness(want_b[:, 0], want_b[:, 1], want_b[:, 2]))
        first = first or got
        assert all(got[k].tobytes() == first[k].tobytes() for k in got if k != "flags")
    assert np.isnan(first["box_sharpness"][7:10]).all() and np.isfinite(first["sharpness"]).sum() >= 6
    # without rows; rows on the device; a non-contiguous view of a wider raster
    plain = focus_map(r, None, cell=40, shrink=shrink, strip=17)
    assert sorted(plain) == ["n", "s1", "s2", "sharpness"] and np.array_equal(plain["s2"], want_c[:, :, 2])
    on_dev = focus_map(r, torch.from_numpy(rows).to(dev), cell=40, shrink=shrink, strip=17)
    assert np.array_equal(on_dev["boxes"], want_b)
    wide = np.concatenate([r, 255 - r], 1)
    view = wide[:, 5:5 + shape[1]]
    assert not view.flags["C_CONTIGUOUS"]
    want_v, _, _ = fr.focus(np.ascontiguousarray(view), shrink, 200, 16)
    got_v = focus_map(view, None, cell=16, shrink=shrink, bg_level=200, strip=30)
    assert all(np.array_equal(got_v[k], want_v[:, :, i]) for i, k in enumerate(("n", "s1", "s2")))
    assert focus_map(r, np.zeros((0, 7), np.float32), cell=64, shrink=shrink)["boxes"].shape == (0, 3)


# ---- 7. quantify_region(focus=True) ---------------------------------------------------------------------------------------------------
def test_quantify_region_with_focus(tmp_cfg_dir, dev):
    model = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    F, K, cell = 3, 4, 32
    kw = dict(cell=cell, field=F, top_k=K, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    base = quantify_region(model, raster, **kw)
    parent_keys = ["rows", "counts", "tissue", "fields", "n_found", "totals", "below", "flagged", "flags"]
    assert sorted(base) == sorted(parent_keys) and sorted(quantify_region(model, raster, focus=False, **kw)) == sorted(parent_keys)
    got = quantify_region(model, raster, focus=True, **kw)
    new = ["focus_n", "focus_sharpness", "box_sharpness", "field_sharpness"]
    assert sorted(got) == sorted(parent_keys + new)
    assert torch.equal(got["rows"], base["rows"]) and np.array_equal(got["fields"], base["fields"]) and len(got["rows"]) >= 12
    assert np.array_equal(got["tissue"], base["tissue"]) and torch.equal(got["counts"], base["counts"])
    fm = focus_map(raster, got["rows"], cell=cell)
    want_c, want_b, _ = fr.focus(raster, 1, 220, cell, got["rows"].numpy())
    assert np.array_equal(fm["n"], want_c[:, :, 0]) and np.array_equal(fm["s2"], want_c[:, :, 2]) and np.array_equal(fm["boxes"], want_b)
    assert want_c[:, :, 0].sum() > 10000
    assert np.array_equal(got["focus_n"], fm["n"]) and np.array_equal(got["focus_sharpness"], fm["sharpness"], equal_nan=True)
    assert got["box_sharpness"].shape == (len(got["rows"]),) and np.array_equal(got["box_sharpness"], fm["box_sharpness"], equal_nan=True)
    fs = np.full((3, K), np.nan)                                     # the pooled variance over the cells of every picked field
    for c in range(3):
        for k in range(int(got["n_found"][c])):
            y, x = got["fields"][c, k, :2] // cell
            n, s1, s2 = (int(v) for v in want_c[y:y + F, x:x + F].sum((0, 1)))
            if n:
                fs[c, k] = s2 / n - (s1 / n) ** 2
    assert got["n_found"].sum() >= 1 and np.isfinite(fs).sum() >= 1
    np.testing.assert_array_equal(got["field_sharpness"], fs)
    # with a threshold: the classification of wsi.focus_summary; with the load as well: both sets of keys
    cut = float(np.nanmedian(fm["sharpness"]))
    both = quantify_region(model, raster, focus=True, min_sharpness=cut, dab_thres=0.15, load=True, **kw)
    load_keys = ["load_tissue", "load_positive", "load_map", "total_load", "box_load", "field_load"]
    assert sorted(both) == sorted(parent_keys + new + load_keys + ["in_focus", "in_focus_fraction"])
    with np.errstate(invalid="ignore"):
        assert np.array_equal(both["in_focus"], (fm["n"] >= 1) & (fm["sharpness"] >= cut)) and 0 < both["in_focus"].sum() < both["in_focus"].size
    assert both["in_focus_fraction"] == int(fm["n"][both["in_focus"]].sum()) / int(fm["n"].sum())
    assert np.array_equal(both["focus_n"], fm["n"]) and np.array_equal(both["fields"], base["fields"])
