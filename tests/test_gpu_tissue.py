"""Tissue map and tile mask (-m gpu): ay_tile_tissue_u8, ay_ingest_region_tiles_list_u8, wsi.tissue_counts, RegionTileStream and
detect_region with a tile_mask.  Every comparison is exact: integer counts, or tiles / rows that are only selected.

Yardsticks: tests/tissue_reference.py (the rule restated in NumPy) for the counts; the step ingest and tiles cut on the CPU +
oracle/ingest_oracle.ingest for the list ingest and the masked stream; the unmasked detect_region for the masked one; model +
non_max_suppression on CPU-cut tiles filtered by tests/seam_reference.py for the masked overlap path."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import seam_reference as sr
import tissue_reference as tr
import views_reference as vr
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import RegionTileStream, detect_region, tile_grid, tissue_counts
from oracle.ingest_oracle import ingest
from test_gpu_seam import BATCH, CONF, INGEST_CASES, NMS, OVERLAP, S, SEAM, TILE, build_model, cpu_tiles, halve, region_raster

pytestmark = pytest.mark.gpu

BG, GUARD = 170, 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def slide():
    return tr.test_slide(region_raster())


# ---- 1. ay_tile_tissue_u8 ------------------------------------------------------------------------------------------------------
def device_counts(dev, r, shrink, tile, overlap, bg, base=0, pad=0, tiles=None):
    """counts of raster r [H,W,3], placed `base` bytes behind a 16-byte boundary with rows 3 * W + pad bytes apart"""
    H, W = r.shape[:2]
    stride = 3 * W + pad
    host = np.full(base + H * stride, 77, np.uint8)
    np.lib.stride_tricks.as_strided(host[base:], (H, W * 3), (stride, 1))[:] = r.reshape(H, W * 3)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    ty, tx, step = tr.grid(H // shrink, W // shrink, tile, overlap)
    if tiles is not None:
        ty, tx = tiles
    counts = torch.full((ty * tx + GUARD,), -7, device=dev, dtype=torch.int32)
    out = []
    for _ in range(2):
        counts[: ty * tx] = -3   # the call zeroes what it counts into
        check(_lib.lib().ay_tile_tissue_u8(ptr(buf[base:]), H, W, stride, shrink, tile, step, ty, tx, bg, ptr(counts), _lib.stream_ptr()),
              "ay_tile_tissue_u8")
        out.append(counts.cpu().numpy())
    assert out[0].tobytes() == out[1].tobytes()               # two runs, the same bytes
    assert (out[0][ty * tx:] == -7).all()                     # guard words behind the counts untouched
    return out[0][: ty * tx].reshape(ty, tx)


def dark_and_bright(seed, H, W):
    """random pixels, a third of them bright in every channel, so that no level makes the count trivial"""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    bright = rng.random((H, W)) < 0.33
    r[bright] = rng.integers(200, 256, size=(int(bright.sum()), 3), dtype=np.uint8)
    return r


@pytest.mark.parametrize("case", INGEST_CASES, ids=str)
def test_tissue_counts_kernel_on_the_ingest_geometries(dev, case):
    H, W, tile, _, shrink, overlap = case
    r = dark_and_bright(H * 1000 + W + overlap, H, W)
    for bg in (0, 1, 128, 210, 255, 256):
        want = tr.tissue_counts(r, tile, shrink, overlap, bg)
        if bg == 210:
            assert 0 < want.sum() < tr.tissue_counts(r, tile, shrink, overlap, 256).sum()
        for base, pad in ((0, 0), (1, 0), (2, 5), (3, 0), (0, 16 - (3 * W) % 16), (0, 48 - (3 * W) % 16), (16, 7)):
            got = device_counts(dev, r, shrink, tile, overlap, bg, base, pad)
            assert np.array_equal(got, want), (bg, base, pad)
    assert tr.tissue_counts(r, tile, shrink, overlap, 0).sum() == 0
    if overlap == 0:
        assert tr.tissue_counts(r, tile, shrink, overlap, 256).sum() == (H // shrink) * (W // shrink)


def test_tissue_counts_kernel_on_a_full_size_strip(dev):
    """one strip of 1536 rows, a few tiles wide, width no multiple of 16, as the stream calls it (tiles_y = 1)"""
    r = dark_and_bright(11, 1536, 3 * 1536 - 100)
    for overlap in (0, 128):
        want = tr.tissue_counts(r, 1536, 1, overlap, 190)
        assert want.shape[0] == 1 and want.shape[1] == (3 if overlap == 0 else 4) and want.min() > 0
        for base, pad in ((0, 0), (0, 12), (3, 0)):     # 3 * W = 13524: not a multiple of 16, + 12 is
            assert np.array_equal(device_counts(dev, r, 1, 1536, overlap, 190, base, pad), want)
    r2 = dark_and_bright(12, 2 * 96 + 1, 2 * 500 + 1)
    want = tr.tissue_counts(r2, 96, 2, 8, 190, tiles=(1, 6))
    assert np.array_equal(device_counts(dev, r2, 2, 96, 8, 190, 0, 5, tiles=(1, 6)), want)


# ---- 2. ay_ingest_region_tiles_list_u8 -------------------------------------------------------------------------------------------
def list_ingest(dev, rd, H, W, shrink, tile, origins, S_, out):
    o = torch.tensor(origins, dtype=torch.int32, device=dev).reshape(-1, 2)
    check(_lib.lib().ay_ingest_region_tiles_list_u8(ptr(rd), H, W, W * 3, shrink, tile, ptr(o), o.shape[0], S_, ptr(out), _lib.stream_ptr()),
          "ay_ingest_region_tiles_list_u8")
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", INGEST_CASES, ids=str)
def test_list_ingest(dev, case):
    H, W, tile, S_, shrink, overlap = case
    r = np.random.default_rng(H * 1000 + W + overlap).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rd = torch.from_numpy(r).to(dev)
    ty, tx, step = tile_grid(H // shrink, W // shrink, tile, overlap)
    L = _lib.lib()
    # a full grid in grid order: the step kernel, bit for bit
    want = torch.empty(ty * tx, 3, S_, S_, device=dev)
    check(L.ay_ingest_region_tiles_step_u8(ptr(rd), H, W, W * 3, shrink, tile, step, ty, tx, S_, ptr(want), _lib.stream_ptr()), "step")
    got = torch.full((ty * tx + 2, 3, S_, S_), -7.0, device=dev)
    list_ingest(dev, rd, H, W, shrink, tile, [(i * step, j * step) for j in range(ty) for i in range(tx)], S_, got)
    assert torch.equal(got[: ty * tx], want) and (got[ty * tx:] == -7.0).all()
    # a permuted subset, one origin twice, origins on no grid (one of them hangs over the right and bottom edges)
    h, w = H // shrink, W // shrink
    rng = np.random.default_rng(case[0] + case[5])
    grid_o = [(i * step, j * step) for j in range(ty) for i in range(tx)]
    pick = [grid_o[k] for k in rng.permutation(len(grid_o))[: max(1, len(grid_o) // 2)]]
    origins = pick + [pick[0], (1, 2), (w // 3 + 1, h // 2 + 1), (max(w - 5, 0), max(h - 3, 0)),
                      (-3, 2), (4, -5), (-tile + 1, -tile + 2), (-tile, 0)]     # left of and above the region: background there
    rr = halve(r) if shrink == 2 else r
    crops = []
    for x, y in origins:
        t = np.full((tile, tile, 3), 255, np.uint8)
        c = rr[max(y, 0):max(y + tile, 0), max(x, 0):max(x + tile, 0)]
        t[max(-y, 0):max(-y, 0) + c.shape[0], max(-x, 0):max(-x, 0) + c.shape[1]] = c
        crops.append(ingest(t, S_))
    assert (crops[-1] == 1.0).all() and not (crops[-4] == 1.0).all()          # (-tile, 0) lies entirely outside, (-3, 2) does not
    got = torch.full((len(origins) + 3, 3, S_, S_), -7.0, device=dev)
    list_ingest(dev, rd, H, W, shrink, tile, origins, S_, got)
    assert torch.equal(got[: len(origins)].cpu(), torch.stack(crops)) and (got[len(origins):] == -7.0).all()


@pytest.mark.parametrize("shrink", [1, 2])
def test_list_and_views_ingest_at_extreme_origins(dev, shrink):
    """Origins at both ends of int32 through the list entry and the views entry: origin + offset is formed without signed overflow
    and the bounds test gates every read, so such a tile is all background, and a tile at (1, 2) in the same call is its CPU crop."""
    H, W, tile, S_ = 70, 100, 32, 32
    r = np.random.default_rng(7 + shrink).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rd = torch.from_numpy(r).to(dev)
    rr = halve(r) if shrink == 2 else r
    far = [(2**31 - 1, 0), (0, 2**31 - 1), (-2**31, 0), (0, -2**31), (2**31 - 32, 3)]
    origins = far + [(1, 2)]
    t = np.full((tile, tile, 3), 255, np.uint8)
    c = rr[2:2 + tile, 1:1 + tile]
    t[:c.shape[0], :c.shape[1]] = c
    crop = ingest(t, S_)
    assert not (crop == 1.0).all()
    got = torch.full((len(origins) + 1, 3, S_, S_), -7.0, device=dev)
    list_ingest(dev, rd, H, W, shrink, tile, origins, S_, got)
    got = got.cpu()
    assert (got[:len(far)] == 1.0).all() and torch.equal(got[len(far)], crop) and (got[len(far) + 1:] == -7.0).all()
    views = (0, 5)
    o = torch.tensor(origins, dtype=torch.int32, device=dev)
    ids = (C.c_int * len(views))(*views)
    got = torch.full(((len(origins) + 1) * len(views), 3, S_, S_), -7.0, device=dev)
    check(_lib.lib().ay_ingest_region_tiles_views_u8(ptr(rd), H, W, W * 3, shrink, tile, ptr(o), len(origins), ids, len(views), S_, ptr(got),
                                                     _lib.stream_ptr()), "ay_ingest_region_tiles_views_u8")
    got = got.cpu()
    assert (got[:len(far) * 2] == 1.0).all() and (got[len(origins) * 2:] == -7.0).all()
    for i, v in enumerate(views):      # tile-major: the views of the last tile lie one after another
        assert torch.equal(got[len(far) * 2 + i], torch.from_numpy(vr.view_image_fast(crop.numpy(), v))), v


# ---- 3. wsi.tissue_counts through the strip stream ---------------------------------------------------------------------------------
def test_tissue_counts_through_the_stream(slide):
    for overlap in (0, 64):
        want = tr.tissue_counts(slide, TILE, 1, overlap, BG)
        assert int(tr.wanted(want, TILE, 0.01).sum()) == (7 if overlap == 0 else 11)
        got = tissue_counts(slide, TILE, overlap=overlap, bg_level=BG)
        assert got.dtype == np.int32 and np.array_equal(got, want)
        view = slide[::16, ::16]                              # a strided view is a valid raster
        assert not view.flags["C_CONTIGUOUS"]
        assert np.array_equal(tissue_counts(view, TILE // 16, overlap=overlap // 16, bg_level=BG),
                              tr.tissue_counts(view, TILE // 16, 1, overlap // 16, BG))
    r = dark_and_bright(5, 133, 97)                           # shrink 2, odd extents, several strips
    want = tr.tissue_counts(r, 32, 2, 8, 200)
    assert want.shape == (3, 2) and want.min() > 0
    assert np.array_equal(tissue_counts(r, 32, shrink=2, overlap=8, bg_level=200), want)
    with pytest.raises(ValueError):
        tissue_counts(slide, TILE, bg_level=257)


# ---- 4. RegionTileStream(tile_mask=...) ----------------------------------------------------------------------------------------------
def masks_of(slide, overlap):
    """explicit masks from the restatement; their sizes are asserted before the device is looked at"""
    c = tr.tissue_counts(slide, TILE, 1, overlap, BG)
    sel = {m: tr.wanted(c, TILE, m) for m in (0.01, 0.0005, 0.05)}
    assert [int(sel[m].sum()) for m in (0.01, 0.0005, 0.05)] == ([7, 8, 2] if overlap == 0 else [11, 15, 3])   # 15: see test_tissue_cpu
    return sel


@pytest.mark.parametrize("overlap", [0, 64])
def test_masked_stream_yields_the_wanted_tiles(slide, overlap):
    want, (ty, tx, step) = cpu_tiles(slide, TILE, S, 1, overlap)
    for min_tissue, mask in masks_of(slide, overlap).items():
        stream = RegionTileStream(slide, TILE, S, 1, overlap=overlap, tile_mask=mask)
        got, coords, strips = [], [], 0
        for tiles, cs in stream:
            assert tiles.shape[0] == len(cs) > 0
            got.append(tiles.cpu())
            coords += cs
            strips += 1
        idx = np.flatnonzero(mask.ravel())
        assert coords == [(int(k) // tx, int(k) % tx) for k in idx]                          # the wanted tiles, in grid order
        assert strips == int(mask.any(1).sum()) == len(stream)                              # a strip without a wanted tile yields nothing
        assert torch.equal(torch.cat(got), want[torch.from_numpy(idx)])
        full = RegionTileStream(slide, TILE, S, 1, overlap=overlap)
        assert stream._staged_bytes() < full._staged_bytes() == sum(min(TILE, 1000 - j * step) for j in range(ty)) * 1314 * 3
    # an all-True mask yields what no mask yields
    a = [(t.cpu(), cs) for t, cs in RegionTileStream(slide, TILE, S, 1, overlap=overlap)]
    b = [(t.cpu(), cs) for t, cs in RegionTileStream(slide, TILE, S, 1, overlap=overlap, tile_mask=np.ones((ty, tx), np.bool_))]
    assert len(a) == len(b) == ty and all(x[1] == y[1] and torch.equal(x[0], y[0]) for x, y in zip(a, b))
    with pytest.raises(ValueError):
        RegionTileStream(slide, TILE, S, 1, overlap=overlap, tile_mask=np.ones((ty + 1, tx), np.bool_))


# ---- 5. detect_region with a mask ----------------------------------------------------------------------------------------------------
def count_forward_calls(m):
    calls, real = [], m.forward_device

    def wrapper(x, *a, **k):
        calls.append(int(x.shape[0]))
        return real(x, *a, **k)

    m.forward_device = wrapper
    return calls


def same_entries(a, b):
    return len(a) == len(b) and all(x[:2] == y[:2] and torch.equal(x[2], y[2]) for x, y in zip(a, b))


@pytest.mark.parametrize("batch_size", [3, 4])
def test_detect_region_with_a_mask_is_the_unmasked_result_on_the_wanted_tiles(tmp_cfg_dir, dev, slide, batch_size):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    mask = masks_of(slide, 0)[0.01]
    assert mask[1, 2:5].all() and not mask[1, :2].any() and mask[0].sum() == 1   # batch_size 3: strip 1's tiles straddle a batch boundary
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=batch_size)
    full = detect_region(m, slide, **kw)
    calls = count_forward_calls(m)
    try:
        got = detect_region(m, slide, tile_mask=mask, **kw)
        assert len(calls) == math.ceil(7 / batch_size) and sum(calls) == 7 and max(calls) == batch_size
        del calls[:]
        assert detect_region(m, slide, tile_mask=np.zeros_like(mask), **kw) == [] and calls == []
    finally:
        del m.forward_device
    expect = [e for e in full if mask[e[0], e[1]]]
    assert len(expect) >= 1 and len(full) > len(expect)      # a wanted tile has detections, an unwanted one has an entry in the full run
    assert [e[:2] for e in got] == sorted(e[:2] for e in got) and same_entries(got, expect)
    # the one-call form
    assert same_entries(detect_region(m, slide, min_tissue=0.01, bg_level=BG, probe_stride=1, **kw), expect)
    assert same_entries(detect_region(m, slide, min_tissue=0.01, bg_level=BG, probe_stride=16, **kw), expect)
    coarse = tr.wanted(tr.tissue_counts(slide[::32, ::32], TILE // 32, 1, 0, BG), TILE // 32, 0.01)
    assert int(coarse.sum()) == 4
    assert same_entries(detect_region(m, slide, min_tissue=0.01, bg_level=BG, probe_stride=32, **kw), [e for e in full if coarse[e[0], e[1]]])
    with pytest.raises(ValueError):
        detect_region(m, slide, min_tissue=0.01, bg_level=BG, probe_stride=10, **kw)
    with pytest.raises(ValueError):
        detect_region(m, slide, tile_mask=mask[:, :-1], **kw)


def wanted_tile_rows(m, slide, mask, overlap, batch_size):
    """test_gpu_seam.per_tile_rows for the wanted tiles, in the batches the masked path forms: `batch_size` wanted tiles in grid
    order, across strips"""
    from amyloid_yolo_paper_amd.utils import non_max_suppression
    want, (ty, tx, step) = cpu_tiles(slide, TILE, S, 1, overlap)
    idx = np.flatnonzero(mask.ravel())
    det = []
    for s0 in range(0, len(idx), batch_size):
        det += list(non_max_suppression(m(want[torch.from_numpy(idx[s0:s0 + batch_size])]), CONF, NMS))
    rows, tid = [], []
    for t, d in zip(idx, det):
        if d is not None:
            d = d.clone()
            d[:, :4] *= TILE / S
            d[:, [0, 2]] += (int(t) % tx) * step
            d[:, [1, 3]] += (int(t) // tx) * step
            rows.append(d)
            tid += [int(t)] * len(d)
    return torch.cat(rows), np.asarray(tid, np.int32), tx


@pytest.mark.parametrize("batch_size", [3, 4])
def test_detect_region_with_a_mask_and_overlap(tmp_cfg_dir, dev, slide, batch_size):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    mask = masks_of(slide, OVERLAP)[0.01]
    rows, tid, tx = wanted_tile_rows(m, slide, mask, OVERLAP, batch_size)
    keep = sr.seam_merge(rows.numpy(), tid, SEAM)
    print(f"rows {len(rows)} of {len(np.unique(tid))} tiles, dropped by the seam rule {int((~keep).sum())}")
    assert (~keep).sum() >= 1
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=batch_size, overlap=OVERLAP, seam_thres=SEAM)
    calls = count_forward_calls(m)
    try:
        res = detect_region(m, slide, tile_mask=mask, **kw)
        assert len(calls) == math.ceil(11 / batch_size) and sum(calls) == 11
        del calls[:]
        assert detect_region(m, slide, tile_mask=np.zeros_like(mask), **kw) == [] and calls == []
    finally:
        del m.forward_device
    expect = {}
    for t in np.unique(tid[keep]):
        expect[(int(t) // tx, int(t) % tx)] = rows[torch.from_numpy(keep & (tid == t))]
    assert [(a, b_) for a, b_, _ in res] == sorted(expect)
    for a, b_, d in res:
        assert mask[a, b_] and torch.equal(d, expect[(a, b_)])
    assert same_entries(detect_region(m, slide, min_tissue=0.01, bg_level=BG, probe_stride=16, **kw), res)


def test_default_arguments_are_the_present_path(tmp_cfg_dir, dev):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    a = detect_region(m, raster, **kw)                        # the call of test_detect_region_without_overlap_is_the_present_path
    assert len(a) > 0
    for _ in range(2):
        b = detect_region(m, raster, tile_mask=None, min_tissue=0, **kw)
        assert len(a) == len(b) and all(x[:2] == y[:2] and x[2].numpy().tobytes() == y[2].numpy().tobytes() for x, y in zip(a, b))
    ty, tx, _ = tile_grid(raster.shape[0], raster.shape[1], TILE)
    assert same_entries(detect_region(m, raster, tile_mask=np.ones((ty, tx), np.bool_), **kw), a)
    ty, tx, _ = tile_grid(raster.shape[0], raster.shape[1], TILE, OVERLAP)
    c = detect_region(m, raster, overlap=OVERLAP, seam_thres=SEAM, **kw)
    assert same_entries(detect_region(m, raster, overlap=OVERLAP, seam_thres=SEAM, tile_mask=np.ones((ty, tx), np.bool_), **kw), c)
