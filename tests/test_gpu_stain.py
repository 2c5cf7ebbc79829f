"""Stain normalisation (-m gpu): ay_stain_hist_u8, ay_ingest_region_tiles_stain_u8, ay_stain_apply_u8, wsi.stain_stats,
wsi.normalize_region, RegionTileStream / detect_region / quantify_region with a stain map.  Every comparison is exact -- integer
counts, bytes, or fp32 values that tests/stain_reference.py (THE STAIN RULE restated in NumPy fp32) gives bit for bit -- but for the
one against the plain cut, whose bound of 1.7e-4 is derived in tests/test_stain_cpu.py.

Yardsticks: tests/stain_reference.py for the histograms, the map and the cut; tests/tissue_reference.py and ay_tile_tissue_u8 for the
tissue totals; model + non_max_suppression on the reference's tiles, filtered by tests/seam_reference.py and mapped back by
tests/views_reference.py, for detect_region."""
import ctypes as C

import numpy as np
import pytest
import torch

import seam_reference as sr
import stain_reference as sref
import tissue_reference as tr
import views_reference as vr
from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.utils import non_max_suppression
from amyloid_yolo_paper_amd.views import ALL_VIEWS, FLIPS
from amyloid_yolo_paper_amd.wsi import (H_DAB, RegionTileStream, StainMap, StainStats, detect_region, normalize_region, quantify_region,
                                        stain_stats, tile_grid)
from test_gpu_seam import BATCH, CONF, NMS, OVERLAP, S, SEAM, TILE, build_model, region_raster
from test_gpu_tissue import dark_and_bright

pytestmark = pytest.mark.gpu

GUARD = 16
BOUND = 1.7e-4          # tests/test_stain_cpu.py: the table's interpolation error, 1.63e-4, plus fp32 rounding
GAINS = ((1.0, 1.0), (1.3, 0.7), (4.0, 0.25))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def stain_map(gains):
    """a StainMap with exactly these gains: source strengths (1, 1), the gains as target"""
    h = np.zeros((2, 512), np.int64)
    h[:, 63] = 1
    m = StainMap(StainStats(h, 1), gains, max_gain=4.0)
    assert m.gains == tuple(gains)
    return m


def placed(dev, r, base, pad):
    """raster r [H,W,3] on the device, `base` bytes behind a 16-byte boundary with rows 3 * W + pad bytes apart -> (tensor, stride)"""
    H, W = r.shape[:2]
    stride = 3 * W + pad
    host = np.full(base + H * stride, 77, np.uint8)
    np.lib.stride_tricks.as_strided(host[base:], (H, W * 3), (stride, 1))[:] = r.reshape(H, W * 3)
    buf = torch.from_numpy(host).to(dev)
    assert buf.data_ptr() % 16 == 0
    return buf[base:], stride


# ---- 1. ay_stain_hist_u8 -----------------------------------------------------------------------------------------------------------
def hist_rasters(H, W):
    one = np.empty((H, W, 3), np.uint8)
    one[:] = (150, 90, 60)                                    # every count in one bin per stain: the LDS atomics collide
    prim = np.random.default_rng(H).integers(0, 2, size=(H, W, 3)).astype(np.uint8) * 255      # saturated primaries: the top bins
    return {"random": dark_and_bright(H + W, H, W), "one colour": one, "primaries": prim}


def device_hist(dev, params, r, shrink, bg, base, pad, hist):
    buf, stride = placed(dev, r, base, pad)
    check(_lib.lib().ay_stain_hist_u8(ptr(buf), r.shape[0], r.shape[1], stride, shrink, bg, ptr(params), ptr(hist), _lib.stream_ptr()),
          "ay_stain_hist_u8")


def tissue_total(dev, r, shrink, bg):
    """ay_tile_tissue_u8 with one tile that covers the region"""
    H, W = r.shape[:2]
    rd = torch.from_numpy(r).to(dev)
    counts = torch.empty(1, device=dev, dtype=torch.int32)
    side = max(H, W)
    check(_lib.lib().ay_tile_tissue_u8(ptr(rd), H, W, W * 3, shrink, side, side, 1, 1, bg, ptr(counts), _lib.stream_ptr()), "ay_tile_tissue_u8")
    return int(counts.item())


@pytest.mark.parametrize("shape", [(97, 131), (200, 304)], ids=str)
def test_histogram_kernel(dev, shape):
    params = StainMap.identity().params
    t = sref.tables()
    top = 0
    for name, r in hist_rasters(*shape).items():
        other = np.ascontiguousarray(r[::-1, ::-1] // 2 + 40)                       # the "next strip": other pixels, other bins
        for shrink in (1, 2):
            for bg in (0, 170, 256):
                want, want2 = sref.hist(r, shrink, bg, t), sref.hist(other, shrink, bg, t)
                n = int(want[1024])
                assert n == want[:512].sum() == want[512:1024].sum() == int(tr.tissue(r, shrink, bg).sum())
                if bg == 256:
                    assert n == (shape[0] // shrink) * (shape[1] // shrink)
                    if name == "one colour":
                        assert (want[:512] > 0).sum() == 1 and (want[512:1024] > 0).sum() == 1
                    top = max(top, int((np.flatnonzero(want[:1024]) % 512).max()))
                if bg == 0:
                    assert n == 0
                assert n == tissue_total(dev, r, shrink, bg)
                for base, pad in ((0, 0), (0, 7), (5, 0), (5, 7)):
                    runs = []
                    for _ in range(2):
                        hist = torch.full((1025 + GUARD,), -7, device=dev, dtype=torch.int64)
                        hist[:1025] = 0                                               # the caller zeroes what is added to
                        device_hist(dev, params, r, shrink, bg, base, pad, hist)
                        runs.append(hist.cpu().numpy())
                    assert runs[0].tobytes() == runs[1].tobytes()                     # two runs, the same bytes
                    assert (runs[0][1025:] == -7).all()                               # guard words behind hist untouched
                    assert np.array_equal(runs[0][:1025], want), (name, shrink, bg, base, pad)
                    device_hist(dev, params, other, shrink, bg, base, pad, hist)      # a second call adds
                    got = hist.cpu().numpy()
                    assert np.array_equal(got[:1025], want + want2) and (got[1025:] == -7).all(), (name, shrink, bg, base, pad)
    assert top >= 256                                                                 # the primaries reach the upper half of the bins
    # 3 * 304 and 3 * 131 + 7 are multiples of 16: base 0 with those strides took the 16-byte loads, everything else the byte loads
    assert (3 * 304) % 16 == 0 and (3 * 131 + 7) % 16 == 0


def test_histogram_kernel_on_rows_longer_than_a_work_unit(dev):
    """a work unit holds 2048 48-byte items of 16 rows: rows of 99 003 bytes are walked in two units, 19 rows in two bands"""
    params, t = StainMap.identity().params, sref.tables()
    r = dark_and_bright(21, 19, 33001)
    assert 2048 * 48 < 3 * r.shape[1] < 2 * 2048 * 48
    for shrink in (1, 2):
        want = sref.hist(r, shrink, 170, t)
        assert 0 < want[1024] < (19 // shrink) * (33001 // shrink)
        for base, pad in ((0, 5), (5, 7)):                        # 99 003 + 5 is a multiple of 16: the 16-byte loads
            hist = torch.zeros(1025, device=dev, dtype=torch.int64)
            device_hist(dev, params, r, shrink, 170, base, pad, hist)
            assert np.array_equal(hist.cpu().numpy(), want), (shrink, base, pad)


def test_histogram_kernel_refuses_bad_arguments(dev):
    L, params = _lib.lib(), StainMap.identity().params
    rd = torch.zeros(8, 8, 3, dtype=torch.uint8, device=dev)
    hist = torch.zeros(1025, dtype=torch.int64, device=dev)
    sp = _lib.stream_ptr()
    assert L.ay_stain_hist_u8(ptr(rd), 8, 8, 24, 1, 257, ptr(params), ptr(hist), sp) == -1
    assert L.ay_stain_hist_u8(ptr(rd), 8, 8, 23, 1, 220, ptr(params), ptr(hist), sp) == -1
    assert L.ay_stain_hist_u8(ptr(rd), 8, 8, 24, 3, 220, ptr(params), ptr(hist), sp) == -1
    assert L.ay_stain_hist_u8(ptr(rd), 8, 8, 24, 1, 220, None, ptr(hist), sp) == -1
    assert L.ay_stain_hist_u8(ptr(rd), 1, 8, 24, 2, 220, ptr(params), ptr(hist), sp) == 0      # no halved image: nothing to count
    assert int(hist.sum()) == 0


# ---- 2. wsi.stain_stats ---------------------------------------------------------------------------------------------------------------
def check_stats(got, want):
    assert got.hist.dtype == np.int64 and got.hist.shape == (2, 512) and got.basis == H_DAB
    assert np.array_equal(got.hist.ravel(), want[:1024]) and got.n_tissue == int(want[1024])
    for p in (99.0, 50.0, 100.0):
        assert got.strength(p) == sref.strength(want[:1024].reshape(2, 512), int(want[1024]), p)


def test_stain_stats_through_the_stream():
    t = sref.tables()
    slide = tr.test_slide(region_raster())
    want = sref.hist(slide, 1, 170, t)
    assert 0 < want[1024] < slide.shape[0] * slide.shape[1]
    check_stats(stain_stats(slide, bg_level=170, probe_stride=1), want)
    view = slide[::16, ::16]
    want16 = sref.hist(view, 1, 170, t)
    assert 0 < want16[1024] < want[1024]
    check_stats(stain_stats(slide, bg_level=170, probe_stride=16), want16)
    check_stats(stain_stats(slide, bg_level=170), want16)                              # 16 is the default probe
    # shrink 2: the exact rule takes the 2x2 means, the probe single source pixels; a tall raster: two strips accumulate
    r = dark_and_bright(9, 3301, 45)
    check_stats(stain_stats(r, shrink=2, bg_level=200, probe_stride=1), sref.hist(r, 2, 200, t))
    check_stats(stain_stats(r, shrink=2, bg_level=200, probe_stride=4), sref.hist(r[0:3300:8, 0:44:8], 1, 200, t))
    check_stats(stain_stats(r, bg_level=200, probe_stride=1), sref.hist(r, 1, 200, t))


# ---- 3. ay_ingest_region_tiles_stain_u8 -------------------------------------------------------------------------------------------------
CUT_TILE = 64
CUT_VIEWS = ((0,), (0, 3, 5), ALL_VIEWS)


def cut_origins(h, w):
    """on a grid; off the grid; negative; hanging over the right and bottom edges; past the region on every side"""
    grid = [(i * CUT_TILE, j * CUT_TILE) for j in range(-(-h // CUT_TILE)) for i in range(-(-w // CUT_TILE))]
    return grid + [(1, 2), (w // 3 + 1, h // 2 + 1), (-3, 2), (4, -5), (max(w - 5, 0), max(h - 3, 0)), (w, 0), (0, h), (-CUT_TILE, 3),
                   (2 ** 31 - 1, 0), (0, -2 ** 31)]


def stain_cut(dev, rd, H, W, shrink, origins, views, params, S_, offset_floats):
    """-> out [n * V,3,S,S] on the CPU; the output lies `offset_floats` floats behind a 16-byte boundary; rows behind n untouched"""
    o = torch.tensor(origins, dtype=torch.int32, device=dev).reshape(-1, 2)
    n, V = o.shape[0], len(views)
    total = n * V * 3 * S_ * S_
    buf = torch.full((offset_floats + total + GUARD + 3 * S_ * S_,), -7.0, device=dev)
    assert buf.data_ptr() % 16 == 0
    ids = (C.c_int * V)(*views)
    check(_lib.lib().ay_ingest_region_tiles_stain_u8(ptr(rd), H, W, W * 3, shrink, CUT_TILE, ptr(o), n, ids, V, ptr(params), S_,
                                                     ptr(buf[offset_floats:]), _lib.stream_ptr()), "ay_ingest_region_tiles_stain_u8")
    host = buf.cpu()
    assert (host[:offset_floats] == -7.0).all() and (host[offset_floats + total:] == -7.0).all()
    return host[offset_floats:offset_floats + total].reshape(n * V, 3, S_, S_)


def plain_cut(dev, rd, H, W, shrink, origins, views, S_):
    o = torch.tensor(origins, dtype=torch.int32, device=dev).reshape(-1, 2)
    n, V = o.shape[0], len(views)
    out = torch.empty(n * V, 3, S_, S_, device=dev)
    ids = (C.c_int * V)(*views)
    L = _lib.lib()
    if views == (0,):
        check(L.ay_ingest_region_tiles_list_u8(ptr(rd), H, W, W * 3, shrink, CUT_TILE, ptr(o), n, S_, ptr(out), _lib.stream_ptr()), "list")
    else:
        check(L.ay_ingest_region_tiles_views_u8(ptr(rd), H, W, W * 3, shrink, CUT_TILE, ptr(o), n, ids, V, S_, ptr(out), _lib.stream_ptr()), "views")
    return out.cpu()


@pytest.mark.parametrize("shrink", [1, 2])
@pytest.mark.parametrize("S_,offset", [(48, 0), (50, 1)], ids=["S48 vec4", "S50 scalar misaligned"])
def test_stain_cut_is_the_reference_cut_bit_for_bit(dev, S_, offset, shrink):
    H, W = 150 * shrink + 1, 170 * shrink + 1
    r = np.random.default_rng(H + S_).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    r[: H // 4] = np.minimum(r[: H // 4], 40)                    # a dark band: optical densities the gains push past the table's end
    rd = torch.from_numpy(r).to(dev)
    h, w = H // shrink, W // shrink
    origins = cut_origins(h, w)
    outside = [i for i, (x, y) in enumerate(origins) if x >= w or y >= h or x <= -CUT_TILE or y <= -CUT_TILE]
    assert len(outside) == 5
    before = {v: plain_cut(dev, rd, H, W, shrink, origins, v, S_) for v in CUT_VIEWS}
    for gains in GAINS:
        m = stain_map(gains)
        t = sref.tables(gains)
        assert bytes(m.params.cpu().numpy()) == b"".join(t[k].tobytes() for k in ("od", "D", "A", "T"))
        for views in CUT_VIEWS:
            V = len(views)
            want = sref.cut(r, shrink, CUT_TILE, origins, views, S_, t)
            got = stain_cut(dev, rd, H, W, shrink, origins, views, m.params, S_, offset)
            assert got.numpy().tobytes() == want.tobytes(), (gains, views)
            for i in outside:                                     # past the region: exactly 1.0
                assert (got[i * V:(i + 1) * V] == 1.0).all()
            if gains == (1.0, 1.0):                               # the identity map against the plain entry point
                err = (got.double() - before[views].double()).abs().max().item()
                print(f"identity map against the plain cut, views {views}: {err:.3e}")
                assert err <= BOUND
            else:
                assert (got.double() - before[views].double()).abs().max().item() > 0.05
    for v in CUT_VIEWS:                                           # the plain entry points after the stain calls: the same bytes
        assert plain_cut(dev, rd, H, W, shrink, origins, v, S_).numpy().tobytes() == before[v].numpy().tobytes()


def test_stain_cut_refuses_bad_arguments(dev):
    L, params, sp = _lib.lib(), StainMap.identity().params, _lib.stream_ptr()
    rd = torch.zeros(8, 8, 3, dtype=torch.uint8, device=dev)
    o = torch.zeros(1, 2, dtype=torch.int32, device=dev)
    out = torch.empty(8, 3, 8, 8, device=dev)
    ids = lambda *v: (C.c_int * len(v))(*v)
    call = lambda views, n_views, p=params, shrink=1, n=1: L.ay_ingest_region_tiles_stain_u8(ptr(rd), 8, 8, 24, shrink, 8, ptr(o), n, views, n_views,
                                                                                          None if p is None else ptr(p), 8, ptr(out), sp)
    assert call(ids(0), 1) == 0 and call(ids(0, 5), 2) == 0
    assert call(ids(0, 0), 2) == -1 and call(ids(8), 1) == -1 and call(ids(0), 0) == -1 and call(ids(0), 9) == -1
    assert call(ids(0), 1, p=None) == -1 and call(ids(0), 1, shrink=3) == -1 and call(ids(0), 1, n=0) == -1


# ---- 4. ay_stain_apply_u8, wsi.normalize_region -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_apply_kernel(dev, shrink):
    r = np.random.default_rng(shrink).integers(0, 256, size=(91, 123, 3), dtype=np.uint8)
    H, W = r.shape[0] // shrink, r.shape[1] // shrink
    for gains in GAINS:
        want = sref.apply(r, shrink, sref.tables(gains))
        if gains == (1.0, 1.0):
            assert np.array_equal(want, sref.image(r, shrink))      # the identity map returns the (halved) raster
        else:
            assert (want != sref.image(r, shrink)).mean() > 0.25
        for base, pad, opad in ((0, 0, 0), (5, 7, 0), (0, 3, 11)):
            buf, stride = placed(dev, r, base, pad)
            ostride = W * 3 + opad
            out = torch.full((H * ostride + GUARD,), 99, dtype=torch.uint8, device=dev)
            check(_lib.lib().ay_stain_apply_u8(ptr(buf), r.shape[0], r.shape[1], stride, shrink, ptr(stain_map(gains).params), ptr(out), ostride,
                                               _lib.stream_ptr()), "ay_stain_apply_u8")
            got = out.cpu().numpy()
            rows = np.lib.stride_tricks.as_strided(got, (H, ostride), (ostride, 1))
            assert np.array_equal(rows[:, :W * 3].reshape(H, W, 3), want), (gains, base, pad, opad)
            assert (rows[:, W * 3:] == 99).all() and (got[H * ostride:] == 99).all()       # row padding and what lies behind: untouched
    assert _lib.lib().ay_stain_apply_u8(ptr(buf), r.shape[0], r.shape[1], stride, shrink, ptr(stain_map(gains).params), ptr(out), W * 3 - 1,
                                        _lib.stream_ptr()) == -1


def test_normalize_region(dev):
    m = stain_map((1.3, 0.7))
    t = sref.tables((1.3, 0.7))
    for r, shrink in ((region_raster(), 1), (region_raster(), 2), (dark_and_bright(4, 3301, 45), 2), (dark_and_bright(5, 1700, 33), 1)):
        want = sref.apply(r, shrink, t)                              # the tall rasters: more than one strip
        got = normalize_region(r, m, shrink=shrink)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and np.array_equal(got, want)
        on_dev = normalize_region(r, m, shrink=shrink, device=True)
        assert on_dev.is_cuda and on_dev.dtype == torch.uint8 and np.array_equal(on_dev.cpu().numpy(), want)
        assert np.array_equal(normalize_region(r, StainMap.identity(), shrink=shrink), sref.image(r, shrink))


# ---- 5. RegionTileStream(stain=) and detect_region(stain=) ---------------------------------------------------------------------------------
DETECT_GAINS = (1.3, 0.7)


def grid_origins(raster, overlap):
    ty, tx, step = tile_grid(raster.shape[0], raster.shape[1], TILE, overlap)
    return [(i * step, j * step) for j in range(ty) for i in range(tx)], (ty, tx, step)


_tiles = {}


def reference_tiles(raster, overlap):
    """the stain cut of every tile of the grid by the reference, [n,3,S,S] on the CPU"""
    if overlap not in _tiles:
        origins, grid = grid_origins(raster, overlap)
        _tiles[overlap] = (torch.from_numpy(sref.cut(raster, 1, TILE, origins, (0,), S, sref.tables(DETECT_GAINS))), grid)
    return _tiles[overlap]


def in_views(tiles, views):
    """[n,3,S,S] -> [n * V,3,S,S], tile-major"""
    return torch.from_numpy(np.stack([vr.view_image_fast(tiles.numpy(), v) for v in views], 1).reshape(-1, *tiles.shape[1:]))


def expected_detections(m, dev, raster, overlap, views, mask):
    """model + NMS on the reference's tiles in the batches detect_region forms (the bf16 network's batches of 1 .. 8 images agree
    among themselves bit for bit: test_gpu_seam.per_tile_rows), rows to slide coordinates, then the seam rule -> {(ty, tx): rows}"""
    I0, (ty, tx, step) = reference_tiles(raster, overlap)
    V = len(views)
    per_call = BATCH if V == 1 else max(1, BATCH // V)
    assert per_call * V <= 8
    idx = np.arange(ty * tx) if mask is None else np.flatnonzero(mask.ravel())
    det = []
    for s0 in range(0, len(idx), per_call):
        tiles = I0[torch.from_numpy(idx[s0:s0 + per_call])]
        if V == 1:
            det += [None if d is None else d.cpu() for d in non_max_suppression(m(tiles), CONF, NMS)]
        else:
            pred = m.forward_device(in_views(tiles, views)).cpu().numpy()
            cat = vr.unview_rows(pred, views, S).reshape(tiles.shape[0], V * pred.shape[1], pred.shape[2])
            det += [None if d is None else d.cpu() for d in non_max_suppression(torch.from_numpy(cat).to(dev), CONF, NMS)]
    rows, tid = [], []
    for t, d in zip(idx, det):
        if d is not None:
            d = d.clone()
            d[:, :4] *= TILE / S
            d[:, [0, 2]] += (int(t) % tx) * step
            d[:, [1, 3]] += (int(t) // tx) * step
            rows.append(d)
            tid += [int(t)] * len(d)
    rows, tid = torch.cat(rows), np.asarray(tid, np.int32)
    keep = sr.seam_merge(rows.numpy(), tid, SEAM) if overlap else np.ones(len(tid), bool)
    return {(int(t) // tx, int(t) % tx): rows[torch.from_numpy(keep & (tid == t))] for t in np.unique(tid[keep])}


def test_stream_with_a_stain_map(dev):
    raster = region_raster()
    m = stain_map(DETECT_GAINS)
    for overlap in (0, OVERLAP):
        I0, (ty, tx, step) = reference_tiles(raster, overlap)
        mask = np.random.default_rng(3).random((ty, tx)) < 0.6
        assert 0 < mask.sum() < mask.size
        for views in ((0,), FLIPS):
            want = in_views(I0, views)
            V = len(views)
            for tile_mask in (None, mask):
                got, coords = [], []
                for tiles, cs in RegionTileStream(raster, TILE, S, 1, overlap=overlap, tile_mask=tile_mask, views=views, stain=m):
                    assert tiles.shape[0] == len(cs) * V
                    got.append(tiles.cpu())
                    coords += cs
                idx = np.arange(ty * tx) if tile_mask is None else np.flatnonzero(tile_mask.ravel())
                assert coords == [(int(k) // tx, int(k) % tx) for k in idx]
                sel = (torch.from_numpy(idx)[:, None] * V + torch.arange(V)[None]).reshape(-1)
                assert torch.cat(got).numpy().tobytes() == want[sel].numpy().tobytes(), (overlap, views, tile_mask is not None)
    # stain=None is the stream without the argument
    a = [(t.cpu(), cs) for t, cs in RegionTileStream(raster, TILE, S, 1)]
    b = [(t.cpu(), cs) for t, cs in RegionTileStream(raster, TILE, S, 1, stain=None)]
    assert len(a) == len(b) and all(x[1] == y[1] and x[0].numpy().tobytes() == y[0].numpy().tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("overlap,views,masked", [(0, (0,), False), (0, (0,), True), (OVERLAP, (0,), False), (OVERLAP, (0,), True),
                                                  (0, FLIPS, False), (OVERLAP, FLIPS, True)], ids=str)
def test_detect_region_with_a_stain_map(tmp_cfg_dir, dev, overlap, views, masked):
    model = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    ty, tx, _ = tile_grid(raster.shape[0], raster.shape[1], TILE, overlap)
    mask = (np.random.default_rng(3).random((ty, tx)) < 0.6) if masked else None
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, overlap=overlap, seam_thres=SEAM, views=views)
    expect = expected_detections(model, dev, raster, overlap, views, mask)
    assert sum(len(d) for d in expect.values()) >= 1
    res = detect_region(model, raster, tile_mask=mask, stain=stain_map(DETECT_GAINS), **kw)
    assert [(a, b) for a, b, _ in res] == sorted(expect)
    for a, b, d in res:
        assert torch.equal(d, expect[(a, b)]), (a, b)
    plain = detect_region(model, raster, tile_mask=mask, **kw)
    print(f"rows with the stain map {sum(len(d) for _, _, d in res)}, without {sum(len(d) for _, _, d in plain)}")
    assert len(plain) != len(res) or not all(x[:2] == y[:2] and x[2].shape == y[2].shape and torch.equal(x[2], y[2]) for x, y in zip(plain, res))
    none = detect_region(model, raster, tile_mask=mask, stain=None, **kw)     # stain=None: the call without the argument, bytes and order
    assert len(none) == len(plain) and all(x[:2] == y[:2] and x[2].numpy().tobytes() == y[2].numpy().tobytes() for x, y in zip(none, plain))


# ---- 6. quantify_region(stain_stats=, dab_thres=) ---------------------------------------------------------------------------------------
def test_quantify_region_reports_the_dab_positive_fraction(tmp_cfg_dir, dev):
    model = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    kw = dict(cell=32, field=3, top_k=4, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    base = quantify_region(model, raster, **kw)
    assert sorted(base) == sorted(["rows", "counts", "tissue", "fields", "n_found", "totals", "below", "flagged", "flags"])
    want = sref.hist(raster, 1, 220, sref.tables())
    stats = stain_stats(raster, probe_stride=1)
    check_stats(stats, want)
    frac, thres = sref.positive_fraction(want[:1024].reshape(2, 512), int(want[1024]), 1, 0.15)
    assert thres == 10 / 64 and 0.0 < frac < 1.0
    got = quantify_region(model, raster, stain_stats=stats, dab_thres=0.15, **kw)
    assert sorted(got) == sorted(list(base) + ["dab_positive_fraction", "dab_thres"])
    assert got["dab_positive_fraction"] == frac and got["dab_thres"] == thres
    assert torch.equal(got["rows"], base["rows"]) and np.array_equal(got["tissue"], base["tissue"])
    # with a stain map among the keyword arguments the detections are those of detect_region(stain=...)
    m = StainMap(stats, tuple(g * q for g, q in zip(DETECT_GAINS, stats.strength())))
    assert m.gains == pytest.approx(DETECT_GAINS)
    mapped = quantify_region(model, raster, stain_stats=stats, dab_thres=0.15, stain=m, **kw)
    rows = torch.cat([d for _, _, d in detect_region(model, raster, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, stain=m)])
    assert torch.equal(mapped["rows"], rows) and mapped["dab_positive_fraction"] == frac
