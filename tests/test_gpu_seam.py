"""Whole-slide detection with overlapping tiles (-m gpu): the strided tile ingest, ay_seam_append, ay_seam_merge and
wsi.detect_region(overlap > 0), every comparison exact (the seam rule only SELECTS rows).

Yardsticks: tiles cut on the CPU + oracle/ingest_oracle.ingest for the ingest; tests/seam_reference.py (the rule restated in NumPy
float32) for the merge; torch on the CPU for the append arithmetic; model + non_max_suppression on CPU-cut tiles, filtered by the
restatement, for the end-to-end path."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import seam_reference as sr
from amyloid_yolo_paper_amd import _lib, cfg_gen, parse_config, synth
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.models import Darknet
from amyloid_yolo_paper_amd.postprocess import seam_merge_device
from amyloid_yolo_paper_amd.wsi import RegionTileStream, detect_region, tile_grid
from oracle.ingest_oracle import ingest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


# ---- 1. strided ingest -----------------------------------------------------------------------------------------------------
def halve(r):
    h2, w2 = r.shape[0] // 2, r.shape[1] // 2
    q = r[: 2 * h2, : 2 * w2].astype(np.uint16)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def cpu_tiles(raster, tile, S, shrink, overlap):
    """overlapping tiles cut on the CPU: a 255-padded crop at (ty * step, tx * step), then the N1 chain of the oracle"""
    r = halve(raster) if shrink == 2 else raster
    ty, tx, step = tile_grid(r.shape[0], r.shape[1], tile, overlap)
    out = []
    for j in range(ty):
        for i in range(tx):
            t = np.full((tile, tile, 3), 255, np.uint8)
            c = r[j * step:j * step + tile, i * step:i * step + tile]
            t[: c.shape[0], : c.shape[1]] = c
            out.append(ingest(t, S))
    return torch.stack(out), (ty, tx, step)


INGEST_CASES = [  # H, W, tile, S, shrink, overlap
    (70, 100, 32, 32, 1, 8),       # ragged right and bottom edges
    (70, 100, 32, 24, 1, 12),      # with the nearest resize
    (133, 97, 32, 32, 2, 8),       # 2x2 halving, odd extents
    (64, 64, 16, 40, 2, 5),        # upsampling resize, odd step
    (50, 20, 32, 32, 1, 8),        # a raster narrower than one tile
    (90, 75, 32, 30, 1, 29),       # step 3: most of a tile is shared; out_size not a multiple of 4 (scalar stores)
    (70, 100, 32, 32, 1, 0),       # step == tile
    (133, 97, 32, 24, 2, 0),
]


@pytest.mark.parametrize("case", INGEST_CASES, ids=str)
def test_strided_ingest(dev, case):
    H, W, tile, S, shrink, overlap = case
    r = np.random.default_rng(H * 1000 + W + overlap).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    want, (ty, tx, step) = cpu_tiles(r, tile, S, shrink, overlap)
    L = _lib.lib()
    rd = torch.from_numpy(r).to(dev)
    out = torch.empty(ty * tx, 3, S, S, device=dev)
    check(L.ay_ingest_region_tiles_step_u8(ptr(rd), H, W, W * 3, shrink, tile, step, ty, tx, S, ptr(out), _lib.stream_ptr()), "step")
    assert torch.equal(out.cpu(), want)
    if overlap == 0:   # step == tile: the existing entry point, bit for bit
        old = torch.empty_like(out)
        check(L.ay_ingest_region_tiles_u8(ptr(rd), H, W, W * 3, shrink, tile, ty, tx, S, ptr(old), _lib.stream_ptr()), "region")
        assert torch.equal(out, old)
    got, coords = [], []
    stream = RegionTileStream(r, tile, S, shrink, overlap=overlap)
    assert (stream.tiles_y, stream.tiles_x, stream.step) == (ty, tx, step)
    for tiles, cs in stream:
        got.append(tiles.cpu())
        coords += cs
    assert coords == [(j, i) for j in range(ty) for i in range(tx)]
    assert torch.equal(torch.cat(got), want)


@pytest.mark.parametrize("case", INGEST_CASES, ids=str)
def test_stores_of_the_three_entries(dev, case):
    """The grid (step == tile), step and list entries share one cut: each writes the tiles exactly, into an output that starts on a
    16-byte boundary (16-byte stores where out_size % 4 == 0) and into one that starts one float behind it (scalar stores), and
    touches none of the 16 guard floats before and behind it."""
    H, W, tile, S, shrink, overlap = case
    r = np.random.default_rng(H * 1000 + W + overlap).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    want, (ty, tx, step) = cpu_tiles(r, tile, S, shrink, overlap)
    L, sp = _lib.lib(), _lib.stream_ptr()
    rd = torch.from_numpy(r).to(dev)
    org = torch.tensor([(i * step, j * step) for j in range(ty) for i in range(tx)], dtype=torch.int32, device=dev)
    entries = {"step": lambda o: L.ay_ingest_region_tiles_step_u8(ptr(rd), H, W, W * 3, shrink, tile, step, ty, tx, S, o, sp),
               "list": lambda o: L.ay_ingest_region_tiles_list_u8(ptr(rd), H, W, W * 3, shrink, tile, ptr(org), ty * tx, S, o, sp)}
    if overlap == 0:
        entries["grid"] = lambda o: L.ay_ingest_region_tiles_u8(ptr(rd), H, W, W * 3, shrink, tile, ty, tx, S, o, sp)
    n, G = want.numel(), 16
    for name, call in entries.items():
        for shift in (0, 1):
            buf = torch.full((G + shift + n + G,), -7.0, device=dev)
            assert buf.data_ptr() % 16 == 0
            check(call(ptr(buf[G + shift:])), name)
            got = buf.cpu()
            assert torch.equal(got[G + shift:G + shift + n].view_as(want), want), (name, shift)
            assert (got[:G + shift] == -7.0).all() and (got[G + shift + n:] == -7.0).all(), (name, shift)


# ---- 2. ay_seam_merge ------------------------------------------------------------------------------------------------------
def device_merge(dev, rows, tile_id, thres=0.5):
    rows = torch.from_numpy(np.ascontiguousarray(np.asarray(rows, np.float32).reshape(-1, 7))).to(dev)
    tid = torch.from_numpy(np.ascontiguousarray(np.asarray(tile_id, np.int32).reshape(-1))).to(dev)
    keep, (n_kept, rounds) = seam_merge_device(rows, tid, thres, return_stats=True)
    keep = keep.cpu().numpy()
    assert n_kept == int(keep.sum())
    return keep, rounds


def test_seam_merge_empty_and_single(dev):
    keep, _ = device_merge(dev, np.zeros((0, 7), np.float32), np.zeros(0, np.int32))
    assert keep.shape == (0,)
    keep, _ = device_merge(dev, [sr.row(3, 4, 30, 40, 0.5)], [7])
    assert keep.tolist() == [True]


@pytest.mark.parametrize("name", sorted(sr.hand_cases()))
def test_seam_merge_hand_cases(dev, name):
    rows, tile_id, thres, expect = sr.hand_cases()[name]
    assert sr.seam_merge(rows, tile_id, thres).tolist() == expect
    keep, _ = device_merge(dev, rows, tile_id, thres)
    assert keep.tolist() == expect


def test_seam_merge_corner_seen_by_four_tiles(dev):
    rows, tile_id = sr.corner_case()
    want = sr.seam_merge(rows, tile_id)
    assert want.tolist() == [True, False, False, False, True]
    keep, _ = device_merge(dev, rows, tile_id)
    assert np.array_equal(keep, want)


def test_seam_merge_staircase_chain(dev):
    """a dependency chain of 320 rows: kept, dropped, kept, ... -- the number of rounds must not be capped"""
    rows, tile_id = sr.staircase(320)
    want = sr.seam_merge(rows, tile_id)
    assert want.tolist() == [k % 2 == 0 for k in range(320)]
    keep, rounds = device_merge(dev, rows, tile_id)
    print("staircase(320): round launches", rounds)
    assert np.array_equal(keep, want)
    # the same chain listed backwards (the rank is by score, not by position) and shuffled
    for perm in (np.arange(320)[::-1], np.random.default_rng(5).permutation(320)):
        keep, _ = device_merge(dev, rows[perm], tile_id[perm])
        assert np.array_equal(keep, sr.seam_merge(rows[perm], tile_id[perm]))


def check_not_trivial(rows, tile_id, want, thres=0.5):
    """asserted on the RESTATEMENT's output, before the kernel is looked at"""
    dropped = 1.0 - want.mean()
    behind, ties = sr.kept_behind_dropped(rows, tile_id, want, thres), sr.score_ties(rows)
    print(f"rows {len(rows)}, dropped {dropped:.3f}, kept behind a dropped stronger partner {behind}, score ties {ties}")
    assert 0.2 <= dropped <= 0.7 and behind >= 100 and ties >= 100


def test_seam_merge_random_slide(dev):
    rows, tile_id = sr.synthetic_slide(3000, 6, 7, seed=1)
    want = sr.seam_merge(rows, tile_id)
    check_not_trivial(rows, tile_id, want)
    keep, rounds = device_merge(dev, rows, tile_id)
    print("round launches", rounds)
    assert np.array_equal(keep, want)
    keep2, _ = device_merge(dev, rows, tile_id)
    assert np.array_equal(keep, keep2)
    # rows in another order: the tie-break follows the index
    perm = np.random.default_rng(9).permutation(len(rows))
    keep, _ = device_merge(dev, rows[perm], tile_id[perm])
    assert np.array_equal(keep, sr.seam_merge(rows[perm], tile_id[perm]))
    # another threshold
    keep, _ = device_merge(dev, rows, tile_id, 0.8)
    assert np.array_equal(keep, sr.seam_merge(rows, tile_id, 0.8))


def test_seam_merge_boxes_as_large_as_a_tile(dev):
    """three tile-sized boxes among small ones: larger than a cell, they are tested against everything"""
    rows, tile_id = sr.synthetic_slide(3000, 6, 7, seed=3, big=3)
    side = np.maximum(rows[:, 2] - rows[:, 0], rows[:, 3] - rows[:, 1])
    assert (side > 180).sum() == 3 and np.median(side) < 48
    want = sr.seam_merge(rows, tile_id, 0.25)
    big = np.flatnonzero(side > 180)
    # not idle: the large boxes suppress small ones, or are suppressed
    without = sr.seam_merge(np.delete(rows, big, 0), np.delete(tile_id, big), 0.25)
    assert not np.array_equal(np.delete(want, big), without)
    keep, _ = device_merge(dev, rows, tile_id, 0.25)
    assert np.array_equal(keep, want)


def far_row_not_trivial(rows, want):
    rest = 1.0 - want[:-2].mean()
    print(f"far_row: rows {len(rows)}, far pair {want[-2:].tolist()}, dropped among the rest {rest:.3f}")
    return want[-2:].tolist() == [True, False] and 200 <= len(rows) < 2048 and 0.2 <= rest <= 0.7


def one_cell_not_trivial(rows, want):
    cx, cy = (rows[:, 0] + rows[:, 2]) * np.float32(0.5), (rows[:, 1] + rows[:, 3]) * np.float32(0.5)
    print(f"one_cell: rows {len(rows)}, kept {int(want.sum())}")
    return len(rows) >= 64 and (cx == cx[0]).all() and (cy == cy[0]).all() and 0.25 <= want.mean() <= 0.75


def borders_not_trivial(rows, want):
    w, h = rows[:, 2] - rows[:, 0] + 1, rows[:, 3] - rows[:, 1] + 1
    cx, cy = (rows[:, 0] + rows[:, 2]) * np.float32(0.5), (rows[:, 1] + rows[:, 3]) * np.float32(0.5)
    off = np.concatenate([cx - cx.min(), cy - cy.min()]) % 32                # 0, 0.5 or 31.5: on a multiple of 32 or half a pixel off
    print(f"borders: rows {len(rows)}, sides {int(min(w.min(), h.min()))} .. {int(max(w.max(), h.max()))}, offsets {np.unique(off).tolist()}")
    return (len(rows) >= 17 and min(w.min(), h.min()) >= 17 and max(w.max(), h.max()) <= 31 and (cx[0], cy[0]) == (cx.min(), cy.min())
            and set(np.unique(off).tolist()) == {0.0, 0.5, 31.5} and (want[0::2] != want[1::2]).all())


def every_row_oversize_not_trivial(rows, want):
    side = np.maximum(rows[:, 2] - rows[:, 0], rows[:, 3] - rows[:, 1])
    print(f"every_row_oversize: rows {len(rows)}, smallest side {side.min():.0f}, kept {int(want.sum())}")
    return len(rows) <= 16 and side.min() >= 100 and (~want).sum() >= 1 and want.sum() >= 2


GEOMETRY_NOT_TRIVIAL = {"far_row": far_row_not_trivial, "one_cell": one_cell_not_trivial, "borders": borders_not_trivial,
                        "every_row_oversize": every_row_oversize_not_trivial}


@pytest.mark.parametrize("name", sorted(GEOMETRY_NOT_TRIVIAL))
def test_seam_merge_geometry(dev, name):
    """extents and box sizes at which the centre grid (csrc/ay_box_grid.h) takes another path: a side doubled until the grid fits
    the cell cap, a 1 x 1 grid, centres on cell borders, an oversize list that holds every row"""
    rows, tile_id = sr.geometry_cases()[name]
    want = sr.seam_merge(rows, tile_id)
    assert GEOMETRY_NOT_TRIVIAL[name](rows, want)   # asserted on the RESTATEMENT's output, before the kernel is looked at
    keep, _ = device_merge(dev, rows, tile_id)
    assert np.array_equal(keep, want)
    perm = np.random.default_rng(11).permutation(len(rows))
    keep, _ = device_merge(dev, rows[perm], tile_id[perm])
    assert np.array_equal(keep, sr.seam_merge(rows[perm], tile_id[perm]))


def test_seam_merge_large_slide(dev):
    """a few 10^5 rows on a grid of 2 500 tiles against the binned restatement, which is first shown equal to the plain one"""
    rows, tile_id = sr.synthetic_slide(3000, 6, 7, seed=1)
    assert np.array_equal(sr.seam_merge_binned(rows, tile_id), sr.seam_merge(rows, tile_id))
    rows, tile_id = sr.synthetic_slide(120000, 50, 50, seed=2)
    assert len(rows) > 200000
    want = sr.seam_merge_binned(rows, tile_id)
    check_not_trivial(rows, tile_id, want)
    keep, rounds = device_merge(dev, rows, tile_id)
    print("round launches", rounds)
    assert np.array_equal(keep, want)


# ---- 3. ay_seam_append -----------------------------------------------------------------------------------------------------
GUARD = 64


def append_setup(dev, B, max_det, capacity, seed):
    rng = np.random.default_rng(seed)
    rows = torch.from_numpy(rng.uniform(0, 128, (B, max_det, 7)).astype(np.float32))
    slide_rows = torch.full((capacity + GUARD, 7), -7.0, device=dev)
    slide_tile = torch.full((capacity + GUARD,), -7, device=dev, dtype=torch.int32)
    slide_count = torch.zeros(2, device=dev, dtype=torch.int32)
    return rows, slide_rows, slide_tile, slide_count


def append(dev, rows, count, scale, origins, ids, slide_rows, slide_tile, slide_count, capacity):
    B, max_det, _ = rows.shape
    rows_d, count_d = rows.to(dev), torch.tensor(count, dtype=torch.int32, device=dev)
    origins_d, ids_d = torch.tensor(origins, dtype=torch.float32, device=dev), torch.tensor(ids, dtype=torch.int32, device=dev)
    check(_lib.lib().ay_seam_append(ptr(rows_d), ptr(count_d), B, max_det, C.c_float(scale), ptr(origins_d), ptr(ids_d), ptr(slide_rows),
                                    ptr(slide_tile), ptr(slide_count), capacity, _lib.stream_ptr()), "ay_seam_append")
    torch.cuda.synchronize()


def expected_append(rows, count, scale, origins, ids):
    out_r, out_t = [], []
    for b in range(rows.shape[0]):
        d = rows[b, :count[b]].clone()
        d[:, :4] *= scale                      # the arithmetic of detect_region's host path, in its order
        d[:, [0, 2]] += origins[b][0]
        d[:, [1, 3]] += origins[b][1]
        out_r.append(d)
        out_t += [ids[b]] * count[b]
    return torch.cat(out_r), torch.tensor(out_t, dtype=torch.int32)


def test_seam_append_moves_rows_to_slide_coordinates_in_order(dev):
    B, max_det, capacity = 5, 300, 2000
    rows, slide_rows, slide_tile, slide_count = append_setup(dev, B, max_det, capacity, 1)
    scale = 1536.0 / 1024.0
    want_r, want_t = [], []
    for call, count in enumerate([[3, 0, 300, 1, 257], [0, 0, 0, 0, 0], [64, 65, 0, 256, 2]]):   # three batches into one buffer
        origins = [[(call * B + b) * 1408, 7 * 1408] for b in range(B)]
        ids = [100 * call + b for b in range(B)]
        append(dev, rows, count, scale, origins, ids, slide_rows, slide_tile, slide_count, capacity)
        r, t = expected_append(rows, count, scale, origins, ids)
        want_r.append(r)
        want_t.append(t)
    want_r, want_t = torch.cat(want_r), torch.cat(want_t)
    n = want_r.shape[0]
    assert slide_count.cpu().tolist() == [n, 0]
    assert torch.equal(slide_rows[:n].cpu(), want_r) and torch.equal(slide_tile[:n].cpu(), want_t)
    assert (slide_rows[n:] == -7.0).all() and (slide_tile[n:] == -7).all()
    # a scale that is not a binary fraction (tile 192, network 128 is 1.5; 1000 / 768 is not): still two roundings
    rows, slide_rows, slide_tile, slide_count = append_setup(dev, B, max_det, capacity, 2)
    scale = 1000.0 / 768.0
    count, origins, ids = [7, 9, 0, 300, 11], [[936 * b, 936 * 3] for b in range(B)], list(range(B))
    append(dev, rows, count, scale, origins, ids, slide_rows, slide_tile, slide_count, capacity)
    r, t = expected_append(rows, count, scale, origins, ids)
    assert torch.equal(slide_rows[:len(r)].cpu(), r) and torch.equal(slide_tile[:len(r)].cpu(), t)


def test_seam_append_reports_overfull_tiles_and_a_full_buffer(dev):
    """bounds on valid inputs: what does not fit is not written, and the flag word says so"""
    B, max_det, capacity = 4, 64, 150
    rows, slide_rows, slide_tile, slide_count = append_setup(dev, B, max_det, capacity, 3)
    origins, ids = [[0, 0]] * B, [0, 1, 2, 3]
    # count[1] > max_det (ay_nms_sort_merge's "rows were dropped"): the first max_det rows are taken, flag 1
    append(dev, rows, [10, 70, 5, 0], 1.0, origins, ids, slide_rows, slide_tile, slide_count, capacity)
    assert slide_count.cpu().tolist() == [10 + 64 + 5, 1]
    r, t = expected_append(rows, [10, 64, 5, 0], 1.0, origins, ids)
    assert torch.equal(slide_rows[:79].cpu(), r) and torch.equal(slide_tile[:79].cpu(), t)
    assert (slide_rows[79:] == -7.0).all() and (slide_tile[79:] == -7).all()
    # 79 + 100 rows into a buffer of 150: rows up to the capacity are written, nothing behind it, flag 2 joins
    append(dev, rows, [60, 20, 20, 0], 1.0, origins, ids, slide_rows, slide_tile, slide_count, capacity)
    assert slide_count.cpu().tolist() == [capacity, 3]
    r2, t2 = expected_append(rows, [60, 20, 20, 0], 1.0, origins, ids)
    assert torch.equal(slide_rows[79:capacity].cpu(), r2[:capacity - 79]) and torch.equal(slide_tile[79:capacity].cpu(), t2[:capacity - 79])
    assert (slide_rows[capacity:] == -7.0).all() and (slide_tile[capacity:] == -7).all()
    # a full buffer takes nothing more
    append(dev, rows, [1, 1, 1, 1], 1.0, origins, ids, slide_rows, slide_tile, slide_count, capacity)
    assert slide_count.cpu().tolist() == [capacity, 3]
    assert (slide_rows[capacity:] == -7.0).all() and (slide_tile[capacity:] == -7).all()


# ---- 4. / 5. detect_region(overlap > 0) end to end ------------------------------------------------------------------------------
_models = {}


def build_model(C_, cfg_dir, dev, precision):
    key = (C_, precision)
    if key not in _models:
        cfg = cfg_gen.write_cfg(C_, cfg_dir)
        defs = parse_config.parse_model_config(cfg)
        params = synth.synth_params(defs, seed=7)
        wpath = os.path.join(cfg_dir, f"synth_c{C_}.weights")
        if not os.path.exists(wpath):
            synth.write_darknet_weights(wpath, defs, params, seen=12345)
        m = Darknet(cfg, precision=precision).to(dev).eval()
        m.load_darknet_weights(wpath)
        _models[key] = m
    return _models[key]


S, TILE, OVERLAP, CONF, NMS, SEAM, BATCH = 128, 192, 64, 0.5, 0.4, 0.5, 4


def region_raster():
    tiles = (gc.model_inputs(S, 6, 40) * 255).astype(np.uint8).transpose(0, 2, 3, 1)         # six synthetic tiles
    big = np.concatenate([np.concatenate(list(tiles[:3]), 1), np.concatenate(list(tiles[3:]), 1)], 0)
    return np.repeat(np.repeat(big, 2, 0), 2, 1)[: 2 * S + 77, : 3 * 2 * S - 50]              # 256-px content, ragged edges


def per_tile_rows(m, raster, overlap):
    """model + non_max_suppression on CPU-cut overlapping tiles, moved to slide coordinates: rows [M,7], tile_id [M], tiles_x, step.
    The bf16 network takes another kernel path for batches of 9 images and more, whose outputs differ in the last bits from those
    of smaller batches (batches of 1 .. 8 agree among themselves bit for bit): the tiles go through the model in the batches
    detect_region forms, so that the comparison stays exact."""
    from amyloid_yolo_paper_amd.utils import non_max_suppression
    want, (ty, tx, step) = cpu_tiles(raster, TILE, S, 1, overlap)
    det = []
    for j in range(ty):                                    # the batches of detect_region(batch_size=BATCH): a strip at a time
        for s0 in range(0, tx, BATCH):
            det += list(non_max_suppression(m(want[j * tx + s0:j * tx + min(s0 + BATCH, tx)]), CONF, NMS))
    rows, tid = [], []
    for t, d in enumerate(det):
        if d is not None:
            d = d.clone()
            d[:, :4] *= TILE / S
            d[:, [0, 2]] += (t % tx) * step
            d[:, [1, 3]] += (t // tx) * step
            rows.append(d)
            tid += [t] * len(d)
    return torch.cat(rows), np.asarray(tid, np.int32), tx, step


def in_overlap_band(rows, tx, step, tid):
    """rows whose box lies entirely inside the band its tile shares with the next tile to the right or below"""
    r = rows.numpy()
    ox, oy = (tid % tx) * step, (tid // tx) * step
    return ((r[:, 0] >= ox + step) & (r[:, 2] < ox + TILE)) | ((r[:, 1] >= oy + step) & (r[:, 3] < oy + TILE))


def test_detect_region_with_overlap_equals_per_tile_detection_plus_seam_rule(tmp_cfg_dir, dev):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    rows, tid, tx, step = per_tile_rows(m, raster, OVERLAP)
    keep = sr.seam_merge(rows.numpy(), tid, SEAM)
    band = in_overlap_band(rows, tx, step, tid)
    print(f"rows {len(rows)}, dropped {int((~keep).sum())}, kept in an overlap band {int((keep & band).sum())}")
    assert (~keep).sum() >= 1 and (keep & band).sum() >= 1
    res = detect_region(m, raster, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, overlap=OVERLAP, seam_thres=SEAM)
    expect = {}
    for t in np.unique(tid[keep]):
        expect[(int(t) // tx, int(t) % tx)] = rows[torch.from_numpy(keep & (tid == t))]
    assert [(a, b_) for a, b_, _ in res] == sorted(expect)          # tiles in grid order, none empty
    for a, b_, d in res:
        assert torch.equal(d, expect[(a, b_)])


def test_detect_region_without_overlap_is_the_present_path(tmp_cfg_dir, dev):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    a = detect_region(m, raster, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    b = detect_region(m, raster, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, overlap=0)
    assert len(a) == len(b) > 0
    for (ty, tx, d), (ty2, tx2, d2) in zip(a, b):
        assert (ty, tx) == (ty2, tx2) and torch.equal(d, d2)


def test_detect_region_with_overlap_properties(tmp_cfg_dir, dev):
    """independent of the restatement's greedy walk: no two kept rows of one class from different tiles overlap beyond the
    threshold; every dropped row has a kept stronger partner; the same call twice gives identical bytes"""
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, overlap=OVERLAP, seam_thres=SEAM)
    res = detect_region(m, raster, **kw)
    again = detect_region(m, raster, **kw)
    assert len(res) == len(again) and all(x[:2] == y[:2] and x[2].numpy().tobytes() == y[2].numpy().tobytes() for x, y in zip(res, again))
    tx = tile_grid(raster.shape[0], raster.shape[1], TILE, OVERLAP)[1]
    kept = np.concatenate([d.numpy() for _, _, d in res])
    kept_tile = np.concatenate([[a * tx + b_] * len(d) for a, b_, d in res])
    thres = np.float32(SEAM)
    for i in range(len(kept)):
        other = (kept[:, 6] == kept[i, 6]) & (kept_tile != kept_tile[i])
        assert not (sr.ov(kept[i, :4], kept[other, :4]) > thres).any()
    rows, tid, _, _ = per_tile_rows(m, raster, OVERLAP)
    rows = rows.numpy()
    kept_set = {r.tobytes() + bytes([t]) for r, t in zip(kept, kept_tile)}
    score, kscore = sr.scores(rows), sr.scores(kept)
    n_dropped = 0
    for i in range(len(rows)):
        if rows[i].tobytes() + bytes([tid[i]]) in kept_set:
            continue
        n_dropped += 1
        stronger = (kept[:, 6] == rows[i, 6]) & (kept_tile != tid[i]) & (kscore >= score[i])
        assert (sr.ov(rows[i, :4], kept[stronger, :4]) > thres).any()
    assert n_dropped >= 1 and len(kept) + n_dropped == len(rows)


def test_detect_region_reports_a_tile_beyond_max_det(tmp_cfg_dir, dev):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    with pytest.raises(_lib.AyError):
        detect_region(m, region_raster(), tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, overlap=OVERLAP, max_det=1)
