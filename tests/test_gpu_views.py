"""Dihedral test-time views (-m gpu): ay_ingest_region_tiles_views_u8, ay_unview_rows, ay_view_votes, ay_view_select,
RegionTileStream(views=...), views.nms_views_device and wsi.detect_region(views=..., min_views=...).  Every comparison is exact:
a view is a permutation of the tile's bits, the box mapping is one fp32 operation per value, the votes are integers and the
selection only drops rows.

Yardsticks: tiles cut on the CPU (test_gpu_seam.cpu_tiles) followed by torch.flip / transpose for the ingest; tests/views_reference.py
(the two rules restated in NumPy, the IoU from oracle.boxes_oracle.bbox_iou) for the boxes, the votes and the selection; for the
end-to-end path CPU-cut, CPU-flipped tiles through model.forward_device, the NumPy unview, the concatenation, the existing
non_max_suppression, the restated votes and, with overlap, tests/seam_reference.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import seam_reference as sr
import views_reference as vr
from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.utils import non_max_suppression
from amyloid_yolo_paper_amd.views import (ALL_VIEWS, FLIPS, nms_views_device, unview_rows_device, view_select_device,
                                          view_votes_device)
from amyloid_yolo_paper_amd.wsi import RegionTileStream, detect_region, tile_grid
from oracle.ingest_oracle import ingest
from test_gpu_seam import BATCH, CONF, INGEST_CASES, NMS, OVERLAP, S, SEAM, TILE, build_model, cpu_tiles, halve, region_raster

pytestmark = pytest.mark.gpu

GUARD = 64
VIEW_LISTS = (ALL_VIEWS, (6, 0, 3), (0,))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def view_t(I0, v):
    """torch yardstick of the pixel rule: flip along x and / or y, then transpose"""
    FX, FY, T = vr.bits(v)
    x = I0
    if FX:
        x = torch.flip(x, [-1])
    if FY:
        x = torch.flip(x, [-2])
    if T:
        x = x.transpose(-1, -2)
    return x.contiguous()


def in_views(tiles, views):
    """[n,3,S,S] -> [n * V,3,S,S], tile-major"""
    return torch.stack([view_t(tiles, v) for v in views], 1).reshape(-1, *tiles.shape[1:])


# ---- 1. the views ingest -------------------------------------------------------------------------------------------------------
# the kernel holds 32 x 32 blocks of I0: sizes above one block and no multiple of it, in both store forms, and an odd size
VIEW_CASES = INGEST_CASES + [
    (230, 200, 96, 100, 1, 16),    # 16-byte stores, blocks of 32, 32, 32, 4
    (230, 200, 96, 70, 1, 16),     # scalar stores, blocks of 32, 32, 6
    (230, 200, 96, 33, 1, 16),     # odd size: a block of one row / one column
    (233, 201, 48, 68, 2, 8),      # 2x2 halving, upsampling, blocks of 32, 32, 4
]


def cpu_crops(rr, tile, origins, S_):
    out = []
    for x, y in origins:
        t = np.full((tile, tile, 3), 255, np.uint8)
        c = rr[max(y, 0):max(y + tile, 0), max(x, 0):max(x + tile, 0)]
        t[max(-y, 0):max(-y, 0) + c.shape[0], max(-x, 0):max(-x, 0) + c.shape[1]] = c
        out.append(ingest(t, S_))
    return torch.stack(out)


def views_ingest(dev, rd, H, W, shrink, tile, origins, views, S_, offset_floats=0):
    """-> (out [n * V,3,S,S] on the CPU); the output lies `offset_floats` floats behind a 16-byte boundary; guards checked"""
    o = torch.tensor(origins, dtype=torch.int32, device=dev).reshape(-1, 2)
    n, V = o.shape[0], len(views)
    total = n * V * 3 * S_ * S_
    buf = torch.full((offset_floats + total + GUARD,), -7.0, device=dev)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset_floats:]
    ids = (C.c_int * V)(*views)
    check(_lib.lib().ay_ingest_region_tiles_views_u8(ptr(rd), H, W, W * 3, shrink, tile, ptr(o), n, ids, V, S_, ptr(out), _lib.stream_ptr()),
          "ay_ingest_region_tiles_views_u8")
    host = buf.cpu()
    assert (host[:offset_floats] == -7.0).all() and (host[offset_floats + total:] == -7.0).all()    # nothing before, nothing behind
    return host[offset_floats:offset_floats + total].reshape(n * V, 3, S_, S_)


@pytest.mark.parametrize("case", VIEW_CASES, ids=str)
def test_views_ingest(dev, case):
    H, W, tile, S_, shrink, overlap = case
    r = np.random.default_rng(H * 1000 + W + overlap).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    rd = torch.from_numpy(r).to(dev)
    rr = halve(r) if shrink == 2 else r
    h, w = rr.shape[:2]
    ty, tx, step = tile_grid(h, w, tile, overlap)
    grid_o = [(i * step, j * step) for j in range(ty) for i in range(tx)]
    # the grid, an origin on no grid, one that hangs over the right and bottom edges, origins left of and above the region
    origins = grid_o + [(1, 2), (max(w - 5, 0), max(h - 3, 0)), (-3, 2), (4, -5), (-tile + 1, -tile + 2)]
    I0 = cpu_crops(rr, tile, origins, S_)
    assert torch.equal(I0[:len(grid_o)], cpu_tiles(r, tile, S_, shrink, overlap)[0])
    assert not (I0[-3] == 1.0).all()                                 # (-3, 2) is not all background
    for views in VIEW_LISTS:
        want = in_views(I0, views)
        for offset in (0, 1):         # 1: the base is 4 bytes off a 16-byte boundary, the scalar form
            got = views_ingest(dev, rd, H, W, shrink, tile, origins, views, S_, offset)
            assert torch.equal(got, want), (views, offset)
    # views = (0,) is the list entry, bit for bit
    o = torch.tensor(origins, dtype=torch.int32, device=dev)
    old = torch.empty(len(origins), 3, S_, S_, device=dev)
    check(_lib.lib().ay_ingest_region_tiles_list_u8(ptr(rd), H, W, W * 3, shrink, tile, ptr(o), len(origins), S_, ptr(old), _lib.stream_ptr()),
          "ay_ingest_region_tiles_list_u8")
    assert torch.equal(old.cpu(), views_ingest(dev, rd, H, W, shrink, tile, origins, (0,), S_))


@pytest.mark.parametrize("case", VIEW_CASES, ids=str)
def test_stream_with_views(dev, case):
    """RegionTileStream(views=...) yields the tiles of the plain stream in every view, tile-major, with the same coordinates"""
    H, W, tile, S_, shrink, overlap = case
    r = np.random.default_rng(H * 1000 + W + overlap).integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    I0, (ty, tx, step) = cpu_tiles(r, tile, S_, shrink, overlap)
    mask = np.random.default_rng(H + overlap).random((ty, tx)) < 0.5
    mask[0, 0], mask[-1, -1] = True, False if ty * tx > 1 else True
    for views, m in ((ALL_VIEWS, None), ((6, 0, 3), None), (ALL_VIEWS, mask), ((6, 0, 3), mask), ((5,), mask)):
        got, coords = [], []
        for tiles, cs in RegionTileStream(r, tile, S_, shrink, overlap=overlap, tile_mask=m, views=views):
            assert tiles.shape[0] == len(cs) * len(views)
            got.append(tiles.cpu())
            coords += cs
        idx = np.arange(ty * tx) if m is None else np.flatnonzero(m.ravel())
        assert coords == [(int(k) // tx, int(k) % tx) for k in idx]
        assert torch.equal(torch.cat(got), in_views(I0[torch.from_numpy(idx)], views))
    # the batches detect_region takes: 2 tiles x V images, filled across strips
    stream = RegionTileStream(r, tile, S_, shrink, overlap=overlap, tile_mask=mask, views=(6, 0, 3))
    got, firsts = [], []
    for tiles, w0 in stream._batches(2):
        assert tiles.shape[0] in (3, 6)
        got.append(tiles.cpu())
        firsts.append(w0)
    idx = np.flatnonzero(mask.ravel())
    assert firsts == list(range(0, len(idx), 2))
    assert torch.equal(torch.cat(got), in_views(I0[torch.from_numpy(idx)], (6, 0, 3)))


# ---- 2. ay_unview_rows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S_", [416, 33])
@pytest.mark.parametrize("C_", [1, 2])
def test_unview_rows(dev, C_, S_):
    B, N, K = 3, 50, 5 + C_
    for views in VIEW_LISTS + ((5,),):
        V = len(views)
        rng = np.random.default_rng(S_ + C_ + V)
        pred = rng.uniform(-0.25 * S_, 1.25 * S_, (B * V, N, K)).astype(np.float32)
        pred[..., 4:] = rng.random((B * V, N, K - 4), dtype=np.float32)
        want = vr.unview_rows(pred, views, S_)
        buf = torch.full((pred.size + GUARD,), -7.0, device=dev)
        t = buf[:pred.size].view(B * V, N, K)
        t.copy_(torch.from_numpy(pred))
        assert unview_rows_device(t, views, S_) is t
        host = buf.cpu().numpy()
        got = host[:pred.size].reshape(pred.shape)
        assert got.tobytes() == want.tobytes()
        assert np.array_equal(got[..., 4:], pred[..., 4:]) and (host[pred.size:] == -7.0).all()
        if any(v & 3 for v in views):
            assert not np.array_equal(got[..., :2], pred[..., :2])      # not idle


# ---- 3. votes and selection ----------------------------------------------------------------------------------------------------
def device_votes_and_select(dev, pred, V, conf, vthres, rows, count, min_views):
    """-> votes [B, max_det] and, per keep_idx form, the selection (rows, keep, count) as NumPy; two runs, the same bytes"""
    B, max_det, _ = rows.shape
    pred_d, rows_d = torch.from_numpy(pred).to(dev), torch.from_numpy(rows).to(dev)
    count_d = torch.tensor(count, dtype=torch.int32, device=dev)
    vbuf = torch.full((B * max_det + GUARD,), -3, device=dev, dtype=torch.int32)       # the call zeroes what it writes
    votes = vbuf[:B * max_det].view(B, max_det)
    out = []
    for _ in range(2):
        votes.fill_(-3)
        assert view_votes_device(pred_d, V, conf, vthres, rows_d, count_d, votes=votes) is votes
        out.append(vbuf.cpu().numpy())
    assert out[0].tobytes() == out[1].tobytes() and (out[0][B * max_det:] == -3).all()
    assert torch.equal(pred_d.cpu(), torch.from_numpy(pred)) and torch.equal(rows_d.cpu(), torch.from_numpy(rows))   # read only
    keep = np.arange(B * max_det, dtype=np.int32).reshape(B, max_det) * 3 + 1
    sel = {}
    for with_keep in (True, False):
        rbuf = torch.full((B * max_det * 7 + GUARD,), -7.0, device=dev)
        r = rbuf[:B * max_det * 7].view(B, max_det, 7)
        r.copy_(rows_d)
        k = torch.from_numpy(keep).to(dev) if with_keep else None
        c = count_d.clone()
        view_select_device(r, k, c, votes, min_views)
        assert (rbuf[B * max_det * 7:] == -7.0).all()
        sel[with_keep] = (r.cpu().numpy(), None if k is None else k.cpu().numpy(), c.cpu().numpy())
    return out[0][:B * max_det].reshape(B, max_det), keep, sel


def check_selection(rows, keep, count, votes, min_views, sel):
    want_r, want_k, want_c = vr.view_select(rows, keep, count, votes, min_views)
    max_det = rows.shape[1]
    for with_keep, (r, k, c) in sel.items():
        assert np.array_equal(c, want_c)
        for b in range(rows.shape[0]):
            D = min(int(count[b]), max_det)
            n = int((vr.popcount(votes[b, :D]) >= min_views).sum())       # the rows in front are the contract
            assert n == want_c[b] or count[b] > max_det
            assert r[b, :n].tobytes() == want_r[b, :n].tobytes()
            if with_keep:
                assert np.array_equal(k[b, :n], want_k[b, :n])


def box_row(box, conf, cls, C_=2):
    scores = [0.1] * C_
    scores[cls] = 0.8
    return list(box) + [conf] + scores


def test_votes_and_select_hand_cases(dev):
    V, N, C_, max_det = 8, 12, 2, 16
    conf = np.float32(0.6)
    below = np.nextafter(conf, np.float32(0))
    far = [900.0, 900.0, 910.0, 910.0]
    pred = np.zeros((3, V * N, 5 + C_), np.float32)
    pred[:] = box_row(far, 0.9, 0)
    rows = np.zeros((3, max_det, 7), np.float32)
    # image 0: detection k - 1 (class 1, at x = 40 k) is seen by exactly the views 0 .. k-1
    for k in range(1, 9):
        box = [40.0 * k, 10.0, 40.0 * k + 9, 19.0]
        rows[0, k - 1] = box + [0.9, 0.8, 1]
        for j in range(k):
            pred[0, j * N + (k - 1)] = box_row(box, 0.7, 1)
    # detection 8: a row of the wrong class (view 0), a row one ulp below conf_thres (view 1), a row exactly on it (view 2)
    box = [500.0, 10.0, 509.0, 19.0]
    rows[0, 8] = box + [0.9, 0.8, 0]
    pred[0, 0 * N + 9] = box_row(box, 0.9, 1)
    pred[0, 1 * N + 9] = box_row(box, below, 0)
    pred[0, 2 * N + 9] = box_row(box, conf, 0)
    # detection 9: 10 x 10 pixels (+1 rule); 10 x 5 inside it has IoU 50 / 100 = 0.5 exactly (view 3), 10 x 6 has 0.6 (view 4)
    box = [600.0, 10.0, 609.0, 19.0]
    rows[0, 9] = box + [0.9, 0.8, 0]
    pred[0, 3 * N + 10] = box_row([600.0, 10.0, 609.0, 14.0], 0.9, 0)
    pred[0, 4 * N + 10] = box_row([600.0, 10.0, 609.0, 15.0], 0.9, 0)
    assert float(vr.bbox_iou(np.float32([box]), np.float32([[600, 10, 609, 14]]))[0]) == 0.5
    # detection 10 sits behind count: identical to detection 7, which every view sees
    rows[0, 10] = rows[0, 7]
    # image 1: empty.  image 2: count > max_det; every row is seen by view 5, rows 0, 3, 6 ... also by view 2
    for d in range(max_det):
        box = [30.0 * d, 50.0, 30.0 * d + 9, 59.0]
        rows[2, d] = box + [0.9, 0.8, 1]
    for d in range(N):
        pred[2, 5 * N + d] = box_row(rows[2, d, :4], 0.9, 1)
        if d % 3 == 0:
            pred[2, 2 * N + d] = box_row(rows[2, d, :4], 0.9, 1)
    count = [10, 0, max_det + 5]
    for vthres, nine in ((np.float32(0.5), 0b10000), (np.nextafter(np.float32(0.5), np.float32(0)), 0b11000)):
        want = vr.view_votes(pred, V, conf, vthres, rows, count)
        assert want[0, :11].tolist() == [(1 << k) - 1 for k in range(1, 9)] + [0b100, nine, 0]          # on the restatement first
        assert not want[1].any() and want[2, :N].tolist() == [0b100100 if d % 3 == 0 else 0b100000 for d in range(N)]
        assert not want[2, N:].any()
        for min_views in (1, 2, 5, 8):
            votes, keep, sel = device_votes_and_select(dev, pred, V, conf, vthres, rows, count, min_views)
            assert np.array_equal(votes, want)
            check_selection(rows, keep, count, want, min_views, sel)
            for _, _, c in sel.values():
                assert c[1] == 0 and c[2] == max_det + 5                 # the overfull image keeps its count
            if min_views == 5:
                assert sel[True][2][0] == 4 and sel[True][1][0, :4].tolist() == [3 * d + 1 for d in (4, 5, 6, 7)]   # stable


def random_vote_case(seed, B=4, V=8, N=300, C_=2, max_det=32, S_=416.0):
    rng = np.random.default_rng(seed)
    pred = np.zeros((B, V * N, 5 + C_), np.float32)
    xy = rng.uniform(0, S_, (B, V * N, 2))
    wh = rng.uniform(4, 60, (B, V * N, 2))
    pred[..., 0:2], pred[..., 2:4] = xy, xy + wh
    pred[..., 4] = rng.uniform(0.0, 0.45, (B, V * N))                  # background rows: below the threshold
    pred[..., 5:] = rng.random((B, V * N, C_))
    rows = np.zeros((B, max_det, 7), np.float32)
    count = []
    for b in range(B):
        M = int(rng.integers(7, 11))
        count.append(M)
        for d in range(M):
            x, y = rng.uniform(20, S_ - 80, 2)
            w, h = rng.uniform(15, 50, 2)
            cls = int(rng.integers(0, C_))
            rows[b, d] = [x, y, x + w, y + h, 0.9, 0.8, cls]
            for j in range(V):
                if rng.random() < 0.6:                                  # view j has a sighting, shifted by up to a third of the box
                    r = j * N + int(rng.integers(0, N))
                    dx, dy = rng.uniform(-0.33, 0.33, 2) * (w, h)
                    scores = rng.uniform(0.0, 0.4, C_)
                    scores[cls if rng.random() < 0.9 else (cls + 1) % C_] = 0.9
                    pred[b, r] = [x + dx, y + dy, x + w + dx, y + h + dy, rng.uniform(0.5, 1.0)] + list(scores)
    return pred, rows, count


@pytest.mark.parametrize("seed", [1, 2])
def test_votes_and_select_random_batches(dev, seed):
    pred, rows, count = random_vote_case(seed)
    V, conf, vthres = 8, 0.5, 0.4
    cands = (pred[..., 4] >= np.float32(conf)).sum(1)
    want = vr.view_votes(pred, V, conf, vthres, rows, count)
    pc = np.concatenate([vr.popcount(want[b, :count[b]]) for b in range(len(count))])
    print("candidates per image", cands.tolist(), "vote histogram", np.bincount(pc, minlength=9).tolist())
    assert 20 <= cands.min() and cands.max() <= 70 and len(np.unique(pc)) >= 5 and (pc >= 3).any() and (pc < 3).any()
    for min_views in (1, 3):
        votes, keep, sel = device_votes_and_select(dev, pred, V, conf, vthres, rows, count, min_views)
        assert np.array_equal(votes, want)
        check_selection(rows, keep, count, want, min_views, sel)
    assert 0 < sel[True][2].sum() < sum(count)                          # min_views 3 dropped rows and kept rows


# ---- 4. detect_region(views=...) end to end ---------------------------------------------------------------------------------------
_refs = {}


def reference_rows(m, raster, overlap, views):
    """per tile of the full grid: (rows [n,7] in tile coordinates as non_max_suppression emits them | None, votes of each row).
    The tiles go through the model one call per `max(1, BATCH // V)` tiles, as detect_region forms them; the bf16 network's batches
    of 1 .. 8 images agree among themselves bit for bit (test_gpu_seam.per_tile_rows), so the masked runs, which fill their batches
    with other tiles, share this reference."""
    key = (overlap, views)
    if key in _refs:
        return _refs[key]
    I0, (ty, tx, step) = cpu_tiles(raster, TILE, S, 1, overlap)
    V = len(views)
    per_call = max(1, BATCH // V)
    assert per_call * V <= 8
    out = []
    for j in range(ty):
        for s0 in range(0, tx, per_call):
            tiles = I0[j * tx + s0:j * tx + min(s0 + per_call, tx)]
            pred = m.forward_device(in_views(tiles, views)).cpu().numpy()
            cat = vr.unview_rows(pred, views, S).reshape(tiles.shape[0], V * pred.shape[1], pred.shape[2])
            t = torch.from_numpy(cat).to(m_device(m))
            det = non_max_suppression(t, CONF, NMS)            # corners in place in t
            corners = t.cpu().numpy()
            for b, d in enumerate(det):
                if d is None:
                    out.append((None, None))
                    continue
                d = d.cpu()
                votes = vr.view_votes(corners[b:b + 1], V, CONF, NMS, d.numpy()[None], [len(d)])[0]
                out.append((d, vr.popcount(votes)))
    _refs[key] = (out, ty, tx, step)
    return _refs[key]


def m_device(m):
    return next(m.parameters()).device


def expected_result(ref, mask, overlap, min_views):
    out, ty, tx, step = ref
    rows, tid = [], []
    for t, (d, pc) in enumerate(out):
        if d is None or (mask is not None and not mask.ravel()[t]):
            continue
        d = d[torch.from_numpy(pc >= min_views)].clone()
        if len(d) == 0:
            continue
        d[:, :4] *= TILE / S
        d[:, [0, 2]] += (t % tx) * step
        d[:, [1, 3]] += (t // tx) * step
        rows.append(d)
        tid += [t] * len(d)
    rows, tid = torch.cat(rows), np.asarray(tid, np.int32)
    keep = sr.seam_merge(rows.numpy(), tid, SEAM) if overlap else np.ones(len(tid), bool)
    return {(int(t) // tx, int(t) % tx): rows[torch.from_numpy(keep & (tid == t))] for t in np.unique(tid[keep])}, int((~keep).sum())


@pytest.mark.parametrize("overlap", [0, OVERLAP])
@pytest.mark.parametrize("views", [ALL_VIEWS, FLIPS, (5,)], ids=str)
def test_detect_region_with_views(tmp_cfg_dir, dev, views, overlap):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    ref = reference_rows(m, raster, overlap, views)
    out, ty, tx, _ = ref
    V = len(views)
    pc = np.concatenate([p for d, p in out if d is not None])
    print(f"views {views}, overlap {overlap}: rows {len(pc)}, vote histogram {np.bincount(pc, minlength=V + 1).tolist()}")
    choices = [1]
    if V > 1:     # from the reference's own histogram: the rows with the fewest votes go, the others stay
        assert pc.min() < pc.max(), "every row has the same number of votes: no min_views separates them"
        choices.append(int(np.unique(pc)[1]))
        assert 1 < choices[1] <= V
    mask = np.random.default_rng(3).random((ty, tx)) < 0.6
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH, overlap=overlap, seam_thres=SEAM, views=views)
    for min_views in choices:
        for tile_mask in (None, mask):
            expect, seam_dropped = expected_result(ref, tile_mask, overlap, min_views)
            n_all = sum(len(d) for t, (d, _) in enumerate(out) if d is not None and (tile_mask is None or tile_mask.ravel()[t]))
            n_exp = sum(len(d) for d in expect.values())
            assert n_exp >= 1
            if min_views > 1 and tile_mask is None:
                assert n_exp + seam_dropped < n_all                   # the votes dropped a row
            if overlap and tile_mask is None and min_views == 1:
                assert seam_dropped >= 1
            res = detect_region(m, raster, tile_mask=tile_mask, min_views=min_views, **kw)
            assert [(a, b_) for a, b_, _ in res] == sorted(expect)
            for a, b_, d in res:
                assert torch.equal(d, expect[(a, b_)]), (min_views, tile_mask is not None, a, b_)


def test_views_change_the_result_and_a_tile_beyond_max_det_is_reported(tmp_cfg_dir, dev):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    plain = detect_region(m, raster, **kw)
    tta = detect_region(m, raster, views=ALL_VIEWS, **kw)
    assert sum(len(d) for _, _, d in tta) != sum(len(d) for _, _, d in plain) or not all(torch.equal(x[2], y[2]) for x, y in zip(plain, tta))
    for overlap in (0, OVERLAP):
        with pytest.raises(_lib.AyError):
            detect_region(m, raster, views=FLIPS, overlap=overlap, max_det=1, **kw)


def test_defaults_are_the_path_without_views(tmp_cfg_dir, dev, monkeypatch):
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    kw = dict(tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    calls = []
    monkeypatch.setattr(wsi.detect, "nms_views_device", lambda *a, **k: calls.append(1) or nms_views_device(*a, **k))
    for extra in (dict(), dict(overlap=OVERLAP, seam_thres=SEAM)):
        a = detect_region(m, raster, **kw, **extra)                 # never passes the new arguments
        b = detect_region(m, raster, views=(0,), min_views=1, vote_thres=None, **kw, **extra)
        assert len(a) == len(b) > 0 and all(x[:2] == y[:2] and x[2].numpy().tobytes() == y[2].numpy().tobytes() for x, y in zip(a, b))
        assert calls == []                                           # nothing new is called
        c = detect_region(m, raster, views=[0], min_views=1, vote_thres=0.3, **kw, **extra)
        assert calls == [] and all(torch.equal(x[2], y[2]) for x, y in zip(a, c))
    detect_region(m, raster, views=(0, 1), **kw)
    assert calls


# ---- 5. HIP graph ----------------------------------------------------------------------------------------------------------------
def test_hip_graph_of_a_step_with_views_replays_after_eager_steps(tmp_cfg_dir, dev):
    """views ingest + forward + nms_views_device(min_views=2) captured as one graph (kernel nodes only), replayed UNFENCED after
    eager steps on other tiles that use the same buffers: the bytes of the eager step on the same tiles"""
    m = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    W = raster.shape[1]
    strips = [torch.from_numpy(np.ascontiguousarray(raster[a:a + TILE])).to(dev) for a in (0, 70, 141)]
    origins = torch.tensor([(0, 0), (300, 0)], dtype=torch.int32, device=dev)
    views, V = FLIPS, len(FLIPS)
    ids = (C.c_int * V)(*views)
    tiles = torch.empty(2 * V, 3, S, S, device=dev)
    L = _lib.lib()

    def step(strip):
        check(L.ay_ingest_region_tiles_views_u8(ptr(strip), TILE, W, W * 3, 1, TILE, ptr(origins), 2, ids, V, S, ptr(tiles), _lib.stream_ptr()),
              "ay_ingest_region_tiles_views_u8")
        return nms_views_device(m.forward_device(tiles, out_slot=0), views, CONF, NMS, 256, min_views=2, img_dim=S, slot=7)

    ref = [[t.clone() for t in step(s)] for s in strips]             # eager results (also the warm-up: plans, buffers)
    torch.cuda.synchronize()
    counts = [r[2].tolist() for r in ref]
    print("rows kept per tile and strip", counts)
    assert any(c > 0 for cs in counts for c in cs)
    static = strips[0].clone()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        res = step(static)
    torch.cuda.synchronize()
    for k in (1, 2, 0, 1):
        step(strips[(k + 1) % 3])                                     # an eager step in between, on other tiles
        static.copy_(strips[k])
        g.replay()
        torch.cuda.synchronize()
        rows, keep, count, cand = res
        assert torch.equal(count, ref[k][2]) and torch.equal(cand, ref[k][3])
        for b in range(2):
            n = int(count[b])
            assert torch.equal(rows[b, :n], ref[k][0][b, :n]) and torch.equal(keep[b, :n], ref[k][1][b, :n])
