"""CPU: training windows out of annotated slides -- the record mirrors of ay_aug_window_params, the NumPy restatement of THE WINDOW
RULE against the tile rule it extends, ``augment.footprint`` as a superset of the taps, the bookkeeping of ``wsi.SlideSampler``
(no device call: ``plan_batch`` is host code) and its labels."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import augment_reference as ar
import window_reference as wr
from amyloid_yolo_paper_amd import _lib, augment as ag
from amyloid_yolo_paper_amd.wsi import SlideSampler

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rand_img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ---- ABI mirror -----------------------------------------------------------------------------------------------------------------
def test_window_record_mirrors_agree():
    assert ag.AUG_WINDOW_DTYPE.itemsize == C.sizeof(_lib.AugWindowParams) == 136
    for name, _ in _lib.AugWindowParams._fields_:
        assert ag.AUG_WINDOW_DTYPE.fields[name][1] == getattr(_lib.AugWindowParams, name).offset, name
    assert ag.AUG_WINDOW_DTYPE.fields["aug"][0] == ag.AUG_DTYPE
    # the header declares the same fields in the same order
    text = open(os.path.join(REPO, "include", "amyloid_yolo.h")).read()
    body = re.search(r"typedef struct ay_aug_window_params \{(.*?)\} ay_aug_window_params;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n.strip() for decl in body.split(";") if decl.strip() for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == ["src_offset", "row_stride", "bh", "bw", "x0", "y0", "context", "fill", "aug"]
    # (the C size: 8 + 8 + 6 * 4 + sizeof(ay_aug_params) = 96, no padding anywhere)
    assert C.sizeof(_lib.AugParams) == 96 and 40 + 96 == 136


# ---- the reference --------------------------------------------------------------------------------------------------------------
def window_rec(table, i, x0=0, y0=0, context=0, fill=255.0):
    rec = ar.from_row(table.dev[i])
    rec.update(x0=x0, y0=y0, context=context, fill=np.float32(fill))
    return rec


@pytest.mark.parametrize("h,w,S", [(96, 96, 64), (90, 150, 96), (150, 90, 70), (64, 48, 33)])
def test_window_reference_with_window_equal_block_is_the_tile_reference(h, w, S):
    img = rand_img(h + w, h, w)
    for seed in range(3):
        t = ag.sample_params(np.random.default_rng(seed), [(h, w)])
        for fill in (0.0, 255.0):
            assert wr.augment(img, S, window_rec(t, 0, fill=fill)).tobytes() == ar.augment(img, S, ar.from_row(t.dev[0])).tobytes()


def test_window_reference_inside_a_larger_block_is_the_tile_reference_on_the_cut():
    big = rand_img(3, 120, 140)
    t = ag.sample_params(np.random.default_rng(4), [(48, 56)])
    got = wr.augment(big, 36, window_rec(t, 0, x0=31, y0=17))
    assert got.tobytes() == ar.augment(big[17:17 + 48, 31:31 + 56], 36, ar.from_row(t.dev[0])).tobytes()
    ctx = wr.augment(big, 36, window_rec(t, 0, x0=31, y0=17, context=1))
    assert ctx.tobytes() != got.tobytes()               # the surroundings are there


def test_window_reference_without_pixels_is_fill_inside_the_window():
    t = ag.make_table([(40, 40)])
    for blk in (np.zeros((0, 7, 3), np.uint8), np.zeros((5, 0, 3), np.uint8)):
        assert (wr.augment(blk, 30, window_rec(t, 0, context=1, fill=51.0)) == np.float32(51) / np.float32(255)).all()
        assert (wr.augment(blk, 30, window_rec(t, 0, context=0, fill=51.0)) == np.float32(51) / np.float32(255)).all()


# ---- footprint ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [30, 64, 96])
def test_footprint_is_a_superset_of_the_taps(S):
    """200 records at the limits of the default ranges (+-20 degrees, +-20 %, flipped or not), square and ragged windows"""
    rng = np.random.default_rng(S)
    blk = np.zeros((1, 1, 3), np.uint8)
    slack = []
    for n in range(200):
        h, w = [(80, 80), (48, 48), (40, 56), (56, 40)][n % 4]
        deg = (20.0, -20.0, rng.uniform(-20, 20))[n % 3]
        tx, ty = (rng.choice([-0.2, 0.2, rng.uniform(-0.2, 0.2)]) * w, rng.choice([-0.2, 0.2, rng.uniform(-0.2, 0.2)]) * h)
        t = ag.make_table([(h, w)], A=[ag.forward_matrix(deg, tx, ty)], flip=[n // 2 % 2])
        taps = []
        wr.warp(blk, S, window_rec(t, 0, context=1), taps)
        y1, x1, y2, x2 = taps[0]                            # inclusive
        f = ag.footprint(t[0], (h, w), S)
        assert f[0] <= x1 and f[1] <= y1 and f[2] > x2 and f[3] > y2, (n, f, taps[0])
        slack.append(max(x1 - f[0], y1 - f[1], f[2] - 1 - x2, f[3] - 1 - y2))
    assert max(slack) <= 4 + max(80, 80) / S            # ... and no loose one: the taps of a coarse output start up to D / S inside
    ident = ag.footprint(ag.make_table([(80, 80)])[0], 80, 96)
    assert ident == (-1, -1, 81, 81)                        # identity: taps 0 .. 80 (floor and floor + 1 of 0 .. 79), the margin below


# ---- the sampler's bookkeeping --------------------------------------------------------------------------------------------------
H, W, TILE = 400, 520, 160


def slide(seed=0, n=12):
    rng = np.random.default_rng(seed)
    raster = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    x1, y1 = rng.uniform(0, W - 40, n), rng.uniform(0, H - 40, n)
    t = np.stack([rng.integers(0, 2, n).astype(np.float64), x1, y1, x1 + rng.uniform(8, 40, n), y1 + rng.uniform(8, 40, n)], 1)
    return raster, t


def full_mask(h=H, w=W, tile=TILE):
    return np.ones((-(-h // tile), -(-w // tile)), bool)


def test_windows_lie_inside_roi_and_slide():
    raster, t = slide()
    for roi in (None, (37, 21, 480, 390), (-50, -50, 300, 9999)):
        s = SlideSampler([(raster, t, roi)], tile=TILE, img_size=96, batch_size=16, seed=1, tile_mask=full_mask(), p_object=0.5)
        bx1, by1, bx2, by2 = s.slides[0].block
        assert (bx1, by1, bx2, by2) == ((0, 0, W, H) if roi is None else (max(roi[0], 0), max(roi[1], 0), min(roi[2], W), min(roi[3], H)))
        for _ in range(6):
            p = s.plan_batch()
            assert (p.origins[:, 0] >= bx1).all() and (p.origins[:, 0] + TILE <= bx2).all()
            assert (p.origins[:, 1] >= by1).all() and (p.origins[:, 1] + TILE <= by2).all()
            r = p.rects                                       # what is staged never leaves the block either
            assert (r[:, 0] >= bx1).all() and (r[:, 1] >= by1).all() and (r[:, 2] <= bx2).all() and (r[:, 3] <= by2).all()
            assert set(p.kind.tolist()) <= {0, 1}


def test_object_picks_put_the_annotation_centre_inside_the_window():
    raster, t = slide(2)
    s = SlideSampler([(raster, t)], tile=TILE, img_size=96, batch_size=32, seed=3, tile_mask=full_mask(), p_object=1.0)
    seen = set()
    for _ in range(8):
        p = s.plan_batch()
        assert (p.kind == 1).all()
        for (x, y), i in zip(p.origins, p.pick):
            _, x1, y1, x2, y2 = s.slides[0].targets[i]
            assert x <= (x1 + x2) / 2 < x + TILE and y <= (y1 + y2) / 2 < y + TILE
            seen.add(int(i))
    assert len(seen) == len(t)                                # every annotation gets picked
    # hard boxes, when asked for
    hard = np.array([[300.0, 200.0, 330.0, 240.0]])
    s = SlideSampler([dict(raster=raster, targets=t, hard=hard)], tile=TILE, img_size=96, batch_size=32, seed=3, tile_mask=full_mask(), p_hard=1.0)
    p = s.plan_batch()
    assert (p.kind == 2).all() and (p.origins[:, 0] <= 315).all() and (p.origins[:, 0] + TILE > 315).all()
    assert (p.origins[:, 1] <= 220).all() and (p.origins[:, 1] + TILE > 220).all()


def test_tile_picks_hit_only_wanted_tiles_and_unannotated_slides_fall_back_to_tissue():
    raster, _ = slide(4)
    mask = np.zeros((3, 4), bool)
    mask[1, 2] = mask[2, 0] = True
    big = np.zeros((0, 5))
    s = SlideSampler([(raster, big)], tile=TILE, img_size=96, batch_size=32, seed=5, tile_mask=mask, p_object=1.0)
    hit = set()
    for _ in range(4):
        p = s.plan_batch()
        assert (p.kind == 0).all()                            # no annotation: tissue, whatever p_object says
        for (x, y), i in zip(p.origins, p.pick):
            x1, y1, x2, y2 = s.slides[0].wanted[i]
            assert (x1, y1) in {(320, 160), (0, 320)}
            assert x < x2 and x + TILE > x1 and y < y2 and y + TILE > y1      # the window holds a point of the wanted tile
            hit.add((int(x1), int(y1)))
    assert hit == {(320, 160), (0, 320)}


def test_slides_are_drawn_by_weight():
    (r0, t0), (r1, t1) = slide(6, n=30), slide(7, n=2)
    none = np.zeros((3, 4), bool)
    s = SlideSampler([(r0, t0), (r1, t1)], tile=TILE, img_size=96, batch_size=64, seed=0, tile_mask=[none, none], p_object=0.0)
    assert (np.concatenate([s.plan_batch().kind for _ in range(2)]) == 1).all()     # no wanted tile: the annotations
    share = np.mean(np.concatenate([s.plan_batch().slide for _ in range(10)]) == 0)
    assert abs(share - 30 / 32) < 0.04
    assert len(s) == 1 and len(SlideSampler([(r0, t0)], tile=TILE, batch_size=4, tile_mask=full_mask())) == math.ceil((30 + 12) / 4)


def plans(seed, rank, ranges=None, n=3, **kw):
    raster, t = slide(8)
    s = SlideSampler([(raster, t)], tile=TILE, img_size=96, batch_size=8, seed=seed, rank=rank, ranges=ranges, tile_mask=full_mask(), **kw)
    return [s.plan_batch() for _ in range(n)], s


def test_same_seed_and_rank_same_batches_another_rank_others():
    (a, _), (b, _), (c, _) = plans(11, 0), plans(11, 0), plans(11, 1)
    for pa, pb in zip(a, b):
        assert np.array_equal(pa.origins, pb.origins) and pa.table.dev.tobytes() == pb.table.dev.tobytes()
        assert np.array_equal(pa.targets, pb.targets) and np.array_equal(pa.rects, pb.rects)
    assert not np.array_equal(a[0].origins, c[0].origins) and a[0].table.dev.tobytes() != c[0].table.dev.tobytes()
    assert not np.array_equal(a[0].origins, a[1].origins)    # the stream moves on


def test_the_draw_count_per_sample_does_not_depend_on_what_is_switched_off():
    (on, s_on), (off, s_off) = plans(12, 0), plans(12, 0, ranges=ag.OFF)
    (flat, s_flat), (hard, s_hard) = plans(12, 0, p_object=0.0, context=False), plans(12, 0, p_hard=0.0, p_object=1.0)
    for pa, pb in zip(on, off):
        assert np.array_equal(pa.origins, pb.origins) and np.array_equal(pa.kind, pb.kind)     # the same windows ...
        assert np.array_equal(pb.table.A, np.tile([[1.0, 0, 0], [0, 1.0, 0]], (8, 1, 1)))        # ... not moved
    state = lambda s: s.rng.bit_generator.state["state"]
    assert state(s_on) == state(s_off) == state(s_flat) == state(s_hard)
    ref = np.random.default_rng([12, 0])                      # 8 position draws, then sample_params, per sample
    for _ in range(3 * 8):
        ref.uniform(0.0, 1.0, SlideSampler.N_POSITION_DRAWS)
        ag.sample_params(ref, [(TILE, TILE)])
    assert state(s_on) == ref.bit_generator.state["state"]
    assert on[0].table.dev.tobytes() == flat[0].table.dev.tobytes()   # the records do not depend on what was picked


def test_value_errors():
    raster, t = slide()
    with pytest.raises(ValueError):
        SlideSampler([(raster, t)], tile=401, tile_mask=full_mask(tile=401))                 # taller than the slide
    with pytest.raises(ValueError):
        SlideSampler([(raster, t, (0, 0, 159, 400))], tile=TILE, tile_mask=full_mask())       # wider than the roi
    with pytest.raises(ValueError):
        SlideSampler([], tile=TILE)
    with pytest.raises(ValueError):
        SlideSampler([(raster, t)], tile=TILE, tile_mask=np.ones((2, 2), bool))               # another grid
    with pytest.raises(ValueError):
        SlideSampler([(raster, np.zeros((0, 5)))], tile=TILE, tile_mask=np.zeros((3, 4), bool))   # nothing to pick
    with pytest.raises(ValueError):
        SlideSampler([(raster, t)], tile=TILE, tile_mask=full_mask(), p_object=1.5)
    with pytest.raises(ValueError):
        SlideSampler([(raster.astype(np.float32), t)], tile=TILE, tile_mask=full_mask())
    with pytest.raises(ValueError):
        SlideSampler([(raster, t), (raster, t)], tile=TILE, tile_mask=full_mask())            # one mask, two slides


def test_iterating_without_a_device_raises(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    raster, t = slide()
    with pytest.raises(_lib.AyError):
        next(iter(SlideSampler([(raster, t)], tile=TILE, img_size=32, batch_size=2, tile_mask=full_mask())))


# ---- labels ---------------------------------------------------------------------------------------------------------------------
def by_hand(t, x, y, lim):
    """annotations cut to `lim` (x1, y1, x2, y2) and written relative to the TILE window at (x, y), one by one"""
    out = []
    for c, x1, y1, x2, y2 in t:
        x1, x2 = min(max(x1, lim[0]), lim[2]), min(max(x2, lim[0]), lim[2])
        y1, y2 = min(max(y1, lim[1]), lim[3]), min(max(y2, lim[1]), lim[3])
        if x2 - x1 > 0 and y2 - y1 > 0:
            out.append([c, ((x1 + x2) / 2 - x) / TILE, ((y1 + y2) / 2 - y) / TILE, (x2 - x1) / TILE, (y2 - y1) / TILE])
    return np.array(out).reshape(-1, 5)


@pytest.mark.parametrize("context", [False, True])
def test_identity_records_give_the_annotations_cut_to_the_window(context):
    raster, t = slide(9, n=40)
    s = SlideSampler([(raster, t)], tile=TILE, img_size=96, batch_size=16, seed=2, ranges=ag.OFF, context=context, tile_mask=full_mask())
    n = 0
    for _ in range(4):
        p = s.plan_batch()
        for i, (x, y) in enumerate(p.origins):
            got = p.targets[p.targets[:, 0] == i][:, 1:]
            want = by_hand(t, x, y, (x, y, x + TILE, y + TILE))     # the identity shows the window and nothing else
            assert got.shape == want.shape and np.allclose(got, want, atol=1e-12), (i, got, want)
            n += len(got)
    assert n > 50


def test_labels_are_clipped_to_the_block_before_they_move():
    raster, _ = slide(9)
    t = np.array([[1.0, 100.0, 100.0, 260.0, 180.0]])          # leaves the roi on the right
    roi = (40, 40, 220, 360)
    s = SlideSampler([(raster, t, roi)], tile=TILE, img_size=96, batch_size=4, seed=0, ranges=ag.OFF, tile_mask=full_mask(), p_object=0.0)
    p = s.plan_batch()
    for i, (x, y) in enumerate(p.origins):
        lim = (max(x, 40), max(y, 40), min(x + TILE, 220), min(y + TILE, 360))
        got = p.targets[p.targets[:, 0] == i][:, 1:]
        assert np.allclose(got, by_hand(t, x, y, lim), atol=1e-12)


def test_min_visible_drops_exactly_the_boxes_below_the_fraction():
    box = np.array([[0.0, 0.95, 0.5, 0.2, 0.2], [1.0, 0.5, 0.5, 0.2, 0.2], [2.0, 0.99, 0.02, 0.2, 0.2]])   # visible 0.75, 1, 0.55 * 0.6
    r = ag.make_table([(100, 100)])[0]
    assert [int(c) for c in ag.transform_labels(box, 100, 100, r)[:, 0]] == [0, 1, 2]
    assert [int(c) for c in ag.transform_labels(box, 100, 100, r, min_visible=0.32)[:, 0]] == [0, 1, 2]
    assert [int(c) for c in ag.transform_labels(box, 100, 100, r, min_visible=0.34)[:, 0]] == [0, 1]
    assert [int(c) for c in ag.transform_labels(box, 100, 100, r, min_visible=0.75)[:, 0]] == [0, 1]      # at the fraction: kept
    assert [int(c) for c in ag.transform_labels(box, 100, 100, r, min_visible=0.76)[:, 0]] == [1]
    # through the sampler, on rotated windows: the rows with min_visible are those rows without it whose visible share is enough
    raster, t = slide(10, n=60)
    kw = dict(tile=TILE, img_size=96, batch_size=16, seed=4, tile_mask=full_mask())
    a, b = SlideSampler([(raster, t)], **kw), SlideSampler([(raster, t)], min_visible=0.5, **kw)
    pa, pb = a.plan_batch(), b.plan_batch()
    assert len(pb.targets) < len(pa.targets)
    rows = {tuple(r) for r in pa.targets.tolist()}
    assert all(tuple(r) in rows for r in pb.targets.tolist())


def test_without_context_no_label_is_centred_outside_the_window():
    raster, t = slide(11, n=80)
    for context in (False, True):
        s = SlideSampler([(raster, t)], tile=TILE, img_size=96, batch_size=32, seed=6, context=context, tile_mask=full_mask())
        rows = np.concatenate([s.plan_batch().targets for _ in range(6)])
        assert len(rows) > 100
        inside = (rows[:, 2:4] >= 0).all() and (rows[:, 2:4] <= 1).all()
        assert inside                                        # transform_labels clips to the window in both modes
        assert (rows[:, 2] - rows[:, 4] / 2 >= -1e-12).all() and (rows[:, 2] + rows[:, 4] / 2 <= 1 + 1e-12).all()


def test_transform_labels_default_keyword_is_the_old_function():
    """the cases of tests/test_augment_cpu.py, through the function"""
    rec = lambda A=None, flip=0: ag.make_table([(1, 1)], A=None if A is None else [A], flip=[flip])[0]
    BOX = np.array([[2.0, 0.30, 0.40, 0.20, 0.10]])
    two = np.array([[0.0, 0.30, 0.40, 0.20, 0.10], [1.0, 0.80, 0.50, 0.20, 0.20]])
    for kw in ({}, {"min_visible": 0.0}):
        assert np.allclose(ag.transform_labels(BOX, 200, 200, rec(flip=1), **kw), [[2.0, 0.70, 0.40, 0.20, 0.10]], atol=1e-12)
        assert np.allclose(ag.transform_labels(BOX, 200, 200, rec(ag.forward_matrix(0.0, 20.0, -10.0)), **kw), [[2.0, 0.40, 0.35, 0.20, 0.10]], atol=1e-12)
        assert np.allclose(ag.transform_labels(BOX, 200, 200, rec(ag.forward_matrix(90.0, 0.0, 0.0)), **kw), [[2.0, 0.60, 0.30, 0.10, 0.20]], atol=1e-12)
        got = ag.transform_labels(two, 200, 200, rec(ag.forward_matrix(0.0, 40.0, 0.0)), **kw)
        assert np.allclose(got, [[0.0, 0.50, 0.40, 0.20, 0.10], [1.0, 0.95, 0.50, 0.10, 0.20]], atol=1e-12)
        got = ag.transform_labels(two, 200, 200, rec(ag.forward_matrix(0.0, 70.0, 0.0)), **kw)
        assert got.shape == (1, 5) and got[0, 0] == 0.0
        assert ag.transform_labels(np.zeros((0, 5)), 200, 200, rec(), **kw).shape == (0, 5)
    rng = np.random.default_rng(9)
    for _ in range(40):
        h, w = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        n = int(rng.integers(0, 6))
        boxes = np.concatenate([rng.integers(0, 3, (n, 1)).astype(np.float64), rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.02, 0.3, (n, 2))], 1)
        t = ag.sample_params(rng, [(h, w)])
        want = ar.labels(boxes, h, w, t.A[0], t[0].flip)
        got = ag.transform_labels(boxes, h, w, t[0])
        assert got.shape == want.shape and np.allclose(got, want, atol=1e-12)
        assert np.array_equal(got, ag.transform_labels(boxes, h, w, t[0], min_visible=0.0))


# ---- staging --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("context", [False, True])
def test_staged_sub_blocks_give_the_reference_of_the_whole_block(context):
    """block independence on the CPU: the window rule on what ``stage`` copied (footprint ∩ block) equals the rule on roi ∩ slide"""
    raster, t = slide(12)
    roi = (30, 20, 500, 390)
    s = SlideSampler([(raster, t, roi)], tile=TILE, img_size=30, batch_size=6, seed=8, context=context, tile_mask=full_mask(), fill=37.5)
    plan = s.plan_batch()
    table = s.window_table(plan)
    buf = np.full(s.staged_bytes(plan) + 16, 0xAB, np.uint8)
    s.stage(plan, table, buf)
    assert (buf[s.staged_bytes(plan):] == 0xAB).all()
    assert s.staged_bytes(plan) < 6 * (roi[2] - roi[0]) * (roi[3] - roi[1]) * 3
    for i in range(6):
        r = table.dev[i]
        bh, bw, off = int(r["bh"]), int(r["bw"]), int(r["src_offset"])
        assert int(r["row_stride"]) == 3 * bw and int(r["context"]) == int(context) and float(r["fill"]) == 37.5
        sub = buf[off:off + bh * bw * 3].reshape(bh, bw, 3)
        x, y = plan.origins[i]
        whole = wr.from_window_row(r)
        whole.update(x0=int(x) - roi[0], y0=int(y) - roi[1])
        want = wr.augment(raster[roi[1]:roi[3], roi[0]:roi[2]], 30, whole)
        assert wr.augment(sub, 30, wr.from_window_row(r)).tobytes() == want.tobytes(), i
