"""Training windows out of annotated slides on the device (-m gpu): ay_augment_ingest_window_u8 against ay_augment_ingest_u8 where
THE WINDOW RULE says they agree, against its NumPy restatement (tests/window_reference.py) everywhere else, BIT FOR BIT; the records
that must read nothing; wsi.SlideSampler staged against resident, its images against its labels, and train(source=...)."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

import augment_reference as ar
import window_reference as wr
from amyloid_yolo_paper_amd import _lib, augment as ag, cfg_gen
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import SlideSampler

pytestmark = pytest.mark.gpu

GUARD = 64
WINDOWS = [(48, 48), (80, 80), (40, 56)]
SIZES = [30, 36, 64, 96]      # scalar stores | a multiple of 4, not of 16 | exactly one 64-wide block | a partial second block
ALL = dict(rotate=20.0, translate=0.2, fliplr=0.5, sharpen=0.2, dropout=0.01, brightness=30.0, hue=20.0)
ALONE = {"rotate": dict(rotate=20.0), "translate": dict(translate=0.2), "flip": dict(fliplr=1.0), "sharpen": dict(sharpen=0.2),
         "dropout": dict(dropout=0.01), "brightness": dict(brightness=30.0), "hue": dict(hue=20.0), "all": ALL}


def ranges_of(d):
    return ag.AugmentRanges(**{**vars(ag.OFF), **d})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def rand_img(seed, h, w):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[: h // 5, : w // 4] = 255
    img[h // 2: h // 2 + h // 6, w // 3: w // 2] = 0
    return img


def assert_bits(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = got.view(np.uint32) != want.view(np.uint32)
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {i}: {got[i]!r} vs {want[i]!r}")


def run_entry(dev, entry, data, recs, S, lead=0, src_bytes=None, misalign=0):
    """one of the two entry points on `data` (flat uint8) and `recs` (used as they are).  The source sits between GUARD bytes of
    0xEE, `lead` bytes behind a 16-byte boundary; the output is pre-filled, starts `misalign` floats behind a boundary and is
    followed by guard words.  Two runs with two fills: the same bytes, and nothing written around the output."""
    B = len(recs)
    buf = np.full(GUARD + lead + len(data) + GUARD, 0xEE, np.uint8)
    buf[GUARD + lead:GUARD + lead + len(data)] = data
    src = torch.from_numpy(buf).to(dev)
    assert src.data_ptr() % 16 == 0
    table = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).to(dev)
    n = B * 3 * S * S
    out = torch.empty(misalign + n + GUARD, device=dev, dtype=torch.float32)
    f = getattr(_lib.lib(), entry)
    outs = []
    for fill in (-7.0, 9.0):
        out.fill_(fill)
        check(f(C.c_void_p(src.data_ptr() + GUARD + lead), len(data) if src_bytes is None else src_bytes, ptr(table), B, S,
                C.c_void_p(out.data_ptr() + 4 * misalign), _lib.stream_ptr()), entry)
        host = out.cpu().numpy()
        assert (host[:misalign] == fill).all() and (host[misalign + n:] == fill).all()
        outs.append(host[misalign:misalign + n].reshape(B, 3, S, S).copy())
    assert outs[0].tobytes() == outs[1].tobytes()
    return outs[0]


def pack(blocks, pads):
    """blocks (uint8 [bh,bw,3] each) one after another, rows of block i followed by pads[i] bytes of 0x77 (but the last row) ->
    (flat data, src_offsets, row_strides)"""
    parts, offs, strides, off = [], [], [], 0
    for blk, pad in zip(blocks, pads):
        bh, bw = blk.shape[:2]
        stride = 3 * bw + pad
        offs.append(off)
        strides.append(stride)
        if bh and bw:
            rows = np.full((bh, stride), 0x77, np.uint8)
            rows[:, :3 * bw] = blk.reshape(bh, 3 * bw)
            flat = rows.reshape(-1)[:(bh - 1) * stride + 3 * bw]
            parts.append(flat)
            off += len(flat)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), offs, strides


# ---- 1. window == block, context 0: the tile kernel -------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_identity_geometry_equals_the_tile_kernel(dev, S):
    imgs = [rand_img(S + k, h, w) for k, (h, w) in enumerate(WINDOWS)]
    table = ag.sample_params(np.random.default_rng([S, 1]), WINDOWS, ranges_of(ALL))
    data = np.concatenate([i.reshape(-1) for i in imgs])
    want = run_entry(dev, "ay_augment_ingest_u8", data, table.dev, S)
    wt = ag.make_window_table(table, WINDOWS, [(0, 0)] * 3, context=False, fill=123.0)
    assert wt.dev["src_offset"].tolist() == table.dev["src_offset"].tolist()
    for misalign in (0, 1):
        assert_bits(run_entry(dev, "ay_augment_ingest_window_u8", data, wt.dev, S, misalign=misalign), want, f"S {S} misalign {misalign}")
    got = ag.augment_ingest_windows_device(torch.from_numpy(data), wt, S).cpu().numpy()       # the public wrapper, host source
    assert_bits(got, want, "augment_ingest_windows_device, host source")
    got = ag.augment_ingest_windows_device(torch.from_numpy(data).to(dev), wt, S).cpu().numpy()
    assert_bits(got, want, "augment_ingest_windows_device, resident source")


# ---- 2. context 0, the window inside a larger block: the tile kernel on the cut-out tile ------------------------------------------
@pytest.mark.parametrize("S", SIZES)
def test_window_inside_a_block_equals_the_tile_kernel_on_the_cut(dev, S):
    origins = [(13, 9), (5, 21), (1, 1)]
    blocks = [rand_img(S + 10 + k, h + 30, w + 40) for k, (h, w) in enumerate(WINDOWS)]
    cuts = [b[y:y + h, x:x + w] for b, (x, y), (h, w) in zip(blocks, origins, WINDOWS)]
    table = ag.sample_params(np.random.default_rng([S, 2]), WINDOWS, ranges_of(ALL))
    want = run_entry(dev, "ay_augment_ingest_u8", np.concatenate([c.reshape(-1) for c in cuts]), table.dev, S)
    data, offs, strides = pack(blocks, [5, 5, 5])
    wt = ag.make_window_table(table, [b.shape[:2] for b in blocks], origins, context=False, fill=255.0, src_offsets=offs, row_strides=strides)
    assert all(int(r["row_stride"]) == 3 * int(r["bw"]) + 5 for r in wt.dev)
    assert_bits(run_entry(dev, "ay_augment_ingest_window_u8", data, wt.dev, S, lead=1), want, f"S {S}")


# ---- 3. the rule, exact -------------------------------------------------------------------------------------------------------------
def cases(h, w):
    """(block size, window origin) of a window h x w: inside | negative origin | past the far edge | the block smaller than the
    window | a 1 x 1 block | no pixels (twice) | nowhere near the block"""
    return [((h + 30, w + 40), (13, 9)), ((h + 10, w + 10), (-7, -11)), ((h + 10, w + 10), (w // 2 + 3, h // 2 + 1)),
            ((h // 2, w // 3), (-5, -4)), ((1, 1), (-(w // 2), -(h // 2))), ((0, 5), (0, 0)), ((3, 0), (-2, 1)),
            ((h, w), (100000, -100000))]


def window_batch(seed, ranges, context):
    sizes, blocks, origins = [], [], []
    for h, w in WINDOWS:
        for k, (bs, o) in enumerate(cases(h, w)):
            sizes.append((h, w))
            blocks.append(rand_img(seed + len(blocks), *bs) if bs[0] and bs[1] else np.zeros(bs + (3,), np.uint8))
            origins.append(o)
    n = len(sizes)
    table = ag.sample_params(np.random.default_rng([seed, 3]), sizes, ranges)
    data, offs, strides = pack(blocks, [(0, 5, 1)[i % 3] for i in range(n)])
    wt = ag.make_window_table(table, [b.shape[:2] for b in blocks], origins, context=context, src_offsets=offs, row_strides=strides)
    wt.dev["fill"] = [(0.0, 255.0, 37.5)[i % 3] for i in range(n)]
    return blocks, data, wt


@pytest.mark.parametrize("context", [0, 1])
@pytest.mark.parametrize("op", list(ALONE))
def test_window_rule_bit_for_bit(dev, op, context):
    blocks, data, wt = window_batch(len(op) + 7 * context, ranges_of(ALONE[op]), bool(context))
    for S in SIZES:
        want = np.stack([wr.augment(b, S, wr.from_window_row(r)) for b, r in zip(blocks, wt.dev)])
        got = run_entry(dev, "ay_augment_ingest_window_u8", data, wt.dev, S, lead=S % 3, misalign=S % 2)
        for i in range(len(blocks)):
            assert_bits(got[i], want[i], f"{op} context {context} S {S} record {i}")

def test_far_and_non_finite_tap_positions_stay_inside_the_block(dev):
    """inverse matrices that send the taps anywhere: 1e30 is beyond every block (the reference agrees: all `fill`), zeros collapse the
    window onto one pixel, inf and NaN have no defined value -- the call is safe, the same twice, and finite"""
    h = w = 48
    blk = rand_img(5, 60, 70)
    invs = [(1, 0, 1e30, 0, 1, 0), (1, 0, 0, 0, 1, -1e30), (0, 0, 0, 0, 0, 0), (1, 0, np.inf, 0, 1, 0), (np.nan, 0, 0, 0, 1, 0), (1, 0, 0, 0, -np.inf, 7)]
    table = ag.make_table([(h, w)] * len(invs))
    table.dev["inv"] = np.array(invs, np.float32)
    for context in (False, True):
        wt = ag.make_window_table(table, [(60, 70)] * len(invs), [(4, 6)] * len(invs), context=context, fill=200.0, src_offsets=[0] * len(invs))
        got = run_entry(dev, "ay_augment_ingest_window_u8", blk.reshape(-1), wt.dev, 36)
        assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
        for i in range(3):
            assert_bits(got[i], wr.augment(blk, 36, wr.from_window_row(wt.dev[i])), f"context {context} record {i}")


# ---- 4. block independence: staged by the sampler == resident ---------------------------------------------------------------------
H, W, TILE = 400, 520, 160


def synthetic_slide(seed=0):
    """bright noise (every channel >= 160) with dark-red rectangles (R <= 30, B = 255), annotated exactly"""
    rng = np.random.default_rng(seed)
    raster = rng.integers(160, 256, size=(H, W, 3), dtype=np.uint8)
    rects = [(30, 40, 70, 64), (200, 90, 236, 130), (330, 60, 380, 84), (120, 250, 150, 300), (420, 300, 470, 330), (250, 330, 290, 352),
             (8, 180, 40, 210), (480, 150, 512, 190)]
    for x1, y1, x2, y2 in rects:
        raster[y1:y2, x1:x2, 0] = rng.integers(0, 31, size=(y2 - y1, x2 - x1))
        raster[y1:y2, x1:x2, 1] = rng.integers(0, 256, size=(y2 - y1, x2 - x1))
        raster[y1:y2, x1:x2, 2] = 255
    targets = np.array([[k % 2, *r] for k, r in enumerate(rects)], np.float64)
    return raster, targets


FULL = np.ones((3, 4), bool)


@pytest.mark.parametrize("S", [36, 96])
def test_staged_sub_blocks_and_the_resident_raster_give_the_same_batches(dev, S):
    raster, targets = synthetic_slide()
    roi = (16, 10, 510, 396)
    kw = dict(tile=TILE, img_size=S, batch_size=6, batches=3, seed=S, context=True, tile_mask=FULL, fill=37.5)
    staged = SlideSampler([(raster, targets, roi)], **kw)
    wide = torch.from_numpy(np.ascontiguousarray(np.pad(raster, ((0, 0), (0, 3), (0, 0))))).to(dev)[:, :W]      # rows 3 * (W + 3) bytes apart
    assert wide.stride(0) == 3 * (W + 3)
    resident = SlideSampler([(wide, targets, roi)], **kw)
    n = 0
    for (a, ta), (b, tb) in zip(staged, resident):
        assert a.shape == (6, 3, S, S) and a.is_cuda and ta.is_cuda and ta.shape[1] == 6
        assert_bits(a.cpu().numpy(), b.cpu().numpy(), f"batch {n}")
        assert torch.equal(ta, tb)
        n += 1
    assert n == 3 == len(staged)


# ---- 5. records that must read nothing; bad arguments ------------------------------------------------------------------------------
def test_a_block_that_leaves_the_buffer_reads_nothing(dev):
    h, w, S = 48, 48, 36
    blocks = [rand_img(k, 60, 70) for k in range(10)]
    data, offs, strides = pack(blocks, [5] * 10)
    for context in (False, True):
        table = ag.sample_params(np.random.default_rng(3), [(h, w)] * 10, ranges_of(ALL))
        wt = ag.make_window_table(table, [(60, 70)] * 10, [(4, 6)] * 10, context=context, fill=90.0, src_offsets=offs, row_strides=strides)
        good = np.stack([wr.augment(b, S, wr.from_window_row(r)) for b, r in zip(blocks, wt.dev)])
        recs = wt.dev.copy()
        recs[0]["bh"] = 4096                                   # more rows than the buffer holds
        recs[1]["src_offset"] = -3
        recs[2]["row_stride"] = -215
        recs[3]["row_stride"] = 2 ** 62                        # (bh - 1) * row_stride overflows 64 bits
        recs[4]["row_stride"] = 2 ** 63 - 1
        recs[5]["src_offset"] = 2 ** 63 - 1
        recs[6]["aug"]["h"] = 0
        recs[7]["aug"]["w"] = -5
        recs[9]["src_offset"] += 1                             # the last block: one byte over the end
        got = run_entry(dev, "ay_augment_ingest_window_u8", data, recs, S, lead=1)
        assert_bits(got[8], good[8], "the consistent record")
        for i in (0, 1, 2, 3, 4, 5, 9):
            assert_bits(got[i], wr.padding(S, wr.from_window_row(recs[i])), f"context {context} record {i}")
        for i in (6, 7):                                       # no window: all padding too
            assert_bits(got[i], wr.padding(S, wr.from_window_row(wt.dev[i])), f"context {context} record {i}")
        # the same table with the buffer declared one byte short: only the last block no longer fits
        got = run_entry(dev, "ay_augment_ingest_window_u8", data, wt.dev, S, src_bytes=len(data) - 1)
        assert_bits(got[:9], good[:9], "the blocks that still fit")
        assert_bits(got[9], wr.padding(S, wr.from_window_row(wt.dev[9])), "the block that does not")


def test_bad_arguments_are_refused(dev):
    L = _lib.lib()
    x = torch.zeros(64, device=dev)
    assert L.ay_augment_ingest_window_u8(None, 10, ptr(x), 1, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_window_u8(ptr(x), 10, None, 1, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_window_u8(ptr(x), 10, ptr(x), 1, 8, None, None) == -1 and b"ay_augment_ingest_window_u8" in L.ay_last_error()
    assert L.ay_augment_ingest_window_u8(ptr(x), 0, ptr(x), 1, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_window_u8(ptr(x), 10, ptr(x), 0, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_window_u8(ptr(x), 10, ptr(x), 1, 0, ptr(x), None) == -1 and b"ay_augment_ingest_window_u8" in L.ay_last_error()
    assert L.ay_augment_ingest_u8(ptr(x), 10, ptr(x), 1, 0, ptr(x), None) == -1 and b"ay_augment_ingest_u8:" in L.ay_last_error()


# ---- 6. the image and its labels move together -------------------------------------------------------------------------------------
GEOMETRIC = dict(rotate=20.0, translate=0.2, fliplr=0.5)
EDGE = 3.0     # source pixels: no annotation may end this close to the window's edge (see pick_sampler_seed)


def moved_box(b, x, y, rec):
    """the unclipped bounding box, in window pixels, of slide box b = (x1, y1, x2, y2) under the record (the label rule's geometry)"""
    xs = np.array([b[0], b[2], b[0], b[2]]) - x - TILE / 2
    ys = np.array([b[1], b[1], b[3], b[3]]) - y - TILE / 2
    A = rec.A
    px = A[0, 0] * xs + A[0, 1] * ys + A[0, 2] + TILE / 2
    py = A[1, 0] * xs + A[1, 1] * ys + A[1, 2] + TILE / 2
    if rec.flip:
        px = TILE - px
    return px.min(), py.min(), px.max(), py.max()


def pick_sampler_seed(raster, targets, context, B):
    """The first seed whose first batch has a rotated (>= 10 degrees) sample, a flipped one, and no annotation whose moved box ends
    within EDGE pixels of the window's edge: such a box is either kept with a visible part or lies clear of the window, so that no
    dark pixel belongs to a label the clip removed.  Decided on the CPU."""
    for seed in range(500):
        s = SlideSampler([(raster, targets)], tile=TILE, img_size=96, batch_size=B, batches=1, seed=seed, context=context,
                         ranges=ranges_of(GEOMETRIC), tile_mask=FULL, p_object=0.7)
        p = s.plan_batch()
        degs = [abs(math.degrees(math.atan2(A[1, 0], A[0, 0]))) for A in p.table.A]
        if max(degs) < 10.0 or not p.table.dev["flip"].any():
            continue
        ok = True
        for i, (x, y) in enumerate(p.origins):
            for t in targets:
                b = t[1:]
                if not context:   # the label rule cuts to the window before it moves the box
                    b = (max(b[0], x), max(b[1], y), min(b[2], x + TILE), min(b[3], y + TILE))
                    if b[2] - b[0] <= 0 or b[3] - b[1] <= 0:
                        continue
                x1, y1, x2, y2 = moved_box(b, x, y, p.table[i])
                for lo, hi in ((x1, x2), (y1, y2)):
                    ok &= not (abs(hi) < EDGE or abs(lo - TILE) < EDGE)       # ends just inside or just outside the window
        if ok:
            return seed
    raise AssertionError("no seed found")


@pytest.mark.parametrize("context", [False, True])
def test_image_and_labels_move_together(dev, context):
    raster, targets = synthetic_slide(1)
    S, B = 96, 6
    seed = pick_sampler_seed(raster, targets, context, B)
    kw = dict(tile=TILE, img_size=S, batch_size=B, batches=1, seed=seed, context=context, ranges=ranges_of(GEOMETRIC), tile_mask=FULL, p_object=0.7)
    plan = SlideSampler([(raster, targets)], **kw).plan_batch()
    imgs, rows = next(iter(SlideSampler([(raster, targets)], **kw)))
    imgs, rows = imgs.cpu().numpy(), rows.cpu().numpy().astype(np.float64)
    assert np.allclose(rows, plan.targets, atol=1e-6) and len(rows) > 0
    # the images are the window rule on the whole slide
    table = ag.make_window_table(plan.table, [(H, W)] * B, [tuple(o) for o in plan.origins], context=context, fill=255.0)
    for i in range(B):
        assert_bits(imgs[i], wr.augment(raster, S, wr.from_window_row(table.dev[i])), f"sample {i}")
    # Margin.  A dark output pixel has a tap in a rectangle, so its sample point lies within 1 source pixel per axis, sqrt(2) in
    # all, of the rectangle, and the image of that point -- the centre of source pixel q = floor(X * scale) -- within sqrt(2) of
    # the moved box.  Output pixel X spans [X, X + 1) * scale, which lies within scale + 0.5 of q + 0.5.
    scale = TILE / S
    margin = (math.sqrt(2.0) + 0.5) / scale + 1.0 + 1e-4       # output pixels (1e-4: the targets are stored in fp32)
    n_dark = 0
    for i in range(B):
        dark = (imgs[i, 0] < 60 / 255) & (imgs[i, 2] > 128 / 255)           # (black padding has no blue)
        box = rows[rows[:, 0] == i][:, 2:] * S
        ys, xs = np.nonzero(dark)
        n_dark += len(xs)
        for X, Y in zip(xs, ys):
            inside = (box[:, 0] - box[:, 2] / 2 - margin <= X) & (X + 1 <= box[:, 0] + box[:, 2] / 2 + margin) & \
                     (box[:, 1] - box[:, 3] / 2 - margin <= Y) & (Y + 1 <= box[:, 1] + box[:, 3] / 2 + margin)
            assert inside.any(), (i, X, Y, box)
    assert n_dark > 100
    # a rotated sample: its corners show the slide with context, black without
    k = int(np.argmax([abs(math.degrees(math.atan2(A[1, 0], A[0, 0]))) for A in plan.table.A]))
    corners = imgs[k][:, [0, 0, -1, -1], [0, -1, 0, -1]]
    if context:
        assert (corners[2] >= 160 / 255).all()      # blue of slide pixels (>= 160) or of the fill beyond it, never the tile rule's black
    else:
        assert (corners == 0).any()


# ---- 7. train(source=...) ----------------------------------------------------------------------------------------------------------
def test_train_from_a_slide_is_finite_and_reproducible(tmp_path, tmp_cfg_dir):
    from amyloid_yolo_paper_amd.train import train
    raster, targets = synthetic_slide(2)
    (tmp_path / "classes.names").write_text("CAA\nCored\n")
    (tmp_path / "custom.data").write_text(f"classes= 2\nnames={tmp_path}/classes.names\n")
    cfg = cfg_gen.write_cfg(2, tmp_cfg_dir)
    runs = []
    for run in range(2):
        source = SlideSampler([(raster, targets)], tile=TILE, img_size=96, batch_size=2, batches=4, seed=5)      # its own tissue map
        seen = []
        source.hooks.append(lambda imgs, t: seen.append((hashlib.sha256(imgs.cpu().numpy().tobytes()).hexdigest(),
                                                         hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest(), tuple(imgs.shape))))
        _, hist = train(epochs=1, gradient_accumulations=2, model_def=cfg, data_config=str(tmp_path / "custom.data"), img_size=96,
                        checkpoint_dir=str(tmp_path / f"ckpt{run}"), seed=5, precision="bf16", source=source)
        assert len(hist) == 4 and all(np.isfinite(hist)), hist
        assert len(seen) == 4 and all(s[2] == (2, 3, 96, 96) for s in seen)
        runs.append((seen, hist))
    assert runs[0][0] == runs[1][0]                              # the same seed: byte-identical batches and targets
    assert runs[0][1] == runs[1][1]                              # ... and loss histories
    assert len({s[0] for s in runs[0][0]}) == 4                  # which differ from batch to batch
