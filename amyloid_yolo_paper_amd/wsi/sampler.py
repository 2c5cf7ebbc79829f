"""Training reads the same rasters: :class:`SlideSampler` draws windows centred on annotations, hard cases and tissue out of annotated
slides and cuts them with the fused augmentation kernel under THE WINDOW RULE (``ay_augment_ingest_window_u8``), for
``train(source=...)``."""
import math

import numpy as np
import torch

from ..augment import AugmentRanges, AugTable, footprint, launch_windows, make_window_table, sample_params, transform_labels
from ..upload import Uploader, pack_records, record_offset
from .grid import check_tile_mask, hip_device, wanted_tiles
from .tissue import tissue_counts


class _Slide:
    """one annotated slide of a SlideSampler: the raster, its block (roi ∩ slide), the annotations and hard boxes that may be
    picked, the wanted tiles of the tissue grid and a grid index over the annotations"""


class SlideBatchPlan:
    """What one batch of a :class:`SlideSampler` is, decided on the host before anything reaches the device: per sample the slide
    (``slide``), what was picked (``kind``: 0 tile, 1 annotation, 2 hard box; ``pick``: its index), the window origin in slide
    pixels (``origins`` [B,2] = x, y), the augmentation records (``table``, an ``augment.AugTable`` of tile x tile windows), the
    rectangle of slide pixels the records may read (``rects`` [B,4] = x1, y1, x2, y2: the staged sub-block of a host raster, the
    whole block of a resident one) and the labels (``targets`` float64 [n,6]; their candidates are the annotations that intersect
    the sub-block a host raster would stage, for a resident raster too)."""

    def __init__(self, slide, kind, pick, origins, table, rects, targets):
        self.slide, self.kind, self.pick, self.origins, self.table, self.rects, self.targets = slide, kind, pick, origins, table, rects, targets


class SlideSampler:
    """A training source that cuts augmented windows straight out of annotated slides: an iterable with ``__len__`` that yields
    ``(imgs [B,3,S,S] fp32, targets [n,6])`` on the device, what ``augment.DeviceAugmenter`` yields, for ``train(source=...)``.

    ``slides``: a list of ``(raster, targets)`` or ``(raster, targets, roi)`` items or of dicts with the keys ``raster``,
    ``targets`` and optionally ``roi`` and ``hard`` ([K,4] boxes x1, y1, x2, y2 to revisit, e.g. ``missed`` / ``false_alarms`` of
    :func:`evaluate_region`).  ``raster`` is a uint8 ``[H,W,3]`` NumPy array or memmap (staged per batch) or a device tensor (read
    in place); all slides of a sampler are of one kind.  ``targets`` [T,5] = (class, x1, y1, x2, y2) in slide pixels, as
    :func:`evaluate_region` takes them; ``roi`` = (x1, y1, x2, y2) is the annotated part of the slide (default: all of it).
    Only ``shrink=1`` is supported: the caller passes the level they train at.

    The BLOCK of a slide is ``roi ∩ slide``.  No pixel outside it is ever shown to the network (an unlabelled plaque cannot enter
    through a rotated corner); beyond it lies ``fill``.  ``tile`` must fit into the block on both axes (``ValueError``).  With
    ``context=True`` a rotated or shifted window shows its real surroundings inside the block (THE WINDOW RULE,
    ``include/amyloid_yolo.h``), with ``context=False`` black, like a tile cut to disk.

    Draws.  Everything random comes from ``numpy.random.default_rng([seed, rank])``, sample after sample, batch after batch, in
    this order, every draw made whatever is switched off:
      1. ``u_slide``: the slide, with probability ``weight_i / sum(weights)``, ``weight_i = n_annotations_i + n_wanted_tiles_i``
         (annotations whose centre lies in the block; wanted tiles that intersect it);
      2. ``u_hard``, 3. ``u_object``: a hard box if the slide has one and ``u_hard < p_hard``; else an annotation if it has one and
         ``u_object < p_object``; else a wanted tile of the tissue grid (an unannotated slide falls back to tissue; a slide without
         a wanted tile to its annotations);
      4. ``u_pick``: which of them, uniformly;
      5. ``u_px``, 6. ``u_py``: for a tile pick, the point of the tile (inside the block) that is the anchor; the anchor of a box
         is its centre;
      7. ``u_jx``, 8. ``u_jy``: the jitter, so that the anchor can fall anywhere in the window: ``origin = floor(anchor) - tile + 1
         + floor(u * tile)``; then the origin is moved into ``[block_lo, block_hi - tile]``;
      9. the nine draws of ``augment.sample_params`` for the record.
    The tissue grid is ``tile_grid(H, W, tile)`` over the whole slide; its wanted tiles come from ``tile_mask`` (a bool array, or a
    list of one per slide) or from :func:`tissue_mask` with ``min_tissue`` (on the device, once per slide).

    Labels are made on the host in float64: the annotations that intersect the rectangle a sample may read (found through a grid
    index built once per slide) are clipped to the block (for ``context=False`` to the window first), written as ``class cx cy w
    h`` relative to the window (values outside 0..1 are legitimate with context) and moved by ``augment.transform_labels(...,
    min_visible=min_visible)``, the label rule of tile training.

    A host raster is staged per batch: of every sample only ``footprint ∩ block`` (``context=False``: the window) is copied into a
    pinned buffer, with the records behind the pixels, one batch ahead on a worker thread, and uploaded on a copy stream
    (``upload.Uploader``; the plan is drawn in its ``fill``); of a resident raster only the records go up, the same way.
    ``batches`` (default ``ceil(sum(weights) / batch_size)``) is ``len()``.  With ``world > 1`` every rank builds its own sampler
    with its ``rank`` and the same ``batches``.  Callables in ``hooks`` see every ``(imgs, targets)`` that leaves."""

    N_POSITION_DRAWS = 8

    def __init__(self, slides, tile=1536, img_size=1024, batch_size=32, batches=None, seed=0, rank=0, ranges=None, context=True,
                 p_object=0.5, p_hard=0.0, min_visible=0.0, tile_mask=None, min_tissue=0.01, fill=255):
        self.tile, self.S, self.B = int(tile), int(img_size), int(batch_size)
        if self.tile <= 0 or self.S <= 0 or self.B <= 0:
            raise ValueError("SlideSampler: tile, img_size and batch_size must be positive")
        if not (0.0 <= p_object <= 1.0 and 0.0 <= p_hard <= 1.0 and 0.0 <= min_visible <= 1.0 and 0.0 <= float(fill) <= 255.0):
            raise ValueError("SlideSampler: p_object, p_hard, min_visible are fractions and fill lies in 0..255")
        self.context, self.p_object, self.p_hard, self.min_visible, self.fill = bool(context), float(p_object), float(p_hard), float(min_visible), float(fill)
        self.ranges = ranges or AugmentRanges()
        self.rng = np.random.default_rng([seed, rank])
        self.hooks = []
        if not len(slides):
            raise ValueError("SlideSampler: no slides")
        masks = tile_mask if isinstance(tile_mask, (list, tuple)) else [tile_mask] * len(slides)
        if len(masks) != len(slides) or (tile_mask is not None and not isinstance(tile_mask, (list, tuple)) and len(slides) != 1):
            raise ValueError("SlideSampler: one tile_mask per slide")
        self.slides = [self._slide(item, m, min_tissue) for item, m in zip(slides, masks)]
        self.resident = self.slides[0].resident
        if any(s.resident != self.resident for s in self.slides):
            raise ValueError("SlideSampler: the rasters are either all on the host or all on the device")
        w = np.array([len(s.pickable) + len(s.wanted) for s in self.slides], dtype=np.float64)
        if w.sum() <= 0:
            raise ValueError("SlideSampler: neither an annotation nor a wanted tile inside any block")
        self._cum = np.cumsum(w) / w.sum()
        self.batches = int(batches) if batches is not None else int(math.ceil(w.sum() / self.B))
        self._up = None      # upload.Uploader, made on the first iteration

    # ---- set-up -----------------------------------------------------------------------------------------------------------------
    def _slide(self, item, mask, min_tissue):
        if isinstance(item, dict):
            raster, targets, roi, hard = item["raster"], item["targets"], item.get("roi"), item.get("hard")
        else:
            raster, targets, roi, hard = item[0], item[1], (item[2] if len(item) > 2 else None), None
        s = _Slide()
        s.raster = raster
        s.resident = isinstance(raster, torch.Tensor) and raster.is_cuda
        if s.resident:
            ok = raster.dtype == torch.uint8 and raster.dim() == 3 and raster.shape[2] == 3 and raster.stride(2) == 1 and raster.stride(1) == 3
        else:
            ok = isinstance(raster, np.ndarray) and raster.dtype == np.uint8 and raster.ndim == 3 and raster.shape[2] == 3
        if not ok:
            raise ValueError("SlideSampler: a raster is a uint8 [H,W,3] NumPy array or device tensor with packed pixels")
        H, W = int(raster.shape[0]), int(raster.shape[1])
        x1, y1, x2, y2 = (0, 0, W, H) if roi is None else (int(math.ceil(roi[0])), int(math.ceil(roi[1])), int(math.floor(roi[2])), int(math.floor(roi[3])))
        s.block = (max(x1, 0), max(y1, 0), min(x2, W), min(y2, H))
        if s.block[2] - s.block[0] < self.tile or s.block[3] - s.block[1] < self.tile:
            raise ValueError(f"SlideSampler: tile {self.tile} exceeds roi ∩ slide {s.block}")
        t = np.asarray(targets.cpu() if isinstance(targets, torch.Tensor) else targets, dtype=np.float64).reshape(-1, 5)
        s.targets = t[self._intersects(t[:, 1:], s.block)]
        s.pickable = np.flatnonzero(self._centre_inside(s.targets[:, 1:], s.block))
        h = np.zeros((0, 4)) if hard is None else np.asarray(hard.cpu() if isinstance(hard, torch.Tensor) else hard, dtype=np.float64).reshape(-1, 4)
        s.hard = h[self._centre_inside(h, s.block)]
        if mask is None:    # tissue_mask's probe: every d-th pixel, the grid of the full slide (probe_view)
            d = 16 if self.tile % 16 == 0 else 1
            view = raster[::d, ::d].cpu().numpy() if s.resident else (raster[::d, ::d] if d > 1 else raster)
            mask = wanted_tiles(tissue_counts(view, self.tile // d), self.tile // d, min_tissue)
        mask = check_tile_mask(mask, H, W, self.tile)
        ty, tx = np.nonzero(mask)
        boxes = np.stack([tx * self.tile, ty * self.tile, np.minimum((tx + 1) * self.tile, W), np.minimum((ty + 1) * self.tile, H)], 1).reshape(-1, 4)
        inter = np.stack([np.maximum(boxes[:, 0], s.block[0]), np.maximum(boxes[:, 1], s.block[1]),
                          np.minimum(boxes[:, 2], s.block[2]), np.minimum(boxes[:, 3], s.block[3])], 1)
        s.wanted = inter[(inter[:, 2] > inter[:, 0]) & (inter[:, 3] > inter[:, 1])].astype(np.int64)   # tile ∩ block, grid order
        # grid index: cell (tile x tile, from the slide's corner) -> the annotations that touch it
        s.cells = {}
        for i, (_, ax1, ay1, ax2, ay2) in enumerate(s.targets):
            for cy in range(int(ay1 // self.tile), int(ay2 // self.tile) + 1):
                for cx in range(int(ax1 // self.tile), int(ax2 // self.tile) + 1):
                    s.cells.setdefault((cy, cx), []).append(i)
        return s

    @staticmethod
    def _intersects(b, r):
        return (b[:, 2] > r[0]) & (b[:, 0] < r[2]) & (b[:, 3] > r[1]) & (b[:, 1] < r[3])

    @staticmethod
    def _centre_inside(b, r):
        cx, cy = (b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2
        return (cx >= r[0]) & (cx < r[2]) & (cy >= r[1]) & (cy < r[3])

    def __len__(self):
        return self.batches

    # ---- the host side of a batch ------------------------------------------------------------------------------------------------
    def _draw(self):
        """one sample: (slide, kind, pick, x, y) from N_POSITION_DRAWS uniform draws"""
        u_slide, u_hard, u_object, u_pick, u_px, u_py, u_jx, u_jy = self.rng.uniform(0.0, 1.0, self.N_POSITION_DRAWS)
        si = min(int(np.searchsorted(self._cum, u_slide, side="right")), len(self.slides) - 1)
        s = self.slides[si]
        index = lambda n: min(int(u_pick * n), n - 1)
        if len(s.hard) and u_hard < self.p_hard:
            kind, pick = 2, index(len(s.hard))
            b = s.hard[pick]
            ax, ay = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
        elif len(s.pickable) and (u_object < self.p_object or not len(s.wanted)):
            kind, pick = 1, int(s.pickable[index(len(s.pickable))])
            b = s.targets[pick, 1:]
            ax, ay = (b[0] + b[2]) / 2, (b[1] + b[3]) / 2
        else:
            kind, pick = 0, index(len(s.wanted))
            b = s.wanted[pick]
            ax = b[0] + min(int(u_px * (b[2] - b[0])), b[2] - b[0] - 1)
            ay = b[1] + min(int(u_py * (b[3] - b[1])), b[3] - b[1] - 1)
        T = self.tile
        jitter = lambda u: min(int(u * T), T - 1)
        x = int(math.floor(ax)) - T + 1 + jitter(u_jx)
        y = int(math.floor(ay)) - T + 1 + jitter(u_jy)
        x = min(max(x, s.block[0]), s.block[2] - T)
        y = min(max(y, s.block[1]), s.block[3] - T)
        return si, kind, pick, x, y

    def _labels(self, s, rect, x, y, rec):
        """label rows [m,5] of one sample: the slide's annotations that intersect ``rect``, cut and moved as the class docstring says"""
        T = self.tile
        ids = set()
        for cy in range(rect[1] // T, (rect[3] - 1) // T + 1):
            for cx in range(rect[0] // T, (rect[2] - 1) // T + 1):
                ids.update(s.cells.get((cy, cx), ()))
        if not ids:
            return np.zeros((0, 5))
        t = s.targets[sorted(ids)]
        t = t[self._intersects(t[:, 1:], rect)]
        lim = s.block if self.context else (max(x, s.block[0]), max(y, s.block[1]), min(x + T, s.block[2]), min(y + T, s.block[3]))
        x1, y1 = np.clip(t[:, 1], lim[0], lim[2]), np.clip(t[:, 2], lim[1], lim[3])
        x2, y2 = np.clip(t[:, 3], lim[0], lim[2]), np.clip(t[:, 4], lim[1], lim[3])
        keep = (x2 - x1 > 0) & (y2 - y1 > 0)
        rows = np.stack([t[:, 0], ((x1 + x2) / 2 - x) / T, ((y1 + y2) / 2 - y) / T, (x2 - x1) / T, (y2 - y1) / T], 1)[keep]
        return transform_labels(rows, T, T, rec, min_visible=self.min_visible)

    def plan_batch(self):
        """draws the next batch (host only, no device call) -> :class:`SlideBatchPlan`"""
        B, T = self.B, self.tile
        slide, kind, pick = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
        origins, rects = np.zeros((B, 2), np.int64), np.zeros((B, 4), np.int64)
        devs, As, rows = [], [], [np.zeros((0, 6))]
        for i in range(B):
            slide[i], kind[i], pick[i], x, y = self._draw()
            one = sample_params(self.rng, [(T, T)], self.ranges)
            devs.append(one.dev)
            As.append(one.A)
            s = self.slides[slide[i]]
            origins[i] = x, y
            if self.context:
                f = footprint(one[0], T, self.S)
                seen = max(f[0] + x, s.block[0]), max(f[1] + y, s.block[1]), min(f[2] + x, s.block[2]), min(f[3] + y, s.block[3])
            else:
                seen = x, y, x + T, y + T
            if seen[2] <= seen[0] or seen[3] <= seen[1]:
                seen = x, y, x, y                                               # nothing to read: a block without pixels
                b = np.zeros((0, 5))
            else:
                b = self._labels(s, seen, x, y, one[0])
            rects[i] = s.block if self.resident else seen
            rows.append(np.concatenate([np.full((len(b), 1), float(i)), b], 1))
        return SlideBatchPlan(slide, kind, pick, origins, AugTable(np.concatenate(devs), np.concatenate(As)), rects, np.concatenate(rows, 0))

    def staged_bytes(self, plan):
        """bytes of pixels ``stage`` copies for this plan (0 for resident rasters)"""
        r = plan.rects
        return 0 if self.resident else int(((r[:, 2] - r[:, 0]) * (r[:, 3] - r[:, 1]) * 3).sum())

    def window_table(self, plan, base=0):
        """The plan's window records (``augment.WindowTable``).  Host rasters: the staged sub-blocks lie one after another, rows
        ``3 * bw`` bytes apart; resident rasters: the records point into the rasters, ``src_offset`` counted from address ``base``."""
        r, o = plan.rects, plan.origins
        blocks = [(int(b[3] - b[1]), int(b[2] - b[0])) for b in r]
        orig = [(int(o[i, 0] - r[i, 0]), int(o[i, 1] - r[i, 1])) for i in range(len(r))]
        if not self.resident:
            return make_window_table(plan.table, blocks, orig, self.context, self.fill)
        offs, strides = [], []
        for i, si in enumerate(plan.slide):
            ras = self.slides[si].raster
            strides.append(int(ras.stride(0)))
            offs.append(ras.data_ptr() - base + int(r[i, 1]) * int(ras.stride(0)) + int(r[i, 0]) * 3)
        return make_window_table(plan.table, blocks, orig, self.context, self.fill, offs, strides)

    def stage(self, plan, table, dst, pool=None):
        """copies the plan's sub-blocks of the host rasters into ``dst`` (a flat uint8 NumPy array of at least ``staged_bytes``) at
        the records' offsets"""
        def one(i):
            x1, y1, x2, y2 = (int(v) for v in plan.rects[i])
            if x2 > x1 and y2 > y1:
                off = int(table.dev[i]["src_offset"])
                np.copyto(dst[off:off + (y2 - y1) * (x2 - x1) * 3].reshape(y2 - y1, x2 - x1, 3), self.slides[plan.slide[i]].raster[y1:y2, x1:x2])
        list(pool.map(one, range(len(plan.rects)))) if pool is not None else [one(i) for i in range(len(plan.rects))]

    # ---- the device side -----------------------------------------------------------------------------------------------------------
    def _resident_span(self):
        lo = min(s.raster.data_ptr() for s in self.slides)
        hi = max(s.raster.data_ptr() + (s.raster.shape[0] - 1) * s.raster.stride(0) + s.raster.shape[1] * 3 for s in self.slides)
        return lo, hi - lo

    def __iter__(self):
        dev = hip_device("SlideSampler has")
        if self._up is None:
            self._up = Uploader(dev)
        base, span = self._resident_span() if self.resident else (0, 0)

        def fill(idx, host):
            """on the staging thread: plan the batch and write the pixels (host rasters only) and, behind them, the records"""
            plan = self.plan_batch()
            table = self.window_table(plan, base)
            n = 0 if self.resident else max(self.staged_bytes(plan), 1)
            rec = table.dev.view(np.uint8).reshape(-1)
            buf = host(record_offset(n) + rec.size)
            if not self.resident:
                self.stage(plan, table, buf, self._up.pool)
            tab = pack_records(buf, n, rec)
            return (plan, n, tab), tab + rec.size

        for k, (plan, n, tab), buf, _ in self._up.run(self.batches, fill):     # staged while the consumer's training step runs
            out = torch.empty(self.B, 3, self.S, self.S, device=dev, dtype=torch.float32)
            src = (base, span) if self.resident else (buf.data_ptr(), n)
            launch_windows(*src, buf.data_ptr() + tab, self.B, self.S, out)
            self._up.release(k)
            targets = torch.from_numpy(plan.targets).float().to(dev)
            for hook in self.hooks:
                hook(out, targets)
            yield out, targets
