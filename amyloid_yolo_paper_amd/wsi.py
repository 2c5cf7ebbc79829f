"""WSI -> tile streaming: detection over a whole-slide raster without the disk round trip of the
reference (``crop.py:13-25`` writes 1536-px JPEG tiles with pyvips ``dzsave``, ``detect.py:59-105`` reads them back).

A slide (any ``[H, W, 3]`` uint8 array: a NumPy memmap of a decoded level, a pyvips/openslide region fetched by the caller)
is walked in full-width strips of one tile row.  A strip is one contiguous slice of the raster: it goes to the device in a
single copy from a pinned staging buffer on a copy stream (two buffers, so strip i+1 uploads while strip i computes), and
``ay_ingest_region_tiles_u8`` cuts the row of tiles out of it on the device -- dzsave's 'google' layout: a ``tile`` grid from
the top-left corner, edge tiles padded with the background 255 -- with the optional 40x -> 20x halving (``crop.py:44-47``)
and the detect-time ``/255`` + nearest resize fused in.  Detections come back in slide coordinates.

Abutting tiles split every object that straddles a seam.  With ``overlap > 0`` the tile origins are ``tile - overlap`` apart
(:func:`tile_grid`, ``ay_ingest_region_tiles_step_u8``), every object no larger than ``overlap`` is seen whole by at least one
tile, the per-tile detections stay on the device (``utils.nms_device`` -> ``ay_seam_append``) and one slide-level pass removes
the second sightings (``ay_seam_merge``; the rule is stated in ``include/amyloid_yolo.h``).

Most of a histology slide is glass.  :func:`tissue_counts` (``ay_tile_tissue_u8``, the rule in ``include/amyloid_yolo.h``) counts the
tissue pixels of every tile, usually on a low-resolution level, :func:`wanted_tiles` turns the counts into a ``tile_mask``, and with
a mask the stream never stages a strip without a wanted tile, stages of any other strip only the columns between its first and its
last wanted tile and cuts only the wanted tiles out of it (``ay_ingest_region_tiles_list_u8``); :func:`detect_region` then fills its
batches with wanted tiles across strip boundaries.

No CPU fallback: the product path needs the HIP library and a GPU."""
import ctypes as C
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .utils import nms_device, non_max_suppression
from .views import check_views, nms_views_device


def tile_grid(H, W, tile, overlap=0):
    """Tile grid over an ``H x W`` (halved, for ``shrink=2``) slide -> ``(tiles_y, tiles_x, step)``.

    ``step = tile - overlap`` with ``0 <= overlap < tile``; tile ``(ty, tx)`` has its origin at ``(ty * step, tx * step)`` and a
    side of ``tile``; per axis ``max(1, ceil((extent - overlap) / step))`` tiles cover the slide, and none of them lies entirely
    inside its predecessor.  ``overlap=0`` is dzsave's 'google' grid, ``ceil(extent / tile)``."""
    tile, overlap = int(tile), int(overlap)
    if tile <= 0 or not 0 <= overlap < tile:
        raise ValueError(f"tile_grid: need tile > 0 and 0 <= overlap < tile (tile {tile}, overlap {overlap})")
    step = tile - overlap
    n = lambda extent: max(1, -(-(int(extent) - overlap) // step))
    return n(H), n(W), step


def wanted_tiles(counts, tile, min_tissue):
    """Tissue counts ``[tiles_y, tiles_x]`` (:func:`tissue_counts`) -> bool mask of the tiles worth reading: a tile is wanted iff
    ``count >= max(1, ceil(min_tissue * tile * tile))`` (``include/amyloid_yolo.h``, THE TISSUE RULE).  ``tile`` is the tile side on
    the raster that was counted (for a probe level, the divided one); ``min_tissue=0`` keeps every tile with a tissue pixel."""
    if not 0.0 <= float(min_tissue) <= 1.0:
        raise ValueError(f"wanted_tiles: min_tissue {min_tissue} is no fraction of a tile")
    need = max(1, math.ceil(float(min_tissue) * int(tile) * int(tile)))
    return np.asarray(counts) >= need


def check_tile_mask(tile_mask, H, W, tile, overlap=0):
    """``tile_mask`` for the ``tile_grid(H, W, tile, overlap)`` grid: a NumPy bool array ``[tiles_y, tiles_x]``, else ``ValueError``"""
    ty, tx, _ = tile_grid(H, W, tile, overlap)
    if not isinstance(tile_mask, np.ndarray) or tile_mask.dtype != np.bool_ or tile_mask.shape != (ty, tx):
        raise ValueError(f"tile_mask: need a NumPy bool array of shape ({ty}, {tx}), got "
                         f"{getattr(tile_mask, 'dtype', type(tile_mask).__name__)} {getattr(tile_mask, 'shape', '')}")
    return tile_mask


def probe_view(raster, tile, shrink=1, overlap=0, probe_stride=16):
    """The low-resolution stand-in of a raster that has no pyramid level at hand: every ``probe_stride``-th pixel of the (halved)
    slide -> ``(view, tile // d, overlap // d)``.  The view takes SINGLE source pixels (``raster[0:shrink*H:shrink*d,
    0:shrink*W:shrink*d]``, no 2x2 mean, no averaging over the stride) and copies nothing.  ``d`` must divide ``tile`` and ``tile -
    overlap`` (``ValueError``); the probe grid then has the shape of the full grid."""
    d, tile, overlap = int(probe_stride), int(tile), int(overlap)
    if d < 1 or tile % d or (tile - overlap) % d:
        raise ValueError(f"probe_stride {d} must divide tile {tile} and tile - overlap {tile - overlap}")
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    view = raster[0:shrink * H:shrink * d, 0:shrink * W:shrink * d]
    # ceil(ceil(x) / s) == ceil(x / s): the strided extents give the full grid's tile counts
    assert tile_grid(view.shape[0], view.shape[1], tile // d, overlap // d)[:2] == tile_grid(H, W, tile, overlap)[:2]
    return view, tile // d, overlap // d


class RegionTileStream:
    """Iterates over the tile rows of ``raster`` and yields ``(tiles [n,3,S,S] float32 on the device, [(ty, tx), ...])``.

    ``tile`` is the tile side on the (halved, if ``shrink`` == 2) slide, ``img_size`` the network input side.  With ``overlap``
    (pixels of the halved slide, like ``tile``) strip ``j`` holds slide rows ``[j * step, j * step + tile)``, ``step = tile -
    overlap``: consecutive strips share ``overlap`` rows, which are uploaded with both.

    ``tile_mask`` (NumPy bool ``[tiles_y, tiles_x]``, e.g. from :func:`wanted_tiles`; default: every tile): a strip without a wanted
    tile is not staged, not uploaded and yields nothing; of any other strip only the columns from its first to its last wanted tile
    are staged and uploaded (one contiguous block), and only its wanted tiles are cut and yielded, in grid order, with their
    coordinates on the full grid.

    ``views`` (default ``(0,)``: the tile as it lies on the slide): a list of distinct dihedral view ids 0..7 (``views.py``, THE VIEW
    RULE in ``include/amyloid_yolo.h``).  With any other list every tile is cut in each of the ``V`` views by
    ``ay_ingest_region_tiles_views_u8`` -- the strip is read once for all of them -- and a strip yields ``[n * V, 3, S, S]``,
    tile-major (tile ``i`` in view ``views[j]`` is image ``i * V + j``), with the coordinates of the ``n`` tiles."""

    def __init__(self, raster, tile=1536, img_size=1024, shrink=1, overlap=0, tile_mask=None, views=(0,)):
        self.views = check_views(views)
        if not torch.cuda.is_available():
            raise _lib.AyError("no HIP device: RegionTileStream has no CPU fallback")
        assert raster.ndim == 3 and raster.shape[2] == 3 and raster.dtype == np.uint8, "uint8 [H,W,3] raster"
        assert shrink in (1, 2)
        self.raster, self.tile, self.S, self.shrink = raster, int(tile), int(img_size), int(shrink)
        H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
        self.overlap = int(overlap)
        self.tiles_y, self.tiles_x, self.step = tile_grid(H, W, self.tile, self.overlap)
        self.tile_mask = None if tile_mask is None else check_tile_mask(tile_mask, H, W, self.tile, self.overlap)
        self._jobs = self._strip_jobs()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        rows = self.tile * shrink
        self._pinned = [torch.empty(rows, raster.shape[1], 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._strips = [torch.empty(rows, raster.shape[1], 3, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self._copy = torch.cuda.Stream(device=self.dev)
        self._pool = ThreadPoolExecutor(max_workers=4)      # row chunks of one staging copy
        self._stager = ThreadPoolExecutor(max_workers=1)    # one strip ahead of the consumer
        self._chunk = -(-rows // 4)
        self._uploaded = [None, None]   # event: strip landed in _strips[k]
        self._consumed = [None, None]   # event: every ingest kernel that read _strips[k] is done

    def _strip_jobs(self):
        """the strips that are staged: ``[(j, c0, c1)]`` = tile row and its span of SOURCE columns ``[c0, c1)`` (computed once)"""
        if self.tile_mask is None:
            return [(j, 0, self.raster.shape[1]) for j in range(self.tiles_y)]
        W, out = self.raster.shape[1] // self.shrink, []
        for j in range(self.tiles_y):
            txs = np.flatnonzero(self.tile_mask[j])
            if len(txs):
                out.append((j, int(txs[0]) * self.step * self.shrink, min(int(txs[-1]) * self.step + self.tile, W) * self.shrink))
        return out

    def _staged_bytes(self):
        """bytes of the raster that one pass stages and uploads"""
        rows, first = self.tile * self.shrink, self.step * self.shrink
        return sum(len(range(j * first, min(j * first + rows, self.raster.shape[0]))) * (c1 - c0) * 3 for j, c0, c1 in self._jobs)

    def __len__(self):
        """the number of strips the iteration yields: ``tiles_y`` without a mask, the tile rows that hold a wanted tile with one"""
        return len(self._jobs)

    def _stage(self, idx, job):
        """host side of a strip: raster rows (the job's columns) -> pinned buffer, as one contiguous block with rows ``3 * width``
        bytes apart (runs on the staging thread, under the consumer's GPU work) -> (rows, width) of the block"""
        k = idx & 1
        j, c0, c1 = job
        rows = self.tile * self.shrink
        first = j * self.step * self.shrink
        src = self.raster[first:first + rows, c0:c1]
        n, w = src.shape[0], src.shape[1]
        if self._uploaded[k] is not None:
            self._uploaded[k].synchronize()      # the host buffer is free again once its last copy has run
        # staging copy by NumPy (memcpy speed; torch's uint8 copy_ ran at a quarter of it), rows split over a few threads --
        # the copy releases the GIL -- so that one strip stages faster than the GPU consumes it
        dst = self._pinned[k].numpy().reshape(-1)[:n * w * 3].reshape(n, w, 3)
        parts = [(a, min(a + self._chunk, n)) for a in range(0, n, self._chunk)]
        list(self._pool.map(lambda ab: np.copyto(dst[ab[0]:ab[1]], src[ab[0]:ab[1]]), parts))
        return n, w

    def _copy_to_device(self, idx, nbytes):
        k = idx & 1
        if self._consumed[k] is not None:
            self._copy.wait_event(self._consumed[k])
        with torch.cuda.stream(self._copy):
            self._strips[k].view(-1)[:nbytes].copy_(self._pinned[k].view(-1)[:nbytes], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy)
        self._uploaded[k] = ev

    def _strip_loop(self):
        """The strip machinery every user shares: stage (one strip ahead, on the staging thread), pinned upload on the copy stream,
        two buffers.  Yields ``(j, k, rows, width)`` once the current stream waits for the upload of tile row ``j`` into
        ``_strips[k]``: a ``rows x width`` block of source pixels, rows ``3 * width`` bytes apart.  The user issues every kernel that
        reads the block on the current stream and then calls ``_release(k)``; the buffer is refilled only behind that point."""
        jobs = self._jobs
        main = torch.cuda.current_stream()
        dev_index = self.dev.index

        def stage(idx):
            torch.cuda.set_device(dev_index)
            return self._stage(idx, jobs[idx])

        fut = self._stager.submit(stage, 0) if jobs else None
        for idx, (j, _, _) in enumerate(jobs):
            k = idx & 1
            n, w = fut.result()
            self._copy_to_device(idx, n * w * 3)
            if idx + 1 < len(jobs):  # staged while the consumer's model + NMS of this strip run
                fut = self._stager.submit(stage, idx + 1)
            main.wait_event(self._uploaded[k])
            yield j, k, n, w

    def _release(self, k):
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream())
        self._consumed[k] = done

    def _wanted(self):
        """``[(ty, tx)]`` of the tiles the stream yields, in grid order"""
        if self.tile_mask is None:
            return [(j, i) for j in range(self.tiles_y) for i in range(self.tiles_x)]
        return [(int(j), int(i)) for j, i in zip(*np.nonzero(self.tile_mask))]

    def _wanted_table(self):
        """for the list ingest, on the device: the origin of every wanted tile inside its strip's block, int32 [n][2] = (x, 0) in
        grid order, and per tile row the index of its first wanted tile (host)"""
        span0 = {j: c0 // self.shrink for j, c0, _ in self._jobs}
        xy = np.array([(i * self.step - span0[j], 0) for j, i in self._wanted()], np.int32).reshape(-1, 2)
        starts = np.r_[0, np.cumsum(self.tile_mask.sum(1))]
        return torch.from_numpy(xy).to(self.dev), starts

    def _ingest_list(self, L, k, n, w, origins, m, out):
        """tiles ``origins[:m]`` of the block in ``_strips[k]`` -> ``out[:m * V]``, every tile in the stream's views"""
        if self.views != (0,):
            ids = (C.c_int * len(self.views))(*self.views)
            check(L.ay_ingest_region_tiles_views_u8(ptr(self._strips[k]), n, w, w * 3, self.shrink, self.tile, ptr(origins), m, ids,
                                                    len(ids), self.S, ptr(out), _lib.stream_ptr()), "ay_ingest_region_tiles_views_u8")
            return
        check(L.ay_ingest_region_tiles_list_u8(ptr(self._strips[k]), n, w, w * 3, self.shrink, self.tile, ptr(origins), m, self.S,
                                               ptr(out), _lib.stream_ptr()), "ay_ingest_region_tiles_list_u8")

    def __iter__(self):
        L = _lib.lib()
        V = len(self.views)
        if self.tile_mask is not None:
            table, starts = self._wanted_table()
            coords = self._wanted()
        elif self.views != (0,):     # the views entry takes a list of origins: those of a full tile row
            row = torch.tensor([(i * self.step, 0) for i in range(self.tiles_x)], dtype=torch.int32, device=self.dev)
        for j, k, valid, width in self._strip_loop():
            if self.tile_mask is None:
                out = torch.empty(self.tiles_x * V, 3, self.S, self.S, device=self.dev, dtype=torch.float32)
                if self.views != (0,):
                    self._ingest_list(L, k, valid, width, row, self.tiles_x, out)
                elif self.overlap == 0:
                    check(L.ay_ingest_region_tiles_u8(ptr(self._strips[k]), valid, width, width * 3, self.shrink, self.tile, 1,
                                                      self.tiles_x, self.S, ptr(out), _lib.stream_ptr()), "ay_ingest_region_tiles_u8")
                else:
                    check(L.ay_ingest_region_tiles_step_u8(ptr(self._strips[k]), valid, width, width * 3, self.shrink, self.tile,
                                                           self.step, 1, self.tiles_x, self.S, ptr(out), _lib.stream_ptr()),
                          "ay_ingest_region_tiles_step_u8")
                self._release(k)
                yield out, [(j, i) for i in range(self.tiles_x)]
            else:
                a, b = int(starts[j]), int(starts[j + 1])
                out = torch.empty((b - a) * V, 3, self.S, self.S, device=self.dev, dtype=torch.float32)
                self._ingest_list(L, k, valid, width, table[a:], b - a, out)
                self._release(k)
                yield out, coords[a:b]

    def _batches(self, batch_size):
        """The masked iteration as detect_region takes it: yields ``(tiles [n * V,3,S,S], w0)``, the wanted tiles ``w0 .. w0 + n`` of
        :meth:`_wanted`, ``n == batch_size`` but for the last batch: a strip's wanted tiles are cut into the open batch buffer at its
        fill, so that batches are filled across strip boundaries.  Every ingest of a strip is issued (into as many batch buffers as
        it takes) and the strip released before its batches are handed out, so the refill of a strip buffer never waits for a model
        call, also when a batch holds tiles of two strips."""
        L = _lib.lib()
        table, starts = self._wanted_table()
        V = len(self.views)
        cur, fill, w0 = None, 0, 0
        for j, k, valid, width in self._strip_loop():
            a, b = int(starts[j]), int(starts[j + 1])
            ready = []
            while a < b:
                if cur is None:
                    cur, fill, w0 = torch.empty(batch_size * V, 3, self.S, self.S, device=self.dev, dtype=torch.float32), 0, a
                m = min(b - a, batch_size - fill)
                self._ingest_list(L, k, valid, width, table[a:], m, cur[fill * V:])
                fill, a = fill + m, a + m
                if fill == batch_size:
                    ready.append((cur, w0))
                    cur = None
            self._release(k)
            yield from ready
        if cur is not None:
            yield cur[:fill * V], w0


def tissue_counts(raster, tile, shrink=1, overlap=0, bg_level=220):
    """Tissue pixels per tile of the ``tile_grid(H, W, tile, overlap)`` grid over ``raster`` -> NumPy int32 ``[tiles_y, tiles_x]``.

    A pixel of the (halved, for ``shrink=2``: the ingest's 2x2 round-half-up means) slide is tissue iff ``min(R, G, B) < bg_level``
    (``bg_level`` in 0 .. 256; the default suits scanned glass); pixels of a shared band count for every tile that holds them, the
    padding outside the slide never counts (THE TISSUE RULE in ``include/amyloid_yolo.h``, ``ay_tile_tissue_u8``).  The raster goes
    through the strips of :class:`RegionTileStream` once and the counts come back in one read.  Meant for a low-resolution level
    of the slide, with ``tile`` and ``overlap`` divided by that level's downsample (any ``[H, W, 3]`` uint8 array, strided views
    such as :func:`probe_view`'s included), and exact on any raster: on the full one it costs a full upload of the slide.  A strip
    reaches the kernel with rows ``3 * width`` bytes apart: the kernel's 16-byte loads need that to be a multiple of 16 (a width
    that is a multiple of 16 pixels) and fall back to byte loads otherwise, about three times slower on the device and the same
    counts; on a low-resolution level either is small against the staging copy."""
    bg_level = int(bg_level)
    if not 0 <= bg_level <= 256:
        raise ValueError(f"tissue_counts: bg_level {bg_level} outside 0 .. 256")
    stream = RegionTileStream(raster, tile, tile, shrink, overlap)
    L = _lib.lib()
    counts = torch.empty(stream.tiles_y, stream.tiles_x, device=stream.dev, dtype=torch.int32)
    for j, k, valid, width in stream._strip_loop():
        check(L.ay_tile_tissue_u8(ptr(stream._strips[k]), valid, width, width * 3, stream.shrink, stream.tile, stream.step, 1,
                                  stream.tiles_x, bg_level, ptr(counts[j]), _lib.stream_ptr()), "ay_tile_tissue_u8")
        stream._release(k)
    return counts.cpu().numpy()


def tissue_mask(raster, tile, shrink=1, overlap=0, min_tissue=0.01, bg_level=220, probe_stride=16):
    """The ``tile_mask`` of ``detect_region(min_tissue > 0)``: ``wanted_tiles`` of the tissue counts of :func:`probe_view`
    (``probe_stride=1``: of the raster itself, the exact rule including the 2x2 means, at the cost of a full upload of the slide)."""
    if int(probe_stride) == 1:
        return wanted_tiles(tissue_counts(raster, tile, shrink, overlap, bg_level), tile, min_tissue)
    view, t, o = probe_view(raster, tile, shrink, overlap, probe_stride)
    return wanted_tiles(tissue_counts(view, t, 1, o, bg_level), t, min_tissue)


def detect_region(model, raster, tile=1536, img_size=1024, shrink=1, conf_thres=0.8, nms_thres=0.4, batch_size=64, overlap=0,
                  seam_thres=0.5, max_det=1024, seam_capacity=None, tile_mask=None, min_tissue=0.0, bg_level=220, probe_stride=16,
                  views=(0,), min_views=1, vote_thres=None):
    """Detection over a whole raster: the loop of ``detect.py:88-105`` fed by :class:`RegionTileStream`.

    Returns a list of ``(ty, tx, boxes)`` with ``boxes [n,7]`` = (x1, y1, x2, y2, conf, cls_conf, cls_pred) in pixels of the
    (halved) slide -- the tile-local boxes of ``non_max_suppression`` scaled from the network size back to the tile
    (``rescale_boxes`` of a square tile is a pure scale) and shifted by the tile origin -- tiles without detections omitted.

    ``overlap`` (pixels of the halved slide, like ``tile``; default 0 = abutting tiles, the reference's grid) makes neighbouring
    tiles share a band of that width, so that an object on a seam is seen whole by at least one tile, and removes the second
    sightings with the slide-level seam merge: of two rows of one class from DIFFERENT tiles whose intersection covers more than
    ``seam_thres`` of the smaller box, the one with the lower ``conf * cls_conf`` goes (exact greedy order, rule in
    ``include/amyloid_yolo.h``); rows are only selected, never altered.  Choose ``overlap`` at least as large as the side of the
    largest object that must not be split (for 50-px plaques on 1536-px tiles, 64 or 128); the cost is ``(tile / (tile -
    overlap))**2`` times the tiles.  On this path nothing is read back per batch: per tile at most ``max_det`` rows are kept on the
    device (a tile with more raises ``AyError`` at the end), in a slide buffer of ``seam_capacity`` rows (default: all tiles
    full, at most 4 M rows).  The result has the same form: tiles in grid order, rows of a tile in NMS output order, tiles left
    without a row omitted.

    ``tile_mask`` (NumPy bool ``[tiles_y, tiles_x]`` of the ``tile_grid``; default: every tile) names the tiles worth reading:
    the others are neither staged nor uploaded nor run (see :class:`RegionTileStream`), batches of ``batch_size`` wanted tiles are
    filled across strip boundaries, and the result is that of the full run restricted to the wanted tiles (``(ty, tx)`` and boxes
    on the full grid; with ``overlap`` the seam merge sees no rows of unwanted tiles).  An all-False mask returns ``[]``.
    ``min_tissue > 0`` without a mask is the one-call form: the mask is ``tissue_mask(raster, tile, shrink, overlap, min_tissue,
    bg_level, probe_stride)``, i.e. tiles with at least that fraction of tissue pixels (``min(R, G, B) < bg_level``) on a probe
    that takes every ``probe_stride``-th pixel of the (halved) slide -- single source pixels, no averaging, so an object smaller
    than ``probe_stride`` pixels that is alone in its tile can be missed; ``probe_stride`` must divide ``tile`` and ``tile -
    overlap``.  ``probe_stride=1`` counts on the raster itself (exact, and a full upload of the slide before the detection pass).

    ``views`` (default ``(0,)``; ``views.ALL_VIEWS``, ``views.FLIPS`` or any list of distinct ids 0..7) is test-time augmentation
    over the orientations of the square: every tile is cut in each of the ``V`` views on the device (one read of the strip for all of
    them, THE VIEW RULE in ``include/amyloid_yolo.h``), the network runs on all of them, the boxes are mapped back to the tile's
    frame (exact in fp32) and the rows of all views of a tile go through ONE merge-NMS, so a sighting that several views share comes
    out once, with the confidence-weighted box of its cluster.  ``min_views > 1`` (at most ``V``) then keeps a detection only if at
    least that many views hold a row of its class above ``conf_thres`` whose IoU with it exceeds ``vote_thres`` (default:
    ``nms_thres``; THE VOTE RULE).  Cost: ``V`` times the network (a model call takes ``max(1, batch_size // V)`` tiles, at most
    ``batch_size`` images; the ingest and the post-processing stay small against it), and on both paths at most ``max_det``
    detections per tile (``AyError`` beyond).  What the votes can do: remove rows that only a few orientations report, which for an
    orientation-free object are mostly false alarms.  What they cannot do: they never add a detection, they do not re-score or move
    a box, and an error the network makes in every orientation gets every vote.  The views only agree as far as the model is
    equivariant: for a model that is not (one trained without ``augment=True``), the merged boxes and the votes depend on which
    views are listed and on their order only through the rows the network returns -- the same list always gives the same bytes,
    another list may give another result.  With the defaults nothing of this is called and the result is unchanged, bit for bit."""
    views = check_views(views)
    if isinstance(min_views, bool) or int(min_views) != min_views or not 1 <= int(min_views) <= len(views):
        raise ValueError(f"detect_region: min_views {min_views!r} outside 1 .. {len(views)} (the number of views)")
    if vote_thres is not None and not 0.0 <= float(vote_thres) <= 1.0:      # a NaN fails both comparisons
        raise ValueError(f"detect_region: vote_thres {vote_thres!r} is no IoU in 0 .. 1")
    tta = None if views == (0,) and int(min_views) == 1 else (views, int(min_views), vote_thres)
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    if tile_mask is None and min_tissue > 0:
        tile_mask = tissue_mask(raster, tile, shrink, overlap, min_tissue, bg_level, probe_stride)
    if tile_mask is not None and not check_tile_mask(tile_mask, H, W, tile, overlap).any():
        return []
    if overlap:
        return _detect_region_overlap(model, raster, tile, img_size, shrink, conf_thres, nms_thres, batch_size, overlap, seam_thres,
                                      max_det, seam_capacity, tile_mask, tta)
    if tta is not None:
        return _detect_region_views(model, raster, tile, img_size, shrink, conf_thres, nms_thres, batch_size, max_det, tile_mask, tta)
    results = []
    scale = float(tile) / float(img_size)
    model.eval()

    def run(tiles, coords):
        with torch.no_grad():  # rows stay on the device; only the detections come back
            det = non_max_suppression(model.forward_device(tiles), conf_thres, nms_thres)
        for (ty, tx), d in zip(coords, det):
            if d is None:
                continue
            d = d.cpu()
            d[:, :4] *= scale
            d[:, [0, 2]] += tx * tile
            d[:, [1, 3]] += ty * tile
            results.append((ty, tx, d))

    stream = RegionTileStream(raster, tile, img_size, shrink, tile_mask=tile_mask)
    if tile_mask is None:
        for tiles, coords in stream:
            for s in range(0, tiles.shape[0], batch_size):
                run(tiles[s:s + batch_size], coords[s:s + batch_size])
    else:
        coords = stream._wanted()
        for tiles, w0 in stream._batches(batch_size):
            run(tiles, coords[w0:w0 + tiles.shape[0]])
    return results


def _detect_region_views(model, raster, tile, img_size, shrink, conf_thres, nms_thres, batch_size, max_det, tile_mask, tta):
    """the abutting path with views: per model call ``max(1, batch_size // V)`` tiles in V views, ``nms_views_device``, and the rows of
    the batch read back -- the arithmetic on them is that of the path without views"""
    views, min_views, vote_thres = tta
    V, max_det = len(views), int(max_det)
    per_call = max(1, int(batch_size) // V)
    results = []
    scale = float(tile) / float(img_size)
    model.eval()

    def run(tiles, coords):
        with torch.no_grad():
            rows, _, count, _ = nms_views_device(model.forward_device(tiles), views, conf_thres, nms_thres, max_det, min_views,
                                                 vote_thres, img_dim=img_size)
            count_h, rows_h = count.cpu().tolist(), rows.cpu()
        if max(count_h) > max_det:
            raise _lib.AyError(f"detect_region: a tile holds more than max_det={max_det} detections; raise max_det or conf_thres")
        for (ty, tx), n, d in zip(coords, count_h, rows_h):
            if n == 0:
                continue
            d = d[:n].clone()
            d[:, :4] *= scale
            d[:, [0, 2]] += tx * tile
            d[:, [1, 3]] += ty * tile
            results.append((ty, tx, d))

    stream = RegionTileStream(raster, tile, img_size, shrink, tile_mask=tile_mask, views=views)
    if tile_mask is None:
        for tiles, coords in stream:
            for s in range(0, len(coords), per_call):
                run(tiles[s * V:(s + per_call) * V], coords[s:s + per_call])
    else:
        coords = stream._wanted()
        for tiles, w0 in stream._batches(per_call):
            run(tiles, coords[w0:w0 + tiles.shape[0] // V])
    return results


def _detect_region_overlap(model, raster, tile, img_size, shrink, conf_thres, nms_thres, batch_size, overlap, seam_thres, max_det,
                           seam_capacity, tile_mask=None, tta=None):
    from .postprocess import seam_merge_device
    L = _lib.lib()
    views, min_views, vote_thres = tta if tta is not None else ((0,), 1, None)
    V = len(views)
    if tta is not None:
        batch_size = max(1, int(batch_size) // V)     # tiles per model call: at most batch_size images
    stream = RegionTileStream(raster, tile, img_size, shrink, overlap, tile_mask, views)
    dev, TX, step = stream.dev, stream.tiles_x, stream.step
    # per tile that runs, on the device for the whole slide: its id (grid order on the full grid) and the (x, y) of its corner
    if tile_mask is None:
        ids = torch.arange(stream.tiles_y * TX, dtype=torch.int32)
    else:
        ids = torch.from_numpy(np.flatnonzero(tile_mask.ravel()).astype(np.int32))
    capacity = int(seam_capacity) if seam_capacity else min(len(ids) * int(max_det), 1 << 22)
    origins = torch.stack([(ids % TX) * step, (ids // TX) * step], 1).to(torch.float32).to(dev)
    ids = ids.to(dev)
    slide_rows = torch.empty(capacity, 7, device=dev, dtype=torch.float32)
    slide_tile = torch.empty(capacity, device=dev, dtype=torch.int32)
    slide_count = torch.zeros(2, device=dev, dtype=torch.int32)
    scale = C.c_float(float(tile) / float(img_size))
    model.eval()

    def batches():   # (tiles [n * V ...], index of the first of the n in ids / origins)
        if tile_mask is not None:
            yield from stream._batches(batch_size)
            return
        for tiles, coords in stream:
            for s in range(0, len(coords), batch_size):
                yield tiles[s * V:(s + batch_size) * V], coords[s][0] * TX + coords[s][1]

    for tiles, t0 in batches():
        with torch.no_grad():  # no read-back: the NMS result buffers are overwritten by the next batch, the append is right behind
            if tta is None:
                rows, _, count, _ = nms_device(model.forward_device(tiles), conf_thres, nms_thres, int(max_det))
            else:             # rows and count in nms_device's form, one image per TILE
                rows, _, count, _ = nms_views_device(model.forward_device(tiles), views, conf_thres, nms_thres, int(max_det), min_views,
                                                     vote_thres, img_dim=img_size)
        B = rows.shape[0]
        check(L.ay_seam_append(ptr(rows), ptr(count), B, int(max_det), scale, ptr(origins[t0:t0 + B]), ptr(ids[t0:t0 + B]),
                               ptr(slide_rows), ptr(slide_tile), ptr(slide_count), capacity, _lib.stream_ptr()), "ay_seam_append")
    M, flags = (int(v) for v in slide_count.cpu())
    if flags & 1:
        raise _lib.AyError(f"detect_region: a tile holds more than max_det={max_det} detections; raise max_det or conf_thres")
    if flags & 2:
        raise _lib.AyError(f"detect_region: more than seam_capacity={capacity} detections on the slide; raise seam_capacity")
    if M == 0:
        return []
    keep = seam_merge_device(slide_rows[:M], slide_tile[:M], seam_thres)
    kept, kept_tile = slide_rows[:M][keep].cpu(), slide_tile[:M][keep].cpu().numpy()
    # rows were appended in tile order: every tile is one run
    starts = np.flatnonzero(np.r_[True, kept_tile[1:] != kept_tile[:-1]])
    ends = np.r_[starts[1:], len(kept_tile)]
    return [(int(kept_tile[a]) // TX, int(kept_tile[a]) % TX, kept[a:b].clone()) for a, b in zip(starts, ends)]


def evaluate_region(model, raster, targets, iou_thres=0.5, roi=None, **detect_region_kwargs):
    """Slide-level precision / recall / AP of :func:`detect_region` against the annotations of the slide.

    Runs ``detect_region(model, raster, **detect_region_kwargs)`` unchanged, concatenates its ``(ty, tx, boxes)`` result in that
    order into ``rows`` [M,7] and returns ``stats.slide_statistics(rows, targets, iou_thres, roi)`` with ``rows`` added to the
    dict.  ``targets`` [T,5] = (class, x1, y1, x2, y2) are in pixels of the (halved) slide, like the boxes ``detect_region``
    returns; ``roi`` = (x1, y1, x2, y2) restricts the evaluation to the annotated part of the slide (rows and targets whose centre
    lies outside are ignored).  The slide is ONE image: an annotation on a tile seam stays one target (cutting the annotations
    back into tiles would make it two truncated ones), and there is no cap on their number (THE SLIDE MATCH RULE,
    ``include/amyloid_yolo.h``).

    What the number is for: comparing settings of ``overlap`` / ``seam_thres``, ``views`` / ``min_views`` / ``vote_thres``,
    ``min_tissue`` and ``conf_thres`` on an annotated slide -- each of them changes which rows come out, and this says whether the
    change helped.  ``missed`` and ``false_alarms`` index ``targets`` and ``rows`` for a look at the cases themselves."""
    from .stats import slide_statistics
    res = detect_region(model, raster, **detect_region_kwargs)
    rows = torch.cat([d for _, _, d in res]) if res else torch.zeros(0, 7)
    out = slide_statistics(rows, targets, iou_thres, roi)
    out["rows"] = rows
    return out
