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

No CPU fallback: the product path needs the HIP library and a GPU."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .utils import nms_device, non_max_suppression


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


class RegionTileStream:
    """Iterates over the tile rows of ``raster`` and yields ``(tiles [n,3,S,S] float32 on the device, [(ty, tx), ...])``.

    ``tile`` is the tile side on the (halved, if ``shrink`` == 2) slide, ``img_size`` the network input side.  With ``overlap``
    (pixels of the halved slide, like ``tile``) strip ``j`` holds slide rows ``[j * step, j * step + tile)``, ``step = tile -
    overlap``: consecutive strips share ``overlap`` rows, which are uploaded with both."""

    def __init__(self, raster, tile=1536, img_size=1024, shrink=1, overlap=0):
        if not torch.cuda.is_available():
            raise _lib.AyError("no HIP device: RegionTileStream has no CPU fallback")
        assert raster.ndim == 3 and raster.shape[2] == 3 and raster.dtype == np.uint8, "uint8 [H,W,3] raster"
        assert shrink in (1, 2)
        self.raster, self.tile, self.S, self.shrink = raster, int(tile), int(img_size), int(shrink)
        H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
        self.overlap = int(overlap)
        self.tiles_y, self.tiles_x, self.step = tile_grid(H, W, self.tile, self.overlap)
        self.dev = torch.device("cuda", torch.cuda.current_device())
        rows = self.tile * shrink
        self._pinned = [torch.empty(rows, raster.shape[1], 3, dtype=torch.uint8).pin_memory() for _ in range(2)]
        self._strips = [torch.empty(rows, raster.shape[1], 3, dtype=torch.uint8, device=self.dev) for _ in range(2)]
        self._copy = torch.cuda.Stream(device=self.dev)
        self._pool = ThreadPoolExecutor(max_workers=4)      # row chunks of one staging copy
        self._stager = ThreadPoolExecutor(max_workers=1)    # one strip ahead of the consumer
        self._chunk = -(-rows // 4)
        self._uploaded = [None, None]   # event: strip landed in _strips[k]
        self._consumed = [None, None]   # event: the ingest kernel that read _strips[k] is done

    def __len__(self):
        return self.tiles_y

    def _stage(self, j):
        """host side of strip j: raster rows -> pinned buffer (runs on the staging thread, under the consumer's GPU work)"""
        k = j & 1
        rows = self.tile * self.shrink
        first = j * self.step * self.shrink
        src = self.raster[first:first + rows]
        n = src.shape[0]
        if self._uploaded[k] is not None:
            self._uploaded[k].synchronize()      # the host buffer is free again once its last copy has run
        # staging copy by NumPy (memcpy speed; torch's uint8 copy_ ran at a quarter of it), rows split over a few threads --
        # the copy releases the GIL -- so that one strip stages faster than the GPU consumes it
        dst = self._pinned[k].numpy()
        parts = [(a, min(a + self._chunk, n)) for a in range(0, n, self._chunk)]
        list(self._pool.map(lambda ab: np.copyto(dst[ab[0]:ab[1]], src[ab[0]:ab[1]]), parts))
        return n

    def _copy_to_device(self, j, n):
        k = j & 1
        if self._consumed[k] is not None:
            self._copy.wait_event(self._consumed[k])
        with torch.cuda.stream(self._copy):
            self._strips[k][:n].copy_(self._pinned[k][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self._copy)
        self._uploaded[k] = ev

    def __iter__(self):
        L = _lib.lib()
        main = torch.cuda.current_stream()
        dev_index = self.dev.index

        def stage(j):
            torch.cuda.set_device(dev_index)
            return self._stage(j)

        fut = self._stager.submit(stage, 0) if self.tiles_y else None
        for j in range(self.tiles_y):
            k = j & 1
            valid = fut.result()
            self._copy_to_device(j, valid)
            if j + 1 < self.tiles_y:  # staged while the consumer's model + NMS of this strip run
                fut = self._stager.submit(stage, j + 1)
            main.wait_event(self._uploaded[k])
            out = torch.empty(self.tiles_x, 3, self.S, self.S, device=self.dev, dtype=torch.float32)
            if self.overlap == 0:
                check(L.ay_ingest_region_tiles_u8(ptr(self._strips[k]), valid, self.raster.shape[1], self.raster.shape[1] * 3, self.shrink,
                                                  self.tile, 1, self.tiles_x, self.S, ptr(out), _lib.stream_ptr()),
                      "ay_ingest_region_tiles_u8")
            else:
                check(L.ay_ingest_region_tiles_step_u8(ptr(self._strips[k]), valid, self.raster.shape[1], self.raster.shape[1] * 3,
                                                       self.shrink, self.tile, self.step, 1, self.tiles_x, self.S, ptr(out),
                                                       _lib.stream_ptr()), "ay_ingest_region_tiles_step_u8")
            done = torch.cuda.Event()
            done.record(main)
            self._consumed[k] = done
            yield out, [(j, i) for i in range(self.tiles_x)]


def detect_region(model, raster, tile=1536, img_size=1024, shrink=1, conf_thres=0.8, nms_thres=0.4, batch_size=64, overlap=0,
                  seam_thres=0.5, max_det=1024, seam_capacity=None):
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
    without a row omitted."""
    if overlap:
        return _detect_region_overlap(model, raster, tile, img_size, shrink, conf_thres, nms_thres, batch_size, overlap, seam_thres,
                                      max_det, seam_capacity)
    results = []
    scale = float(tile) / float(img_size)
    model.eval()
    for tiles, coords in RegionTileStream(raster, tile, img_size, shrink):
        for s in range(0, tiles.shape[0], batch_size):
            with torch.no_grad():  # rows stay on the device; only the detections come back
                det = non_max_suppression(model.forward_device(tiles[s:s + batch_size]), conf_thres, nms_thres)
            for (ty, tx), d in zip(coords[s:s + batch_size], det):
                if d is None:
                    continue
                d = d.cpu()
                d[:, :4] *= scale
                d[:, [0, 2]] += tx * tile
                d[:, [1, 3]] += ty * tile
                results.append((ty, tx, d))
    return results


def _detect_region_overlap(model, raster, tile, img_size, shrink, conf_thres, nms_thres, batch_size, overlap, seam_thres, max_det,
                           seam_capacity):
    from .postprocess import seam_merge_device
    L = _lib.lib()
    stream = RegionTileStream(raster, tile, img_size, shrink, overlap)
    dev, TX, step = stream.dev, stream.tiles_x, stream.step
    T = stream.tiles_y * TX
    capacity = int(seam_capacity) if seam_capacity else min(T * int(max_det), 1 << 22)
    # per tile, on the device for the whole slide: its id (grid order) and the (x, y) of its corner
    ids = torch.arange(T, dtype=torch.int32)
    origins = torch.stack([(ids % TX) * step, (ids // TX) * step], 1).to(torch.float32).to(dev)
    ids = ids.to(dev)
    slide_rows = torch.empty(capacity, 7, device=dev, dtype=torch.float32)
    slide_tile = torch.empty(capacity, device=dev, dtype=torch.int32)
    slide_count = torch.zeros(2, device=dev, dtype=torch.int32)
    scale = C.c_float(float(tile) / float(img_size))
    model.eval()
    for tiles, coords in stream:
        for s in range(0, tiles.shape[0], batch_size):
            t0 = coords[s][0] * TX + coords[s][1]
            with torch.no_grad():  # no read-back: the NMS result buffers are overwritten by the next batch, the append is right behind
                rows, _, count, _ = nms_device(model.forward_device(tiles[s:s + batch_size]), conf_thres, nms_thres, int(max_det))
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
