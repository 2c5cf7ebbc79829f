"""Strips of a raster on the device.  Three layers: ``upload.Uploader`` holds the double-buffer protocol and nothing about slides;
:class:`StripStream` feeds it the strips of a raster (height, step, shrink, optionally column spans and the strips to visit) and is
all the slide passes need; :class:`RegionTileStream` owns a strip stream and adds the tile side (views, stain, masks, batches)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from ..upload import Uploader
from ..views import check_views
from .colour import StainMap
from .grid import check_tile_mask, hip_device, tile_grid

STRIP_ROWS = 1536       # rows of the (halved) slide per strip of the passes that are free to choose (a tile row of the default tile)


class StripStream:
    """Strips of a uint8 ``[H, W, 3]`` raster on the device, one after another: strip ``j`` is rows ``[j * step, j * step +
    height)`` of the (halved, for ``shrink == 2``) slide, ``tile_grid``'s ``max(1, ceil((H - (height - step)) / step))`` of them
    (``count``).  ``jobs`` (default: every strip at full width) lists the strips to visit as ``(j, c0, c1)`` with the span of
    SOURCE columns ``[c0, c1)`` to stage.

    The iteration yields ``(j, k, rows, width)`` once the current stream waits for the upload of strip ``j``: a ``rows x width``
    block of source pixels, rows ``3 * width`` bytes apart, whose leading kernel arguments are ``args(k, rows, width)``.  The user
    issues every kernel that reads the block on the current stream and then calls ``release(k)``; :meth:`each` does both around a
    call.  Staging, upload and their order are ``upload.Uploader``'s, with the buffers for the largest job allocated here."""

    def __init__(self, raster, height, step, shrink=1, jobs=None):
        dev = hip_device("the strip stream has")
        assert raster.ndim == 3 and raster.shape[2] == 3 and raster.dtype == np.uint8, "uint8 [H,W,3] raster"
        assert shrink in (1, 2)
        self.raster, self.height, self.step, self.shrink = raster, int(height), int(step), int(shrink)
        self.count = tile_grid(raster.shape[0] // shrink, 1, self.height, self.height - self.step)[0]
        self.jobs = [(j, 0, raster.shape[1]) for j in range(self.count)] if jobs is None else jobs
        self.dev = dev
        rows = self.height * self.shrink
        self._chunk = -(-rows // 4)
        self._up = Uploader(self.dev, rows * 3 * max((c1 - c0 for _, c0, c1 in self.jobs), default=0))
        self.blocks = [None, None]      # the device buffer that holds block k

    def staged_bytes(self):
        """bytes of the raster that one pass stages and uploads"""
        rows, first = self.height * self.shrink, self.step * self.shrink
        return sum(len(range(j * first, min(j * first + rows, self.raster.shape[0]))) * (c1 - c0) * 3 for j, c0, c1 in self.jobs)

    def _fill(self, idx, host):
        """host side of a strip: raster rows (the job's columns) -> pinned buffer, as one contiguous block"""
        j, c0, c1 = self.jobs[idx]
        first = j * self.step * self.shrink
        src = self.raster[first:first + self.height * self.shrink, c0:c1]
        n, w = src.shape[0], src.shape[1]
        # staging copy by NumPy (memcpy speed; torch's uint8 copy_ ran at a quarter of it), rows split over a few threads --
        # the copy releases the GIL -- so that one strip stages faster than the GPU consumes it
        dst = host(n * w * 3)[:n * w * 3].reshape(n, w, 3)
        parts = [(a, min(a + self._chunk, n)) for a in range(0, n, self._chunk)]
        list(self._up.pool.map(lambda ab: np.copyto(dst[ab[0]:ab[1]], src[ab[0]:ab[1]]), parts))
        return (j, n, w), n * w * 3

    def __iter__(self):
        for k, (j, n, w), block, _ in self._up.run(len(self.jobs), self._fill):
            self.blocks[k] = block
            yield j, k, n, w

    def args(self, k, rows, width):
        """the leading arguments of every entry point that reads a strip: region, rows, width, row stride in bytes, shrink"""
        return ptr(self.blocks[k]), rows, width, width * 3, self.shrink

    def release(self, k):
        self._up.release(k)

    def each(self, call):
        """``call(k, j, rows, width)`` on every block, released behind the kernels the call issues"""
        for j, k, rows, width in self:
            call(k, j, rows, width)
            self.release(k)


class ResidentStrips:
    """:class:`StripStream`'s ``dev`` / ``args`` / ``each`` over a uint8 ``[H, W, 3]`` tensor that lives on the device: the strips of
    the stream at ``step == height``, read in place; block ``k`` is the one that starts at source row ``k``"""

    def __init__(self, raster, height, shrink=1):
        self.raster, self.height, self.shrink, self.dev = raster.contiguous(), int(height), int(shrink), raster.device

    def args(self, k, rows, width):
        return ptr(self.raster[k:]), rows, width, width * 3, self.shrink

    def each(self, call):
        rows, per = (self.raster.shape[0] // self.shrink) * self.shrink, self.height * self.shrink
        for y in range(0, rows, per):
            call(y, y // per, min(per, rows - y), self.raster.shape[1])


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
    tile-major (tile ``i`` in view ``views[j]`` is image ``i * V + j``), with the coordinates of the ``n`` tiles.

    ``stain`` (default ``None``: ``byte / 255``, the present cut): a :class:`StainMap`.  Every tile, masked or not, in any list of
    views, is then cut by ``ay_ingest_region_tiles_stain_u8``, which stores THE STAIN RULE's mapped value instead."""

    def __init__(self, raster, tile=1536, img_size=1024, shrink=1, overlap=0, tile_mask=None, views=(0,), stain=None):
        self.views = check_views(views)
        if stain is not None and not isinstance(stain, StainMap):
            raise ValueError(f"stain: need a wsi.StainMap or None, got {type(stain).__name__}")
        self.stain = stain
        hip_device("RegionTileStream has")
        self.raster, self.tile, self.S, self.shrink = raster, int(tile), int(img_size), int(shrink)
        H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
        self.overlap = int(overlap)
        self.tiles_y, self.tiles_x, self.step = tile_grid(H, W, self.tile, self.overlap)
        self.tile_mask = None if tile_mask is None else check_tile_mask(tile_mask, H, W, self.tile, self.overlap)
        self._strips = StripStream(raster, self.tile, self.step, self.shrink, self._strip_jobs())
        self.dev = self._strips.dev
        self._view_ids = (C.c_int * len(self.views))(*self.views)

    def _strip_jobs(self):
        """with a mask, the strips that are staged: ``[(j, c0, c1)]`` = tile row and its span of SOURCE columns ``[c0, c1)``"""
        if self.tile_mask is None:
            return None
        W, out = self.raster.shape[1] // self.shrink, []
        for j in range(self.tiles_y):
            txs = np.flatnonzero(self.tile_mask[j])
            if len(txs):
                out.append((j, int(txs[0]) * self.step * self.shrink, min(int(txs[-1]) * self.step + self.tile, W) * self.shrink))
        return out

    def _staged_bytes(self):
        """bytes of the raster that one pass stages and uploads"""
        return self._strips.staged_bytes()

    def __len__(self):
        """the number of strips the iteration yields: ``tiles_y`` without a mask, the tile rows that hold a wanted tile with one"""
        return len(self._strips.jobs)

    def _wanted(self):
        """``[(ty, tx)]`` of the tiles the stream yields, in grid order"""
        if self.tile_mask is None:
            return [(j, i) for j in range(self.tiles_y) for i in range(self.tiles_x)]
        return [(int(j), int(i)) for j, i in zip(*np.nonzero(self.tile_mask))]

    def _wanted_table(self):
        """for the list ingest, on the device: the origin of every wanted tile inside its strip's block, int32 [n][2] = (x, 0) in
        grid order, and per tile row the index of its first wanted tile (host)"""
        span0 = {j: c0 // self.shrink for j, c0, _ in self._strips.jobs}
        xy = np.array([(i * self.step - span0[j], 0) for j, i in self._wanted()], np.int32).reshape(-1, 2)
        starts = np.r_[0, np.cumsum(self.tile_mask.sum(1))]
        return torch.from_numpy(xy).to(self.dev), starts

    def _cut(self, L, k, n, w, origins, m, out):
        """tiles ``origins[:m]`` of strip block ``k`` -> ``out[:m * V]``, every tile in the stream's views; ``origins=None``: the
        ``m`` tiles of a full row, ``step`` apart (the origins are computed, not read: faster than the list entry)"""
        strip, ids = self._strips.args(k, n, w), self._view_ids
        if origins is None:     # overlap == 0 is step == tile
            check(L.ay_ingest_region_tiles_step_u8(*strip, self.tile, self.step, 1, m, self.S, ptr(out), _lib.stream_ptr()),
                  "ay_ingest_region_tiles_step_u8")
        elif self.stain is not None:
            check(L.ay_ingest_region_tiles_stain_u8(*strip, self.tile, ptr(origins), m, ids, len(ids), ptr(self.stain.params), self.S,
                                                    ptr(out), _lib.stream_ptr()), "ay_ingest_region_tiles_stain_u8")
        elif self.views != (0,):
            check(L.ay_ingest_region_tiles_views_u8(*strip, self.tile, ptr(origins), m, ids, len(ids), self.S, ptr(out),
                                                    _lib.stream_ptr()), "ay_ingest_region_tiles_views_u8")
        else:
            check(L.ay_ingest_region_tiles_list_u8(*strip, self.tile, ptr(origins), m, self.S, ptr(out), _lib.stream_ptr()),
                  "ay_ingest_region_tiles_list_u8")

    def __iter__(self):
        L = _lib.lib()
        V = len(self.views)
        row = None
        if self.tile_mask is not None:
            table, starts = self._wanted_table()
            coords = self._wanted()
        elif self.views != (0,) or self.stain is not None:     # the views and stain entries take a list of origins: those of a full tile row
            row = torch.tensor([(i * self.step, 0) for i in range(self.tiles_x)], dtype=torch.int32, device=self.dev)
        for j, k, valid, width in self._strips:
            if self.tile_mask is None:
                origins, m, cs = row, self.tiles_x, [(j, i) for i in range(self.tiles_x)]
            else:
                a, b = int(starts[j]), int(starts[j + 1])
                origins, m, cs = table[a:], b - a, coords[a:b]
            out = torch.empty(m * V, 3, self.S, self.S, device=self.dev, dtype=torch.float32)
            self._cut(L, k, valid, width, origins, m, out)
            self._strips.release(k)
            yield out, cs

    def batches(self, per_call):
        """The iteration as detect_region takes it, one item per model call: ``(tiles [n * V,3,S,S], [(ty, tx)] * n)`` with ``n <=
        per_call``.  Without a mask the tiles of a strip in slices of ``per_call``, never across strips; with one, :meth:`_batches`."""
        V = len(self.views)
        if self.tile_mask is None:
            for tiles, coords in self:
                for s in range(0, len(coords), per_call):
                    yield tiles[s * V:(s + per_call) * V], coords[s:s + per_call]
        else:
            coords = self._wanted()
            for tiles, w0 in self._batches(per_call):
                yield tiles, coords[w0:w0 + tiles.shape[0] // V]

    def _batches(self, batch_size):
        """The masked iteration of :meth:`batches`: yields ``(tiles [n * V,3,S,S], w0)``, the wanted tiles ``w0 .. w0 + n`` of
        :meth:`_wanted`, ``n == batch_size`` but for the last batch: a strip's wanted tiles are cut into the open batch buffer at its
        fill, so that batches are filled across strip boundaries.  Every ingest of a strip is issued (into as many batch buffers as
        it takes) and the strip released before its batches are handed out, so the refill of a strip buffer never waits for a model
        call, also when a batch holds tiles of two strips."""
        L = _lib.lib()
        table, starts = self._wanted_table()
        V = len(self.views)
        cur, fill, w0 = None, 0, 0
        for j, k, valid, width in self._strips:
            a, b = int(starts[j]), int(starts[j + 1])
            ready = []
            while a < b:
                if cur is None:
                    cur, fill, w0 = torch.empty(batch_size * V, 3, self.S, self.S, device=self.dev, dtype=torch.float32), 0, a
                m = min(b - a, batch_size - fill)
                self._cut(L, k, valid, width, table[a:], m, cur[fill * V:])
                fill, a = fill + m, a + m
                if fill == batch_size:
                    ready.append((cur, w0))
                    cur = None
            self._strips.release(k)
            yield from ready
        if cur is not None:
            yield cur[:fill * V], w0
