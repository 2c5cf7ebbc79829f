"""WSI -> tile streaming: detection over a whole-slide raster without the disk round trip of the
reference (``crop.py:13-25`` writes 1536-px JPEG tiles with pyvips ``dzsave``, ``detect.py:59-105`` reads them back).

A slide (any ``[H, W, 3]`` uint8 array: a NumPy memmap of a decoded level, a pyvips/openslide region fetched by the caller)
is walked in full-width strips of one tile row.  A strip is one contiguous slice of the raster: it goes to the device in a
single copy from a pinned staging buffer on a copy stream (two buffers, so strip i+1 uploads while strip i computes).  Three
layers: ``upload.Uploader`` holds that double-buffer protocol and nothing about slides; :class:`StripStream` feeds it the strips
of a raster (height, step, shrink, optionally column spans and the strips to visit) and is all the slide passes below need;
:class:`RegionTileStream` owns a strip stream and adds the tile side (views, stain, masks, batches).
``ay_ingest_region_tiles_step_u8`` cuts the row of tiles out of a strip on the device -- at ``step == tile`` dzsave's 'google' layout:
a ``tile`` grid from the top-left corner, edge tiles padded with the background 255 -- with the optional 40x -> 20x halving
(``crop.py:44-47``) and the detect-time ``/255`` + nearest resize fused in.  Detections come back in slide coordinates.

Abutting tiles split every object that straddles a seam.  With ``overlap > 0`` the tile origins are ``tile - overlap`` apart
(:func:`tile_grid`, the ``step`` of the same entry point), every object no larger than ``overlap`` is seen whole by at least one
tile, the per-tile detections stay on the device (``utils.nms_device`` -> ``ay_seam_append``) and one slide-level pass removes
the second sightings (``ay_seam_merge``; the rule is stated in ``include/amyloid_yolo.h``).

Most of a histology slide is glass.  :func:`tissue_counts` (``ay_tile_tissue_u8``, the rule in ``include/amyloid_yolo.h``) counts the
tissue pixels of every tile, usually on a low-resolution level, :func:`wanted_tiles` turns the counts into a ``tile_mask``, and with
a mask the stream never stages a strip without a wanted tile, stages of any other strip only the columns between its first and its
last wanted tile and cuts only the wanted tiles out of it (``ay_ingest_region_tiles_list_u8``, the same cut with the origins read
from a list); its batches are then filled with wanted tiles across strip boundaries.  Every mode of :func:`detect_region` takes its
model calls from one generator, :meth:`RegionTileStream.batches`.

Training reads the same rasters: :class:`SlideSampler` draws windows centred on annotations, hard cases and tissue out of annotated
slides and cuts them with the fused augmentation kernel under THE WINDOW RULE (``ay_augment_ingest_window_u8``), for
``train(source=...)``.

What a slide carries: :func:`burden_map` bins the rows of a slide into class count maps (``ay_burden_bin``, THE BURDEN RULE),
:func:`densest_fields` picks the densest microscope-sized fields of every class (``ay_field_select``, THE FIELD RULE), and
:func:`quantify_region` joins them with :func:`detect_region` and the tissue of every map cell into counts and densities per slide.

Stain: :func:`stain_stats` unmixes the tissue pixels of a slide into hematoxylin and DAB (``ay_stain_hist_u8``, THE STAIN RULE),
:class:`StainMap` turns its strengths and a target's into gains, and ``detect_region(stain=...)`` cuts every tile through the colour
map (``ay_ingest_region_tiles_stain_u8``); :func:`normalize_region` gives the mapped raster itself.  :func:`estimate_basis` finds the
slide's own two stain vectors (``ay_stain_moments_u8``, ``ay_stain_direction_hist_u8``, THE BASIS RULE) for every ``basis=`` here, and
``StainMap(..., remix=True)`` maps between slides whose bases differ.

Amyloid load: :func:`stain_load` classifies every pixel of a slide (tissue, DAB-positive) and sums it per map cell and per detection
box (``ay_stain_load_u8``, THE LOAD RULE); :func:`box_morphometry` turns the box sums into areas, fill and mean optical density,
and ``quantify_region(load=True)`` puts the load map next to the count maps.

Focus: :func:`focus_map` sums the Laplacian of the luma over the tissue of every map cell and detection box (``ay_focus_u8``, THE
FOCUS RULE) into a sharpness map, :func:`focus_summary` reads it, and ``quantify_region(focus=True)`` reports it next to the counts.

Plaque segmentation: :func:`segment_boxes` labels the connected stain-positive component under every detection (``ay_box_segments_u8``,
THE SEGMENT RULE), :func:`plaque_morphometry` turns its words into area, core fraction, centroid, perimeter and compactness, and
``quantify_region(segment=True)`` reports them next to the counts.

Spatial statistics: :func:`spatial_stats` counts the cross-class pairs of a slide's detections within every radius and finds every
row's nearest neighbour of every class (``ay_pair_counts``, THE PAIR RULE), turns them into Ripley's K and L, the pair correlation
and the nearest-neighbour distribution on the host, and ``quantify_region(spatial_radii=...)`` reports them next to the counts.

No CPU fallback: the product path needs the HIP library and a GPU."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr
from .upload import Uploader, pack_records, record_offset
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
        if not torch.cuda.is_available():
            raise _lib.AyError("no HIP device: the strip stream has no CPU fallback")
        assert raster.ndim == 3 and raster.shape[2] == 3 and raster.dtype == np.uint8, "uint8 [H,W,3] raster"
        assert shrink in (1, 2)
        self.raster, self.height, self.step, self.shrink = raster, int(height), int(step), int(shrink)
        self.count = tile_grid(raster.shape[0] // shrink, 1, self.height, self.height - self.step)[0]
        self.jobs = [(j, 0, raster.shape[1]) for j in range(self.count)] if jobs is None else jobs
        self.dev = torch.device("cuda", torch.cuda.current_device())
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
        if not torch.cuda.is_available():
            raise _lib.AyError("no HIP device: RegionTileStream has no CPU fallback")
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


def tissue_counts(raster, tile, shrink=1, overlap=0, bg_level=220):
    """Tissue pixels per tile of the ``tile_grid(H, W, tile, overlap)`` grid over ``raster`` -> NumPy int32 ``[tiles_y, tiles_x]``.

    A pixel of the (halved, for ``shrink=2``: the ingest's 2x2 round-half-up means) slide is tissue iff ``min(R, G, B) < bg_level``
    (``bg_level`` in 0 .. 256; the default suits scanned glass); pixels of a shared band count for every tile that holds them, the
    padding outside the slide never counts (THE TISSUE RULE in ``include/amyloid_yolo.h``, ``ay_tile_tissue_u8``).  The raster goes
    through a :class:`StripStream` once and the counts come back in one read.  Meant for a low-resolution level
    of the slide, with ``tile`` and ``overlap`` divided by that level's downsample (any ``[H, W, 3]`` uint8 array, strided views
    such as :func:`probe_view`'s included), and exact on any raster: on the full one it costs a full upload of the slide.  A strip
    reaches the kernel with rows ``3 * width`` bytes apart: the kernel's 16-byte loads need that to be a multiple of 16 (a width
    that is a multiple of 16 pixels) and fall back to byte loads otherwise, about three times slower on the device and the same
    counts; on a low-resolution level either is small against the staging copy."""
    bg_level = int(bg_level)
    if not 0 <= bg_level <= 256:
        raise ValueError(f"tissue_counts: bg_level {bg_level} outside 0 .. 256")
    tile = int(tile)
    tiles_y, tiles_x, step = tile_grid(raster.shape[0] // shrink, raster.shape[1] // shrink, tile, overlap)
    strips = StripStream(raster, tile, step, shrink)
    L = _lib.lib()
    counts = torch.empty(tiles_y, tiles_x, device=strips.dev, dtype=torch.int32)
    strips.each(lambda k, j, valid, width: check(
        L.ay_tile_tissue_u8(*strips.args(k, valid, width), tile, step, 1, tiles_x, bg_level, ptr(counts[j]), _lib.stream_ptr()),
        "ay_tile_tissue_u8"))
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
                  views=(0,), min_views=1, vote_thres=None, stain=None):
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
    another list may give another result.  With the defaults nothing of this is called and the result is unchanged, bit for bit.

    ``stain`` (default ``None``; a :class:`StainMap`, e.g. ``StainMap(stain_stats(raster), stain_stats(training_slide).strength())``)
    brings the slide's stain strengths to those the model was trained on: every tile is cut through THE STAIN RULE's colour map
    (``include/amyloid_yolo.h``) instead of ``byte / 255``, on the masked, unmasked, overlap and views paths alike; the tissue probe
    of ``min_tissue`` still looks at the raster's own colours.  With ``None`` nothing of it is called."""
    if stain is not None and not isinstance(stain, StainMap):
        raise ValueError(f"detect_region: stain must be a wsi.StainMap or None, got {type(stain).__name__}")
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
    per_call = int(batch_size) if tta is None else max(1, int(batch_size) // len(views))   # tiles per model call: at most batch_size images
    stream = RegionTileStream(raster, tile, img_size, shrink, overlap, tile_mask, views, stain)
    model.eval()
    if overlap:
        return _detect_region_overlap(model, stream, per_call, conf_thres, nms_thres, seam_thres, int(max_det), seam_capacity, tta)
    results = []
    for tiles, coords in stream.batches(per_call):
        with torch.no_grad():  # rows stay on the device; only the detections come back
            pred = model.forward_device(tiles)
            if tta is None:    # a read-back per tile, no cap on the rows of a tile
                det = [None if d is None else d.cpu() for d in non_max_suppression(pred, conf_thres, nms_thres)]
            else:              # V views per tile through one merge-NMS; one read-back per batch
                rows, _, count, _ = nms_views_device(pred, views, conf_thres, nms_thres, int(max_det), int(min_views), vote_thres,
                                                     img_dim=img_size)
                count_h, rows_h = count.cpu().tolist(), rows.cpu()
                if max(count_h) > int(max_det):
                    raise _lib.AyError(f"detect_region: a tile holds more than max_det={max_det} detections; raise max_det or conf_thres")
                det = [d[:n].clone() if n else None for n, d in zip(count_h, rows_h)]
        results += [(ty, tx, _to_slide(d, ty, tx, stream)) for (ty, tx), d in zip(coords, det) if d is not None]
    return results


def _to_slide(rows, ty, tx, stream):
    """rows of tile ``(ty, tx)`` of an abutting grid, boxes in network pixels -> in pixels of the (halved) slide, in place (fp32)"""
    rows[:, :4] *= float(stream.tile) / float(stream.S)
    rows[:, [0, 2]] += tx * stream.tile
    rows[:, [1, 3]] += ty * stream.tile
    return rows


def _detect_region_overlap(model, stream, per_call, conf_thres, nms_thres, seam_thres, max_det, seam_capacity, tta):
    """the path with overlapping tiles: the rows of every model call are appended to a slide buffer on the device (``ay_seam_append``
    scales and shifts them, the arithmetic of :func:`_to_slide` at ``step`` between origins), one seam merge and one read-back at the end"""
    from .postprocess import seam_merge_device
    L = _lib.lib()
    dev, TX, step = stream.dev, stream.tiles_x, stream.step
    # per tile that runs, on the device for the whole slide: its id (grid order on the full grid) and the (x, y) of its corner
    if stream.tile_mask is None:
        ids = torch.arange(stream.tiles_y * TX, dtype=torch.int32)
    else:
        ids = torch.from_numpy(np.flatnonzero(stream.tile_mask.ravel()).astype(np.int32))
    capacity = int(seam_capacity) if seam_capacity else min(len(ids) * max_det, 1 << 22)
    origins = torch.stack([(ids % TX) * step, (ids // TX) * step], 1).to(torch.float32).to(dev)
    ids = ids.to(dev)
    slide_rows = torch.empty(capacity, 7, device=dev, dtype=torch.float32)
    slide_tile = torch.empty(capacity, device=dev, dtype=torch.int32)
    slide_count = torch.zeros(2, device=dev, dtype=torch.int32)
    scale = C.c_float(float(stream.tile) / float(stream.S))
    t0 = 0   # tiles run so far: the batches come in the order of ids / origins
    for tiles, coords in stream.batches(per_call):
        with torch.no_grad():  # no read-back: the NMS result buffers are overwritten by the next batch, the append is right behind
            if tta is None:
                rows, _, count, _ = nms_device(model.forward_device(tiles), conf_thres, nms_thres, max_det)
            else:             # rows and count in nms_device's form, one image per TILE
                views, min_views, vote_thres = tta
                rows, _, count, _ = nms_views_device(model.forward_device(tiles), views, conf_thres, nms_thres, max_det, min_views,
                                                     vote_thres, img_dim=stream.S)
        B = rows.shape[0]
        check(L.ay_seam_append(ptr(rows), ptr(count), B, max_det, scale, ptr(origins[t0:t0 + B]), ptr(ids[t0:t0 + B]),
                               ptr(slide_rows), ptr(slide_tile), ptr(slide_count), capacity, _lib.stream_ptr()), "ay_seam_append")
        t0 += B
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


# ---- slide-level burden: class count maps, tissue density, densest fields -----------------------------------------------------------
BURDEN_MAX_CLASSES, BURDEN_MAX_FIELDS, BURDEN_MAX_FIELD_SIDE = 64, 64, 46340    # include/amyloid_yolo.h, THE BURDEN / FIELD RULE
BURDEN_FLAG_NONFINITE, BURDEN_FLAG_CLASS = 1, 2


def _whole(v, lo, hi, what):
    """``v`` as an int in ``lo .. hi``, else ``ValueError`` (bools and fractions are no counts)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} {v!r} is no integer in {lo} .. {hi}")
    return int(v)


def _burden_device():
    if not torch.cuda.is_available():
        raise _lib.AyError("no HIP device: the burden maps have no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def _int_planes(a, dev):
    t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.int32)))
    return t.to(device=dev, dtype=torch.int32).contiguous()


def burden_map(rows, slide_hw, cell=128, num_classes=2, min_conf=0.0):
    """Class count maps of a slide's detections (``ay_burden_bin``, THE BURDEN RULE in ``include/amyloid_yolo.h``).

    ``rows`` [M,7] = (x1, y1, x2, y2, conf, cls_conf, cls_pred) in pixels of the (halved) slide, as :func:`detect_region` returns
    them (concatenated), a tensor or array on the host or the device; ``slide_hw`` = (H, W) of that slide; ``cell`` the side of a
    map cell in pixels; ``num_classes`` = C in 1 .. 64 (default: the reference's two, Cored and CAA).  A row counts once, in the cell
    of its centre (a centre outside the slide in the nearest border cell), for its class, if ``conf >= min_conf``; a row with a
    centre that is not finite or a ``cls_pred`` that is no integer in 0 .. C-1 is flagged and counts nowhere.

    Returns a dict: ``counts`` int32 [C,Gy,Gx] on the device (the grid is ``tile_grid(H, W, cell)``, the one :func:`tissue_counts`
    counts on with ``tile=cell``), ``counted`` NumPy [C] (``counts[c].sum()``), ``below``, ``flagged`` (``counted.sum() + below +
    flagged == M``) and ``flags`` (bit 1: a centre not finite, bit 2: a class outside).  Reads the statistics back once."""
    cell, nc = _whole(cell, 1, 2 ** 31 - 1, "burden_map: cell"), _whole(num_classes, 1, BURDEN_MAX_CLASSES, "burden_map: num_classes")
    H, W = (_whole(v, 1, 2 ** 31 - 1, "burden_map: slide_hw") for v in slide_hw)
    if rows is None or len(rows.shape) != 2 or rows.shape[1] != 7:
        raise ValueError(f"burden_map: rows must be [M,7], got {None if rows is None else tuple(rows.shape)}")
    min_conf = float(min_conf)
    gy, gx, _ = tile_grid(H, W, cell)
    if nc * gy * gx > 1 << 30:
        raise ValueError(f"burden_map: {nc} classes x {gy} x {gx} cells exceed 2**30 counters; choose a larger cell")
    from .stats import _slide_array
    dev = _burden_device()
    rows = _slide_array(rows, 7, dev)
    M = int(rows.shape[0])
    counts = torch.empty(nc, gy, gx, device=dev, dtype=torch.int32)
    stats = torch.empty(nc + 3, device=dev, dtype=torch.int32)
    check(_lib.lib().ay_burden_bin(ptr(rows) if M else None, M, nc, H, W, cell, C.c_float(min_conf), ptr(counts), ptr(stats), _lib.stream_ptr()),
          "ay_burden_bin")
    st = stats.cpu().numpy()
    return {"counts": counts, "counted": st[:nc].copy(), "below": int(st[nc]), "flagged": int(st[nc + 1]), "flags": int(st[nc + 2])}


def densest_fields(counts, tissue=None, field=8, top_k=5, need_tissue=0):
    """The densest ``field x field``-cell fields of every class (``ay_field_select``, THE FIELD RULE in ``include/amyloid_yolo.h``).

    ``counts`` int32 [C,Gy,Gx] (:func:`burden_map`), ``tissue`` int32 [Gy,Gx] or None (tissue pixels per cell), on the host or the
    device.  A field lies entirely inside the grid and is eligible iff ``tissue`` is None or its tissue sum reaches ``need_tissue``;
    per class, up to ``top_k`` (1 .. 64) rounds pick the eligible field with the largest count that overlaps no earlier pick of the
    class (ties: the lowest ``fy * (Gx - field + 1) + fx``) and stop at a count of 0.  ``field`` times the cell side the maps were
    made with must not exceed 46340, so that a field's tissue sum fits int32; this function does not know the cell side and only
    refuses ``field > 46340``.

    Returns NumPy ``fields`` int32 [C,top_k,4] = (fy, fx, count, tissue) in pick order (rows not filled: -1; tissue 0 without
    ``tissue``) and ``n_found`` int32 [C]."""
    if counts is None or len(counts.shape) != 3:
        raise ValueError(f"densest_fields: counts must be [C,Gy,Gx], got {None if counts is None else tuple(counts.shape)}")
    Cn, gy, gx = (int(v) for v in counts.shape)
    if not 1 <= Cn <= BURDEN_MAX_CLASSES or gy < 1 or gx < 1 or gy * gx > 1 << 30:
        raise ValueError(f"densest_fields: counts {(Cn, gy, gx)}: need 1 .. {BURDEN_MAX_CLASSES} classes and a grid of 1 .. 2**30 cells")
    if tissue is not None and tuple(tissue.shape) != (gy, gx):
        raise ValueError(f"densest_fields: tissue {tuple(tissue.shape)} is not the grid {(gy, gx)} of counts")
    F = _whole(field, 1, BURDEN_MAX_FIELD_SIDE, "densest_fields: field")
    K = _whole(top_k, 1, BURDEN_MAX_FIELDS, "densest_fields: top_k")
    need = _whole(need_tissue, 0, 2 ** 31 - 1, "densest_fields: need_tissue")
    dev = _burden_device()
    counts = _int_planes(counts, dev)
    tissue = None if tissue is None else _int_planes(tissue, dev)
    L = _lib.lib()
    fields = torch.empty(Cn, K, 4, device=dev, dtype=torch.int32)
    n_found = torch.empty(Cn, device=dev, dtype=torch.int32)
    ws = torch.empty(max(int(L.ay_field_select_workspace_bytes(Cn, gy, gx, F)), 16), device=dev, dtype=torch.uint8)
    check(L.ay_field_select(ptr(counts), Cn, gy, gx, ptr(tissue), F, need, K, ptr(fields), ptr(n_found), ptr(ws), ws.numel(), _lib.stream_ptr()),
          "ay_field_select")
    return fields.cpu().numpy(), n_found.cpu().numpy()


def _field_sums(picked, filled, F, maps):
    """for every filled field ``picked[c, k]`` of :func:`densest_fields`: ``(c, k, [the sum of each map over the field's F x F cells])``"""
    for c, k in zip(*np.nonzero(filled)):
        fy, fx = int(picked[c, k, 0]), int(picked[c, k, 1])
        yield c, k, [int(m[fy:fy + F, fx:fx + F].sum()) for m in maps]


def quantify_region(model, raster, cell=128, field=8, top_k=5, field_min_tissue=0.5, mpp=None, min_conf=0.0, stain_stats=None,
                    dab_thres=None, load=False, focus=False, min_sharpness=None, segment=False, seg_margin=None, core_thres=None,
                    min_area=None, spatial_radii=None, **detect_region_kwargs):
    """What a slide carries: :func:`detect_region`, then per class the count map, the tissue of every map cell and the densest fields.

    1. Runs ``detect_region(model, raster, **detect_region_kwargs)`` unchanged and concatenates its ``(ty, tx, boxes)`` result in
       that order into ``rows`` [M,7], as :func:`evaluate_region` does.
    2. The tissue map on the grid ``tile_grid(H, W, cell)``, in pixels of the (halved) slide, with the ``bg_level``, ``shrink`` and
       ``probe_stride`` (= d, default 16; it must divide ``cell``) among the keyword arguments.  ``probe_stride=1`` counts on the
       raster itself and is EXACT (THE TISSUE RULE, at the cost of one more upload of the slide).  Any other stride counts the
       tissue pixels of :func:`probe_view` (every d-th pixel, single source pixels, no averaging) and multiplies by ``d * d``: an
       ESTIMATE.  It is a multiple of ``d * d``, a cell on the slide's ragged edge can get up to ``d - 1`` rows and columns more
       than it holds, and tissue thinner than d pixels is seen by chance; over a field of ``field * cell`` pixels these errors
       are small against ``field_min_tissue``, per cell they need not be, and densities of single cells inherit them.
    3. ``burden_map(rows, (H, W), cell, C, min_conf)`` (C = the model's classes) and ``densest_fields(counts, tissue, field, top_k,
       need_tissue)`` with ``need_tissue = max(1, ceil(field_min_tissue * (field * cell)**2))``, computed once on the host like
       :func:`wanted_tiles`' bound.  ``field * cell <= 46340``.
    4. Returns a dict: ``rows``; ``counts`` int32 [C,Gy,Gx] on the device; ``tissue`` NumPy int32 [Gy,Gx]; ``fields`` NumPy int64
       [C,top_k,5] = (y0, x0, side, count, tissue_px) in pixels of the (halved) slide, in pick order, rows not filled -1;
       ``n_found`` [C]; ``totals`` [C] (rows counted per class); ``below``, ``flagged``, ``flags`` of :func:`burden_map`.  With
       ``mpp`` (microns per pixel of the halved slide) also ``density_per_mm2`` float64 [C,Gy,Gx], ``total_density_per_mm2`` [C]
       (``totals`` over the tissue of the whole map) and ``field_density_per_mm2`` [C,top_k]: ``count / (tissue_px * mpp**2 * 1e-6)``
       in float64 on the host, NaN where there is no tissue (and for rows not filled).

    5. With ``stain_stats`` (a :class:`StainStats` of this slide, :func:`stain_stats`) and ``dab_thres`` (an optical density) both
       given, also ``dab_positive_fraction`` = ``stain_stats.positive_fraction(1, dab_thres)[0]``, the share of tissue pixels whose
       stain-1 (DAB) concentration reaches the threshold (the classical "amyloid load"), and ``dab_thres`` as it took effect (a
       multiple of 1/64).  Host arithmetic on the histogram; nothing else changes, and without the two arguments the result has
       the keys it had.  A ``stain=`` among the keyword arguments reaches :func:`detect_region`; its basis must be the statistics'.
       A slide's own vectors need no argument of their own: ``est = estimate_basis(raster)``, ``stain_stats(raster,
       basis=est.basis)`` here and, for normalisation, ``stain=StainMap(stats, target, remix=True)``, whose ``basis`` is the
       source's; ``load=`` and ``segment=`` then unmix on the estimated basis by the precedence of item 6.

    6. With ``load=True`` (``dab_thres`` is then required, ``stain_stats`` stays optional; ``cell >= 16``) one more pass over the
       raster, ``stain_load(raster, rows, cell, shrink, bg_level, dab_thres, 1, basis)`` -- exact and at full resolution whatever
       ``probe_stride`` is; the basis is the statistics', else the ``stain=`` map's, else ``H_DAB`` -- adds ``load_tissue`` and
       ``load_positive`` int64 [Gy,Gx], ``load_map`` (their ratio, NaN without tissue), ``total_load``, ``box_load`` int64 [M,4] =
       (pixels, tissue, positive, bin_sum) for ``rows`` (:func:`box_morphometry` makes areas of it) and ``field_load`` float64
       [C,top_k]: positive over tissue, summed on the host over the cells of every picked field, NaN for rows not filled and for a
       field without tissue.  The threshold applies to the slide's own concentrations, with or without a ``stain=`` map.

    7. With ``focus=True`` (``cell >= 16``) one more pass over the raster, ``focus_map(raster, rows, cell, shrink, bg_level)`` -- THE
       FOCUS RULE, exact and at full resolution -- adds ``focus_n`` int64 and ``focus_sharpness`` float64 [Gy,Gx], ``box_sharpness``
       float64 [M] for ``rows`` and ``field_sharpness`` float64 [C,top_k]: the pooled variance of the Laplacian from the summed ``n``,
       ``s1``, ``s2`` of the cells of every picked field, NaN for rows not filled and for a field without an evaluated pixel.  Every
       count and load above assumes the scanner was in focus where it counted; these say where it was.  With ``min_sharpness`` (only
       with ``focus=True``; no default is offered, see :func:`focus_summary`) also ``in_focus`` bool [Gy,Gx] and
       ``in_focus_fraction``.  The fields are picked as before: sharpness is reported, never used.  Without ``focus`` the result has
       the keys it had.

    8. With ``segment=True`` (``dab_thres`` is then required, as for ``load=True``; the basis by the same precedence) one more pass,
       ``segment_boxes(raster, rows, seg_margin, shrink, bg_level, dab_thres, core_thres, 1, basis, min_area)`` (``seg_margin``
       default 8, ``core_thres`` default None, ``min_area`` default 1; any of them without ``segment=True`` is a ``ValueError``) --
       THE SEGMENT RULE; only the strips that hold a detection's window are uploaded -- adds ``segments`` int32 [M,20] and
       ``segment_flags``, ``plaque`` (:func:`plaque_morphometry` of them, with ``mpp`` and the slide's sides) and ``class_area_px``
       float64 [C,3]: the quartiles (25, 50, 75 %) of ``area_px`` per class over the rows with ``conf >= min_conf`` and a selected
       component, NaN for a class without one.  The segments are reported, never used: no detection is moved, re-scored or dropped.
       Without ``segment`` the result has the keys it had.

    9. With ``spatial_radii`` (a sequence of radii in pixels of the (halved) slide; at most 8 classes) also ``spatial`` =
       ``spatial_stats(rows, (H, W), spatial_radii, C, min_conf, area=tissue.sum(), mpp=mpp)``: the cross-class pair counts within
       every radius, Ripley's K and L, the pair correlation g and the nearest-neighbour distribution G over the whole slide, with the
       tissue pixels as the area (THE PAIR RULE; see :func:`spatial_stats` for what a ragged tissue outline does to K).  The
       arguments are checked before any launch.  Without it the result has the keys it had.

    The numbers are counts and areas; mapping them to CERAD categories is a clinical choice and not made here."""
    if not segment and not (seg_margin is None and core_thres is None and min_area is None):
        raise ValueError("quantify_region: seg_margin, core_thres and min_area need segment=True")
    if min_sharpness is not None:
        if not focus:
            raise ValueError("quantify_region: min_sharpness needs focus=True")
        if isinstance(min_sharpness, bool) or not 0.0 <= float(min_sharpness) < math.inf:
            raise ValueError(f"quantify_region: min_sharpness {min_sharpness!r} is no variance >= 0")
    if load:
        if dab_thres is None:
            raise ValueError("quantify_region: load=True needs dab_thres")
        _thres_bin(dab_thres, "quantify_region")
    elif segment:
        if dab_thres is None:
            raise ValueError("quantify_region: segment=True needs dab_thres")
    elif (stain_stats is None) != (dab_thres is None):
        raise ValueError("quantify_region: stain_stats and dab_thres go together")
    if stain_stats is not None:
        if not isinstance(stain_stats, StainStats):
            raise ValueError(f"quantify_region: stain_stats must be a wsi.StainStats, got {type(stain_stats).__name__}")
        stain_stats.positive_fraction(1, dab_thres)       # a bad threshold is refused before any launch
        st = detect_region_kwargs.get("stain")
        if isinstance(st, StainMap) and st.basis != stain_stats.basis:
            raise ValueError("quantify_region: stain and stain_stats were made on different bases")
    cell = _whole(cell, 1, BURDEN_MAX_FIELD_SIDE, "quantify_region: cell")
    F = _whole(field, 1, BURDEN_MAX_FIELD_SIDE, "quantify_region: field")
    K = _whole(top_k, 1, BURDEN_MAX_FIELDS, "quantify_region: top_k")
    if F * cell > BURDEN_MAX_FIELD_SIDE:
        raise ValueError(f"quantify_region: field * cell = {F * cell} exceeds {BURDEN_MAX_FIELD_SIDE} (a field's tissue must fit int32)")
    if not 0.0 <= float(field_min_tissue) <= 1.0:       # a NaN fails both comparisons
        raise ValueError(f"quantify_region: field_min_tissue {field_min_tissue!r} is no fraction of a field")
    if mpp is not None and not 0.0 < float(mpp) < math.inf:
        raise ValueError(f"quantify_region: mpp {mpp!r} is no positive number of microns per pixel")
    d = int(detect_region_kwargs.get("probe_stride", 16))
    if d < 1 or cell % d:
        raise ValueError(f"quantify_region: probe_stride {d} must divide cell {cell}")
    shrink, bg_level = int(detect_region_kwargs.get("shrink", 1)), detect_region_kwargs.get("bg_level", 220)
    if getattr(raster, "ndim", 0) != 3 or raster.shape[0] // shrink < 1 or raster.shape[1] // shrink < 1:
        raise ValueError("quantify_region: raster must be a uint8 [H,W,3] array with at least one (halved) pixel")
    if load:        # refused before any launch, like everything above
        st = detect_region_kwargs.get("stain")
        load_basis = stain_stats.basis if stain_stats is not None else st.basis if isinstance(st, StainMap) else H_DAB
        _check_load("quantify_region", raster, shrink, cell, bg_level, 1, load_basis)
    if focus:
        _check_focus("quantify_region", raster, shrink, cell, bg_level)
    if segment:
        st = detect_region_kwargs.get("stain")
        seg_basis = stain_stats.basis if stain_stats is not None else st.basis if isinstance(st, StainMap) else H_DAB
        seg_margin, min_area = 8 if seg_margin is None else seg_margin, 1 if min_area is None else min_area
        _check_segment("quantify_region", raster, shrink, bg_level, dab_thres, core_thres, 1, seg_basis, seg_margin, min_area)
    min_conf = float(min_conf)
    need = max(1, math.ceil(float(field_min_tissue) * (F * cell) ** 2))
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    if spatial_radii is not None:       # refused before any launch (and before the model is touched), like everything above
        _check_spatial("quantify_region", (H, W), spatial_radii, 1, None, None)
    num_classes = int(model.yolo_layers[0].num_classes)
    if spatial_radii is not None:
        _whole(num_classes, 1, PAIR_MAX_CLASSES, "quantify_region: the model's classes (spatial statistics)")
    res = detect_region(model, raster, **detect_region_kwargs)
    rows = torch.cat([r for _, _, r in res]) if res else torch.zeros(0, 7)
    if d == 1:
        tissue = tissue_counts(raster, cell, shrink, 0, bg_level)
    else:
        view, t, _ = probe_view(raster, cell, shrink, 0, d)
        tissue = tissue_counts(view, t, 1, 0, bg_level) * np.int32(d * d)
    bm = burden_map(rows, (H, W), cell, num_classes, min_conf)
    picked, n_found = densest_fields(bm["counts"], tissue, F, K, need)
    fields = np.full((num_classes, K, 5), -1, np.int64)
    filled = picked[:, :, 0] >= 0
    fields[filled] = np.stack([picked[:, :, 0].astype(np.int64) * cell, picked[:, :, 1].astype(np.int64) * cell,
                               np.full(picked.shape[:2], F * cell, np.int64), picked[:, :, 2], picked[:, :, 3]], 2)[filled]
    out = {"rows": rows, "counts": bm["counts"], "tissue": tissue, "fields": fields, "n_found": n_found, "totals": bm["counted"],
           "below": bm["below"], "flagged": bm["flagged"], "flags": bm["flags"]}
    if stain_stats is not None:
        out["dab_positive_fraction"], out["dab_thres"] = stain_stats.positive_fraction(1, dab_thres)
    if load:
        ld = stain_load(raster, rows, cell, shrink, bg_level, dab_thres, 1, load_basis)
        out["load_tissue"], out["load_positive"], out["load_map"] = ld["tissue"], ld["positive"], ld["load"]
        out["total_load"], out["box_load"] = ld["total_load"], ld["boxes"]
        out["field_load"] = np.full((num_classes, K), np.nan)
        for c, k, (t, p) in _field_sums(picked, filled, F, (ld["tissue"], ld["positive"])):
            if t:
                out["field_load"][c, k] = float(p) / t
    if focus:
        fm = focus_map(raster, rows, cell, shrink, bg_level)
        out["focus_n"], out["focus_sharpness"], out["box_sharpness"] = fm["n"], fm["sharpness"], fm["box_sharpness"]
        out["field_sharpness"] = np.full((num_classes, K), np.nan)
        for c, k, (n, s1, s2) in _field_sums(picked, filled, F, (fm["n"], fm["s1"], fm["s2"])):
            if n:
                out["field_sharpness"][c, k] = s2 / n - (s1 / n) ** 2
        if min_sharpness is not None:
            fs = focus_summary(fm, None, min_sharpness)
            out["in_focus"], out["in_focus_fraction"] = fs["in_focus"], fs["in_focus_fraction"]
    if segment:
        sg = segment_boxes(raster, rows, seg_margin, shrink, bg_level, dab_thres, core_thres, 1, seg_basis, min_area)
        out["segments"], out["segment_flags"] = sg["segments"], sg["flags"]
        out["plaque"] = plaque_morphometry(sg["segments"], mpp, (H, W))
        out["class_area_px"] = np.full((num_classes, 3), np.nan)
        r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
        with np.errstate(invalid="ignore"):
            counted = (r[:, 4] >= min_conf) & np.isfinite(out["plaque"]["area_px"])
        for c in range(num_classes):
            a = out["plaque"]["area_px"][counted & (r[:, 6] == c)]
            if len(a):
                out["class_area_px"][c] = np.percentile(a, [25.0, 50.0, 75.0])
    if spatial_radii is not None:
        out["spatial"] = spatial_stats(rows, (H, W), spatial_radii, num_classes, min_conf, area=int(tissue.sum(dtype=np.int64)), mpp=mpp)
    if mpp is not None:
        mm2 = lambda px: np.where(px > 0, px, np.nan).astype(np.float64) * float(mpp) ** 2 * 1e-6      # NaN where there is no tissue
        out["density_per_mm2"] = bm["counts"].cpu().numpy().astype(np.float64) / mm2(tissue)[None]
        out["total_density_per_mm2"] = bm["counted"].astype(np.float64) / mm2(np.int64(tissue.sum(dtype=np.int64)))
        out["field_density_per_mm2"] = np.where(filled, fields[:, :, 3], 0).astype(np.float64) / mm2(np.where(filled, fields[:, :, 4], 0))
    return out


# ---- spatial statistics: pair counts within a radius, Ripley's K and L, g, nearest neighbours ----------------------------------------
PAIR_MAX_CLASSES, PAIR_MAX_RADII, PAIR_MAX_RADIUS_Q, PAIR_MAX_SIDE = 8, 32, 32767, 1 << 21      # include/amyloid_yolo.h, THE PAIR RULE


def spatial_radii_q(radii):
    """radii in pixels -> int32 ``R_k = floor(4 r_k)`` quarter pixels; ``ValueError`` unless they are 1 .. 32 finite values whose
    ``R_k`` ascend strictly inside 1 .. 32767 (radii that collapse onto one quarter pixel do not)"""
    try:
        r = np.asarray(radii, np.float64).reshape(-1) if not isinstance(radii, (str, bytes)) and np.ndim(radii) == 1 else None
    except (TypeError, ValueError):
        r = None
    if r is None or not 1 <= len(r) <= PAIR_MAX_RADII or not np.isfinite(r).all():
        raise ValueError(f"spatial radii {radii!r}: need a sequence of 1 .. {PAIR_MAX_RADII} finite radii in pixels")
    q = np.floor(4.0 * r)
    if q[0] < 1 or q[-1] > PAIR_MAX_RADIUS_Q or (np.diff(q) <= 0).any():
        raise ValueError(f"spatial radii {radii!r}: floor(4 r) = {q.tolist()} must ascend strictly inside 1 .. {PAIR_MAX_RADIUS_Q} "
                         "(radii below a quarter pixel apart collapse onto one another)")
    return q.astype(np.int32)


def spatial_roi_q(roi, slide_hw):
    """``roi`` = (x1, y1, x2, y2) in pixels -> int32 (ceil(4 x1), ceil(4 y1), floor(4 x2), floor(4 y2)) clipped to the positions
    0 .. 4W-1, 0 .. 4H-1 of the slide: the quarter-pixel positions inside the closed rectangle.  None is the whole slide.
    ``ValueError`` if no position is left."""
    H, W = slide_hw
    if roi is None:
        return np.array([0, 0, 4 * W - 1, 4 * H - 1], np.int32)
    try:
        v = np.asarray(roi, np.float64).reshape(-1)
    except (TypeError, ValueError):
        v = np.zeros(0)
    if len(v) != 4 or not np.isfinite(v).all():
        raise ValueError(f"spatial roi {roi!r}: need (x1, y1, x2, y2), finite, in pixels")
    q = [max(math.ceil(4.0 * v[0]), 0), max(math.ceil(4.0 * v[1]), 0), min(math.floor(4.0 * v[2]), 4 * W - 1), min(math.floor(4.0 * v[3]), 4 * H - 1)]
    if q[0] > q[2] or q[1] > q[3]:
        raise ValueError(f"spatial roi {roi!r} holds no position of the {H} x {W} slide")
    return np.array(q, np.int32)


def _check_spatial(what, slide_hw, radii, num_classes, roi, area, mpp=None):
    """the host checks of :func:`spatial_stats` -> (H, W, C, radii_q, roi_q, area)"""
    if slide_hw is None or isinstance(slide_hw, (str, bytes)) or np.ndim(slide_hw) != 1 or len(slide_hw) != 2:
        raise ValueError(f"{what}: slide_hw {slide_hw!r} is no (H, W)")
    H, W = (_whole(v, 1, PAIR_MAX_SIDE, f"{what}: slide_hw") for v in slide_hw)
    nc = _whole(num_classes, 1, PAIR_MAX_CLASSES, f"{what}: num_classes (spatial statistics)")
    rq = spatial_radii_q(radii)
    roi_q = spatial_roi_q(roi, (H, W))
    if area is None:
        area = float(int(roi_q[2]) - int(roi_q[0]) + 1) * float(int(roi_q[3]) - int(roi_q[1]) + 1) / 16.0
    elif isinstance(area, bool) or not 0.0 <= float(area) < math.inf:
        raise ValueError(f"{what}: area {area!r} is no area >= 0 in square pixels")
    if mpp is not None and (isinstance(mpp, bool) or not 0.0 < float(mpp) < math.inf):
        raise ValueError(f"{what}: mpp {mpp!r} is no positive number of microns per pixel")
    return H, W, nc, rq, roi_q, float(area)


def pair_counts_device(rows, slide_hw, radii_q, num_classes, min_conf=0.0, roi_q=None, border=True, cell_side_q=0):
    """``ay_pair_counts`` on rows that live on the device (float32 [M,7], contiguous) -> a dict of int tensors on the device, all views
    of ONE buffer ``buf`` (so that a caller reads back once): ``pairs`` int64 [C,C,B], ``centres`` int32 [C,B], ``stats`` int32
    [2C+3], ``bd`` int32 [M], ``nn`` int32 [M,C,2], and ``label`` int32 [M], the rows' ``cls_pred`` as integers (a torch copy, for
    the host formulas).  Launches only: nothing is read back here.  ``cell_side_q`` overrides the grid's
    cell side (quarter pixels, at least the largest radius); the result does not depend on it."""
    H, W = slide_hw
    M, nc = int(rows.shape[0]), int(num_classes)
    rq = np.ascontiguousarray(radii_q, np.int32)
    B = len(rq)
    L = _lib.lib()
    sizes = [2 * nc * nc * B, nc * B, 2 * nc + 3, M, 2 * M * nc, M]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in sizes])])       # every piece starts on 16 bytes
    buf = torch.empty(max(int(offs[-1]), 4), device=rows.device, dtype=torch.int32)
    piece = [buf[int(o):int(o) + n] for o, n in zip(offs[:-1], sizes)]
    out = {"buf": buf, "pairs": piece[0].view(torch.int64).view(nc, nc, B), "centres": piece[1].view(nc, B), "stats": piece[2], "bd": piece[3],
           "nn": piece[4].view(M, nc, 2), "label": piece[5]}
    if M:       # cls_pred as an integer next to the outputs (a value that is no class becomes -1 or a number no class has)
        out["label"].copy_(torch.nan_to_num(rows[:, 6], nan=-1.0, posinf=-1.0, neginf=-1.0).clamp(-1.0, 255.0))
    need = int(L.ay_pair_counts_workspace_bytes(M, H, W, int(rq[-1]) if B else 0, int(cell_side_q)))
    ws = torch.empty(max(need, 16), device=rows.device, dtype=torch.uint8)
    i32p = C.POINTER(C.c_int32)
    roi_arg = None if roi_q is None else np.ascontiguousarray(roi_q, np.int32).ctypes.data_as(i32p)
    check(L.ay_pair_counts(ptr(rows) if M else None, M, nc, H, W, C.c_float(min_conf), rq.ctypes.data_as(i32p), B, roi_arg, int(bool(border)),
                           int(cell_side_q), ptr(out["pairs"]), ptr(out["centres"]), ptr(out["nn"]) if M else None, ptr(out["bd"]) if M else None,
                           ptr(out["stats"]), ptr(ws), need, _lib.stream_ptr()), "ay_pair_counts")
    return out


def spatial_summaries(pairs, centres, inside, bd, nn, radii_q, area, mpp=None, labels=None):
    """The host formulas of :func:`spatial_stats`, float64, NaN wherever a denominator is 0.  ``labels`` int [M]: the class of every
    counted row (-1: not counted), needed for ``G``."""
    pairs, centres, inside = np.asarray(pairs, np.float64), np.asarray(centres, np.float64), np.asarray(inside, np.float64)
    rq = np.asarray(radii_q, np.int64)
    r = rq / 4.0
    nc, B = centres.shape
    with np.errstate(all="ignore"):
        intensity = inside / area if area > 0 else np.full(nc, np.nan)
        den = centres[:, None, :] * intensity[None, :, None]
        K = np.where(den > 0, pairs / den, np.nan)
        Lf = np.sqrt(K / math.pi)
        prev_K = np.concatenate([np.zeros((nc, nc, 1)), K[:, :, :-1]], 2)
        prev_r = np.concatenate([[0.0], r[:-1]])
        g = (K - prev_K) / (math.pi * (r ** 2 - prev_r ** 2))
        G = np.full((nc, nc, B), np.nan)
        bd, nn = np.asarray(bd), np.asarray(nn)
        for a in range(nc):
            mine = labels == a
            for k in range(B):
                sel = mine & (bd >= rq[k])
                if sel.any():
                    d2 = nn[sel, :, 0].astype(np.int64)
                    G[a, :, k] = ((d2 >= 0) & (d2 <= rq[k] * rq[k])).mean(0)
    out = {"intensity": intensity, "K": K, "L": Lf, "L_minus_r": Lf - r, "g": g, "G": G}
    if mpp is not None:
        out["radii_um"], out["K_um2"] = r * float(mpp), K * float(mpp) ** 2
    return out


def spatial_stats(rows, slide_hw, radii, num_classes=2, min_conf=0.0, roi=None, border=True, area=None, mpp=None):
    """Spatial statistics of a slide's detections (``ay_pair_counts``, THE PAIR RULE in ``include/amyloid_yolo.h``): the cross-class
    pair counts within every radius, and Ripley's K and L, the pair correlation g and the nearest-neighbour distribution G from them.

    ``rows`` [M,7] as :func:`burden_map` takes them; ``slide_hw`` = (H, W), each at most 2**21; ``num_classes`` = C in 1 .. 8.  A row
    is counted under THE BURDEN RULE's tests (``conf >= min_conf``, a finite centre, a class in 0 .. C-1) and stands at the quarter
    pixel of its centre.  ``radii`` are in pixels: ``R_k = floor(4 r_k)`` quarter pixels, 1 .. 32 of them, strictly ascending after
    the conversion and at most 8191.75 px (``ValueError`` otherwise); the effective radii ``R_k / 4`` are returned.  ``roi`` =
    (x1, y1, x2, y2) in pixels is the window: it becomes (ceil(4 x1), ceil(4 y1), floor(4 x2), floor(4 y2)), clipped to the slide; None
    is the whole slide.  With ``border=True`` (minus-sampling) a row is a centre at radius k only if it lies at least ``R_k`` inside
    the window, so that its whole disc was observed; its partners may lie anywhere.  ``border=False`` takes every row inside the
    window as a centre at every radius.  One call, one read-back.

    Returns a dict.  Raw: ``pairs`` int64 [C,C,B] (ordered pairs, cumulative in k: over the eligible centres of class a, the
    counted rows of class b within ``r_k``, the centre itself excluded), ``centres`` int32 [C,B], ``nn`` int32 [M,C,2] = (d2 in
    quarter pixels squared, row index) of the nearest counted row of every class within the largest radius, ties to the lowest
    index, -1 where there is none, ``nn_index`` int32 [M,C], ``nn_distance`` float64 [M,C] in pixels (NaN where there is none),
    ``bd`` int32 [M] (quarter pixels to the window's border, -1 outside and for rows not counted), ``counted`` and ``inside`` [C],
    ``below``, ``flagged``, ``flags``, ``radii`` (effective, px), ``radii_q``, ``roi_q``, ``area``.  Derived, float64 on the host, NaN
    wherever a denominator is 0: ``intensity[b] = inside[b] / area`` (``area`` in px**2; default: the window's; callers pass
    tissue pixels), ``K[a,b,k] = pairs / (centres[a,k] * intensity[b])``, ``L = sqrt(K / pi)``, ``L_minus_r``, ``g[k] = (K_k -
    K_{k-1}) / (pi (r_k**2 - r_{k-1}**2))`` with ``K_{-1} = r_{-1} = 0``, and ``G[a,b,k]``: the share of the class-a rows with
    ``bd >= R_k`` whose nearest b lies within ``r_k``.  With ``mpp`` also ``radii_um`` and ``K_um2``.  Under complete spatial
    randomness ``K = pi r**2``, ``L - r = 0`` and ``g = 1``; clustering at a scale shows as larger values there.

    Two limits.  The window is a RECTANGLE: with ``area=`` tissue pixels on a slide whose tissue outline is ragged, centres near a
    tissue edge have part of their disc over glass, and K is biased low there.  Comparing ``K[a][b]`` with ``K[a][a]`` on the same
    slide, or working inside a field (``roi=``) that is all tissue, is the robust use.  And the COST is the number of pairs within
    3 x 3 grid cells of side ``r_max``: quadratic in ``r_max`` at a given density.

    Out of scope: Monte-Carlo envelopes (random relabelling of the classes is the natural follow-up), per-field statistics (pass a
    field as ``roi=``) and windows that are no rectangles."""
    H, W, nc, rq, roi_q, area = _check_spatial("spatial_stats", slide_hw, radii, num_classes, roi, area, mpp)
    if rows is None or len(rows.shape) != 2 or rows.shape[1] != 7:
        raise ValueError(f"spatial_stats: rows must be [M,7], got {None if rows is None else tuple(rows.shape)}")
    min_conf = float(min_conf)
    from .stats import _slide_array
    dev = _burden_device()
    rows = _slide_array(rows, 7, dev)
    M = int(rows.shape[0])
    dv = pair_counts_device(rows, (H, W), rq, nc, min_conf, roi_q, border)
    host = dv["buf"].cpu()                                              # the one read-back
    off = lambda t: (t.data_ptr() - dv["buf"].data_ptr()) // 4
    take = lambda t: host[off(t):off(t) + t.numel() * t.element_size() // 4]
    pairs = take(dv["pairs"]).view(torch.int64).view(nc, nc, len(rq)).numpy().copy()
    centres, st = take(dv["centres"]).view(nc, len(rq)).numpy().copy(), take(dv["stats"]).numpy().copy()
    bd, nn = take(dv["bd"]).numpy().copy(), take(dv["nn"]).view(M, nc, 2).numpy().copy()
    d2 = nn[:, :, 0].astype(np.float64)
    labels = np.where(bd >= 0, take(dv["label"]).numpy(), -1)          # G asks rows with bd >= R_k >= 1 only: those are counted
    out = {"pairs": pairs, "centres": centres, "nn": nn, "nn_index": nn[:, :, 1].copy(), "nn_distance": np.where(d2 >= 0, np.sqrt(np.abs(d2)) / 4.0, np.nan),
           "bd": bd, "counted": st[:nc].copy(), "inside": st[nc:2 * nc].copy(), "below": int(st[2 * nc]), "flagged": int(st[2 * nc + 1]),
           "flags": int(st[2 * nc + 2]), "radii": rq / 4.0, "radii_q": rq, "roi_q": roi_q, "area": area}
    out.update(spatial_summaries(pairs, centres, out["inside"], bd, nn, rq, area, mpp, labels))
    return out


# ---- stain normalisation: H/DAB statistics, gains, the colour map of the cut ------------------------------------------------------
STAIN_BINS = 512        # include/amyloid_yolo.h, THE STAIN RULE: bins of 1/64 OD


class StainBasis:
    """Two stain OD vectors (R, G, B), each normalised to unit length; ``M`` (float64 3x3) has them as rows 0 and 1 and their
    normalised cross product as row 2 (THE STAIN RULE, ``include/amyloid_yolo.h``).  ``ValueError`` for vectors that are not three
    finite numbers, of length 0, or (nearly) parallel: the basis would be singular."""

    def __init__(self, stain0, stain1):
        rows = []
        for v in (stain0, stain1):
            v = np.asarray(v, np.float64).reshape(-1)
            if v.shape != (3,) or not np.isfinite(v).all() or not np.linalg.norm(v) > 0:
                raise ValueError(f"StainBasis: a stain vector is three finite numbers, not all 0 (got {v!r})")
            rows.append(v / np.linalg.norm(v))
        cross = np.cross(rows[0], rows[1])
        if not np.linalg.norm(cross) > 1e-6:
            raise ValueError("StainBasis: the two stain vectors are parallel: the basis is singular")
        self.M = np.stack([rows[0], rows[1], cross / np.linalg.norm(cross)])
        self.M.setflags(write=False)

    @classmethod
    def of_unit_vectors(cls, stain0, stain1):
        """the basis whose rows 0 and 1 are exactly the two given unit vectors (they are checked and not divided again)"""
        self = cls(stain0, stain1)
        rows = [np.asarray(v, np.float64).reshape(3) for v in (stain0, stain1)]
        if not all(abs(np.linalg.norm(v) - 1.0) < 1e-12 for v in rows):
            raise ValueError("StainBasis.of_unit_vectors: a vector is not of unit length")
        cross = np.cross(rows[0], rows[1])
        self.M = np.stack([rows[0], rows[1], cross / np.linalg.norm(cross)])
        self.M.setflags(write=False)
        return self

    def __eq__(self, other):
        return isinstance(other, StainBasis) and np.array_equal(self.M, other.M)

    def __hash__(self):
        return hash(self.M.tobytes())

    def __repr__(self):
        return f"StainBasis({tuple(self.M[0])}, {tuple(self.M[1])})"


H_DAB = StainBasis((0.650, 0.704, 0.286), (0.268, 0.570, 0.776))     # Ruifrok & Johnston: hematoxylin, DAB


def stain_tables(basis, gains=(1.0, 1.0), target_basis=None):
    """The tables of THE STAIN RULE, built in float64 and rounded to fp32 once -> ``_lib.StainParams`` (host).  With ``target_basis``
    the concentrations unmixed on ``basis`` are mixed again on the target's vectors: ``A = inv(M) . diag(g0, g1, 1) . M_target``; ``D``
    stays ``basis``' own.  The device reads ``A`` as a table and needs no change for it."""
    v = np.arange(256, dtype=np.float64)
    Minv = np.linalg.inv(basis.M)
    A = Minv @ np.diag([float(gains[0]), float(gains[1]), 1.0]) @ (basis if target_basis is None else target_basis).M
    k = np.arange(257, dtype=np.float64)
    T = (256.0 * 10.0 ** (-k / 64.0) - 1.0) / 255.0
    tabs = [(-np.log10((v + 1.0) / 256.0)), Minv.reshape(-1), A.reshape(-1), T]
    if not all(np.isfinite(t).all() and np.isfinite(t.astype(np.float32)).all() for t in tabs):
        raise ValueError("stain_tables: the basis and gains give tables that are not finite in fp32")
    p = _lib.StainParams()
    for name, t in zip(("od", "D", "A", "T"), tabs):
        getattr(p, name)[:] = t.astype(np.float32).tolist()
    return p


def _params_to_device(p, dev):
    host = torch.from_numpy(np.frombuffer(bytes(p), dtype=np.uint8).copy())
    return host.to(dev)


class StainStats:
    """Histograms of the two stain concentrations over the tissue pixels of a slide (:func:`stain_stats`): ``hist`` int64 ``[2,
    512]`` in bins of 1/64 OD (``hist[s, b]``: pixels with ``b / 64 <= c_s < (b + 1) / 64``, negative concentrations in bin 0, those
    from 8 OD on in bin 511), ``n_tissue`` (every row of ``hist`` sums to it) and the ``basis`` they were unmixed on."""

    def __init__(self, hist, n_tissue, basis=H_DAB):
        hist = np.asarray(hist)
        if hist.shape != (2, STAIN_BINS) or hist.dtype.kind not in "iu" or (hist < 0).any():
            raise ValueError(f"StainStats: hist must be [2, {STAIN_BINS}] non-negative integers")
        if not isinstance(basis, StainBasis):
            raise ValueError("StainStats: basis must be a wsi.StainBasis")
        self.hist, self.n_tissue, self.basis = hist.astype(np.int64), int(n_tissue), basis
        if (self.hist.sum(1) != self.n_tissue).any():
            raise ValueError(f"StainStats: every row of hist must sum to n_tissue = {self.n_tissue}")

    def strength(self, p=99.0):
        """``(q0, q1)``: per stain the upper edge ``(b* + 1) / 64`` of the first bin whose cumulative count reaches ``K = max(1,
        ceil(p * n / 100))``, the ``p``-th percentile of its concentration over the tissue.  ``ValueError`` without tissue or for
        ``p`` outside (0, 100]."""
        p = float(p)
        if not 0.0 < p <= 100.0:       # a NaN fails both comparisons
            raise ValueError(f"StainStats.strength: p {p!r} outside (0, 100]")
        if self.n_tissue == 0:
            raise ValueError("StainStats.strength: no tissue pixel: a slide without tissue has no stain strength")
        K = max(1, math.ceil(p * self.n_tissue / 100.0))
        return tuple((int(np.searchsorted(np.cumsum(self.hist[s]), K, side="left")) + 1) / 64.0 for s in (0, 1))

    def positive_fraction(self, stain=1, thres=0.15):
        """``(share, j / 64)``: the share of tissue pixels whose concentration of ``stain`` (0 or 1) is at least ``j / 64``, ``j =
        round(thres * 64)``: the threshold moves to a bin edge and comes back as it took effect.  NaN without tissue."""
        if stain not in (0, 1):
            raise ValueError(f"StainStats.positive_fraction: stain {stain!r} is neither 0 nor 1")
        thres = float(thres)
        if not 0.0 <= thres < math.inf:
            raise ValueError(f"StainStats.positive_fraction: thres {thres!r} is no optical density >= 0")
        j = min(int(round(thres * 64.0)), STAIN_BINS)
        share = float(self.hist[stain, j:].sum()) / self.n_tissue if self.n_tissue else math.nan
        return share, j / 64.0


class StainMap:
    """The colour map that brings a slide's stain strengths to a target's (THE STAIN RULE): per stain the gain ``g_s = clip(t_s / q_s,
    1 / max_gain, max_gain)`` with ``(q0, q1) = source.strength(p)`` and ``(t0, t1)`` the target: a :class:`StainStats` (its
    ``strength(p)``; it must share the source's basis) or a pair of positive finite strengths, e.g.
    ``stain_stats(training_slide).strength()``.  There is no built-in target.  ``basis``, if given, must be the source's.
    ``gains`` is the pair; ``tables`` the host struct; ``params`` the struct on the current device, uploaded on first use.

    ``remix=True`` lifts the shared basis: the target is a :class:`StainStats` on ANY basis, or a pair of strengths plus
    ``target_basis=``, and the map unmixes on the source's basis and mixes again on the target's (:func:`stain_tables` with
    ``target_basis``): the step that carries a slide with its own estimated vectors (:func:`estimate_basis`) to a reference slide
    with other vectors.  The gains are taken as before, each strength on its own basis.  ``basis`` stays the source's -- what
    :func:`quantify_region` compares with the statistics' -- and ``target_basis`` is the basis mixed on (the source's without
    ``remix``).  With equal bases ``remix=True`` gives the tables of ``remix=False``."""

    def __init__(self, source, target, p=99.0, max_gain=4.0, basis=None, remix=False, target_basis=None):
        if not isinstance(source, StainStats):
            raise ValueError(f"StainMap: source must be a wsi.StainStats, got {type(source).__name__}")
        if basis is not None and basis != source.basis:
            raise ValueError("StainMap: basis differs from the basis of the source statistics")
        if target_basis is not None and not remix:
            raise ValueError("StainMap: target_basis needs remix=True")
        if target_basis is not None and not isinstance(target_basis, StainBasis):
            raise ValueError("StainMap: target_basis must be a wsi.StainBasis")
        max_gain = float(max_gain)
        if not 1.0 <= max_gain < math.inf:
            raise ValueError(f"StainMap: max_gain {max_gain!r} must be a finite number >= 1")
        q = source.strength(p)
        if isinstance(target, StainStats):
            if not remix and target.basis != source.basis:
                raise ValueError("StainMap: source and target statistics were made on different bases")
            if target_basis is not None and target_basis != target.basis:
                raise ValueError("StainMap: target_basis differs from the basis of the target statistics")
            t, target_basis = target.strength(p), target.basis if remix else None
        else:
            try:
                t = tuple(float(v) for v in target)
            except TypeError:
                raise ValueError(f"StainMap: target must be a wsi.StainStats or a pair of strengths, got {target!r}") from None
            if len(t) != 2 or not all(0.0 < v < math.inf for v in t):
                raise ValueError(f"StainMap: target strengths must be two positive finite numbers, got {target!r}")
        self._set(source.basis, tuple(min(max(ts / qs, 1.0 / max_gain), max_gain) for ts, qs in zip(t, q)), target_basis)
        self.source, self.target, self.p, self.max_gain = source, t, float(p), max_gain

    def _set(self, basis, gains, target_basis=None):
        self.basis, self.gains, self.target_basis = basis, gains, basis if target_basis is None else target_basis
        self.tables = stain_tables(basis, gains, target_basis)
        self._params = {}

    @classmethod
    def identity(cls, basis=H_DAB):
        """gains (1, 1) on ``basis``: the map that returns every uint8 value (for tests, and for the statistics' unmixing tables)"""
        if not isinstance(basis, StainBasis):
            raise ValueError("StainMap.identity: basis must be a wsi.StainBasis")
        self = cls.__new__(cls)
        self._set(basis, (1.0, 1.0))
        self.source, self.target, self.p, self.max_gain = None, None, None, None
        return self

    @property
    def params(self):
        if not torch.cuda.is_available():
            raise _lib.AyError("no HIP device: the stain map has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
        if dev not in self._params:
            self._params[dev] = _params_to_device(self.tables, dev)
        return self._params[dev]


def stain_stats(raster, shrink=1, bg_level=220, probe_stride=16, basis=H_DAB):
    """Stain statistics of a slide -> :class:`StainStats`: the two concentration histograms over its TISSUE pixels (THE TISSUE RULE
    with ``bg_level``), by ``ay_stain_hist_u8``.  The probe is :func:`tissue_mask`'s: every ``probe_stride``-th pixel of the (halved)
    slide, single source pixels (:func:`probe_view`); ``probe_stride=1`` is the exact rule, the 2x2 means of ``shrink=2`` included,
    at the cost of a full upload.  The strips of a :class:`StripStream` accumulate on the device; one read-back at the end."""
    bg_level, d = int(bg_level), int(probe_stride)
    if not 0 <= bg_level <= 256:
        raise ValueError(f"stain_stats: bg_level {bg_level} outside 0 .. 256")
    if d < 1:
        raise ValueError(f"stain_stats: probe_stride {d} must be at least 1")
    if not isinstance(basis, StainBasis):
        raise ValueError("stain_stats: basis must be a wsi.StainBasis")
    if d > 1:
        raster, shrink = probe_view(raster, d, shrink, 0, d)[0], 1
    params = StainMap.identity(basis).params
    T = min(1536, max(1, raster.shape[0] // shrink))
    strips = StripStream(raster, T, T, shrink)
    L = _lib.lib()
    hist = torch.zeros(2 * STAIN_BINS + 1, device=strips.dev, dtype=torch.int64)
    strips.each(lambda k, j, valid, width: check(
        L.ay_stain_hist_u8(*strips.args(k, valid, width), bg_level, ptr(params), ptr(hist), _lib.stream_ptr()), "ay_stain_hist_u8"))
    h = hist.cpu().numpy()
    return StainStats(h[:2 * STAIN_BINS].reshape(2, STAIN_BINS), h[2 * STAIN_BINS], basis)


def normalize_region(raster, stain, shrink=1, device=False):
    """The (halved) raster through the stain map, in THE STAIN RULE's uint8 form -> uint8 ``[H // shrink, W // shrink, 3]``: a NumPy
    array, or with ``device=True`` a tensor on the device (:class:`SlideSampler` reads device rasters in place: the way to train on
    normalised slides; also for a look at the result).  Strip by strip through ``ay_stain_apply_u8``."""
    if not isinstance(stain, StainMap):
        raise ValueError(f"normalize_region: stain must be a wsi.StainMap, got {type(stain).__name__}")
    if getattr(raster, "ndim", 0) != 3 or raster.shape[0] // shrink < 1 or raster.shape[1] // shrink < 1:
        raise ValueError("normalize_region: raster must be a uint8 [H,W,3] array with at least one (halved) pixel")
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    T = min(1536, H)
    strips = StripStream(raster, T, T, shrink)
    L = _lib.lib()
    params = stain.params
    out = torch.empty(H, W, 3, device=strips.dev, dtype=torch.uint8)

    def apply(k, j, valid, width):
        if valid // shrink:
            check(L.ay_stain_apply_u8(*strips.args(k, valid, width), ptr(params), ptr(out[j * T:]), W * 3, _lib.stream_ptr()),
                  "ay_stain_apply_u8")

    strips.each(apply)
    return out if device else out.cpu().numpy()


# ---- stain basis estimation: each slide's own two stain vectors ---------------------------------------------------------------------
BASIS_OD_SCALE, BASIS_OD_MAX, BASIS_MOMENT_WORDS, BASIS_DIR_BINS = 1024, 2466, 11, 512     # include/amyloid_yolo.h, THE BASIS RULE
BASIS_STRIP = 1536      # rows of the (halved) slide per strip of estimate_basis: stain_stats'


def basis_tables():
    """``odq`` of THE BASIS RULE, built in float64 -> ``_lib.StainBasisParams`` (host)"""
    v = np.arange(256, dtype=np.float64)
    p = _lib.StainBasisParams()
    p.odq[:] = np.rint(-np.log10((v + 1.0) / 256.0) * BASIS_OD_SCALE).astype(np.int64).tolist()
    return p


def _angle(a, b):
    """degrees between two unit vectors"""
    return math.degrees(math.acos(min(1.0, max(-1.0, float(np.dot(a, b))))))


def basis_plane(moments):
    """THE BASIS RULE's plane from the 11 words of ``ay_stain_moments_u8`` -> ``(eq1, eq2, eigenvalues)``: int32 ``[3]`` each and the
    three eigenvalues of the covariance of the integer optical density, largest first.  ``ValueError`` with fewer than 2 selected
    pixels or a second eigenvalue that is not positive: no stain plane."""
    m = [int(v) for v in moments]
    if len(m) != BASIS_MOMENT_WORDS:
        raise ValueError(f"basis_plane: moments are {BASIS_MOMENT_WORDS} words, got {len(m)}")
    n, S = m[1], m[2:5]
    if n < 2:
        raise ValueError(f"basis_plane: {n} selected pixel(s): a slide without stained tissue has no stain plane")
    cov, at = np.empty((3, 3), np.float64), 5
    for c in range(3):
        for d in range(c, 3):
            cov[c, d] = cov[d, c] = (n * m[at] - S[c] * S[d]) / (n * (n - 1))      # exact integers, divided once
            at += 1
    w, V = np.linalg.eigh(cov)                                                      # ascending
    if not w[1] > 0.0:
        raise ValueError("basis_plane: the optical densities of the selected pixels lie on a line: no stain plane")
    e1, e2 = V[:, 2], V[:, 1]
    if e1.sum() < 0.0:
        e1 = -e1
    if e2[int(np.argmax(np.abs(e2)))] < 0.0:
        e2 = -e2
    return np.rint(BASIS_OD_SCALE * e1).astype(np.int32), np.rint(BASIS_OD_SCALE * e2).astype(np.int32), tuple(float(x) for x in w[::-1])


def basis_vectors(hist, eq1, eq2, alpha=1.0, prior=None, max_angle=None):
    """THE BASIS RULE's two vectors from the direction histogram (the first 512 words of ``ay_stain_direction_hist_u8``'s) ->
    ``(vectors, angle_to_prior, fell_back)``: float64 ``[2, 3]`` unit vectors in the order of ``prior``'s stains (default ``H_DAB``),
    their angles to the prior's in degrees BEFORE the guard, and whether the guard replaced them (``max_angle=None``: never)."""
    prior = H_DAB if prior is None else prior
    h = np.asarray(hist).reshape(-1)[:BASIS_DIR_BINS].astype(np.int64)
    n = int(h.sum())
    if n == 0:
        raise ValueError("basis_vectors: no selected pixel on the half plane of the first direction")
    cum = np.cumsum(h)
    q1, q2 = np.asarray(eq1, np.float64), np.asarray(eq2, np.float64)
    ends = []
    for K in (max(1, math.ceil(alpha * n / 100.0)), max(1, math.ceil((100.0 - alpha) * n / 100.0))):
        d = (int(np.searchsorted(cum, K, side="left")) - BASIS_DIR_BINS // 2 + 0.5) / (BASIS_DIR_BINS // 2)
        v = (1.0 - abs(d)) * q1 + d * q2
        ends.append(v / np.linalg.norm(v))
    m0, m1 = prior.M[0], prior.M[1]
    if float(np.dot(ends[0], m1) + np.dot(ends[1], m0)) > float(np.dot(ends[0], m0) + np.dot(ends[1], m1)):
        ends.reverse()
    angles = (_angle(ends[0], m0), _angle(ends[1], m1))
    fell = tuple(max_angle is not None and a > max_angle for a in angles)
    return np.stack([prior.M[s] if fell[s] else ends[s] for s in (0, 1)]), angles, fell


class StainEstimate:
    """What :func:`estimate_basis` found: ``basis`` (a :class:`StainBasis`, ready for every ``basis=`` of this module) and ``vectors``
    float64 ``[2, 3]`` (its first two rows); ``moments`` int64 ``[11]`` and ``hist`` int64 ``[512]`` as the device summed them,
    ``n_tissue``, ``n_selected`` and ``outside`` (selected pixels with ``p1 <= 0``); ``plane`` = ``(eq1, eq2)`` int32 and
    ``eigenvalues`` (largest first); ``angle_to_prior`` (degrees, a pair, before the guard) and ``fell_back`` (bools, a pair: the
    guard put the prior's vector there); ``alpha`` and ``beta`` as they took effect (``beta`` a multiple of 1/1024)."""

    def __init__(self, moments, hist, alpha, beta_q, prior, max_angle):
        moments, hist = np.asarray(moments, np.int64), np.asarray(hist, np.int64)
        self.moments, self.hist = moments, hist[:BASIS_DIR_BINS].copy()
        self.n_tissue, self.n_selected, self.outside = int(moments[0]), int(moments[1]), int(hist[BASIS_DIR_BINS])
        eq1, eq2, self.eigenvalues = basis_plane(moments)
        self.plane = (eq1, eq2)
        self.vectors, self.angle_to_prior, self.fell_back = basis_vectors(self.hist, eq1, eq2, alpha, prior, max_angle)
        self.basis = StainBasis.of_unit_vectors(self.vectors[0], self.vectors[1])      # rows 0 and 1 are `vectors`, bit for bit
        self.alpha, self.beta = float(alpha), beta_q / BASIS_OD_SCALE


def _check_basis_args(beta, alpha, prior, max_angle):
    """the host checks of :func:`estimate_basis` -> (beta_q, alpha, max_angle)"""
    if not isinstance(prior, StainBasis):
        raise ValueError("estimate_basis: prior must be a wsi.StainBasis")
    beta, alpha = float(beta), float(alpha)
    if not 0.0 <= beta <= 2.4:             # a NaN fails both comparisons
        raise ValueError(f"estimate_basis: beta {beta!r} outside 0 .. 2.4 (optical density)")
    if not 0.0 < alpha < 50.0:
        raise ValueError(f"estimate_basis: alpha {alpha!r} outside (0, 50) per cent")
    if max_angle == "half":
        max_angle = 0.5 * _angle(prior.M[0], prior.M[1])
    elif max_angle is not None:
        if isinstance(max_angle, (bool, str)) or not 0.0 < float(max_angle) <= 90.0:
            raise ValueError(f"estimate_basis: max_angle {max_angle!r} outside (0, 90] degrees")
        max_angle = float(max_angle)
    return int(np.rint(beta * BASIS_OD_SCALE)), alpha, max_angle


def estimate_basis(raster, shrink=1, bg_level=220, probe_stride=16, beta=0.15, alpha=1.0, prior=H_DAB, max_angle="half"):
    """The slide's own two stain vectors -> :class:`StainEstimate`: a Macenko-style estimate (THE BASIS RULE in
    ``include/amyloid_yolo.h``), integers only on the device.  Over the tissue pixels whose integer optical density reaches ``beta``
    in every channel, pass 1 (``ay_stain_moments_u8``) sums the moments, the host takes the plane of the two largest eigenvalues,
    pass 2 (``ay_stain_direction_hist_u8``) counts the directions inside the plane, and the ``alpha``-th and ``(100 - alpha)``-th
    percentile directions are the two vectors, assigned to the stains of ``prior`` by the better pairing.

    The probe and the strips are :func:`stain_stats`': every ``probe_stride``-th pixel of the (halved) slide, single source pixels;
    ``probe_stride=1`` is the exact rule.  Each pass goes through one :class:`StripStream` and is read back once.  The result goes
    wherever a ``basis=`` is taken -- ``stain_stats(raster, basis=est.basis)``, :func:`stain_load`, :func:`segment_boxes` -- and,
    through the statistics, into ``StainMap(stats, target, remix=True)``.

    Guard: a vector further than ``max_angle`` degrees from its prior vector is replaced by the prior's and reported in
    ``fell_back``.  The default ``"half"`` is half the angle between the prior's two vectors (``H_DAB``: about 18.6), with which the two
    results can neither swap nor coincide; ``None`` disables the guard.

    LIMIT: the extreme on the DAB side is the ``alpha``-th percentile of the selected pixels.  On a slide whose DAB-positive share
    of selected pixels is below ``alpha`` per cent that extreme is not DAB; the guard catches it or the caller lowers ``alpha`` (on
    the synthetic slide of ``tests/stain_basis_reference.py`` with 0.4 % DAB, ``alpha=1`` lands 36 degrees off and ``alpha=0.1`` 3.6).

    ``ValueError`` before any launch for ``bg_level`` outside 0 .. 256, ``probe_stride < 1``, ``beta`` outside [0, 2.4], ``alpha``
    outside (0, 50), a ``prior`` that is no :class:`StainBasis`, ``max_angle`` outside (0, 90]; after pass 1 for a slide with fewer
    than 2 selected pixels or without a plane (one colour)."""
    bg_level, d = int(bg_level), int(probe_stride)
    if not 0 <= bg_level <= 256:
        raise ValueError(f"estimate_basis: bg_level {bg_level} outside 0 .. 256")
    if d < 1:
        raise ValueError(f"estimate_basis: probe_stride {d} must be at least 1")
    beta_q, alpha, max_angle = _check_basis_args(beta, alpha, prior, max_angle)
    resident = isinstance(raster, torch.Tensor)
    if getattr(raster, "ndim", 0) != 3 or raster.shape[2] != 3 or raster.dtype != (torch.uint8 if resident else np.uint8) or (
            resident and not raster.is_cuda):
        raise ValueError("estimate_basis: raster must be a uint8 [H,W,3] NumPy array or tensor on the device")
    if d > 1:
        raster, shrink = probe_view(raster, d, shrink, 0, d)[0], 1
    T = min(BASIS_STRIP, max(1, raster.shape[0] // shrink))
    L = _lib.lib()

    def one_pass(words, call):
        """``call(region, params, out)`` on every strip, adding to ``out``; one read-back"""
        if resident:                       # read in place, in the strips of the stream
            dev, rd = raster.device, raster.contiguous()
            rows = (rd.shape[0] // shrink) * shrink
            regions = ((ptr(rd[y:]), min(T * shrink, rows - y), rd.shape[1], rd.shape[1] * 3, shrink) for y in range(0, rows, T * shrink))
            each = lambda run: [run(region) for region in regions]
        else:
            strips = StripStream(raster, T, T, shrink)
            dev = strips.dev
            each = lambda run: strips.each(lambda k, j, valid, width: run(strips.args(k, valid, width)))
        with torch.cuda.device(dev):
            params = _params_to_device(basis_tables(), dev)
            out = torch.zeros(words, device=dev, dtype=torch.int64)
            each(lambda region: call(region, ptr(params), ptr(out)))
            return out.cpu().numpy()

    moments = one_pass(BASIS_MOMENT_WORDS, lambda region, params, out: check(
        L.ay_stain_moments_u8(*region, bg_level, beta_q, params, out, _lib.stream_ptr()), "ay_stain_moments_u8"))
    eq1, eq2, _ = basis_plane(moments)
    hist = one_pass(BASIS_DIR_BINS + 2, lambda region, params, out: check(
        L.ay_stain_direction_hist_u8(*region, bg_level, beta_q, *(int(v) for v in eq1), *(int(v) for v in eq2), params, out,
                                     _lib.stream_ptr()), "ay_stain_direction_hist_u8"))
    return StainEstimate(moments, hist, alpha, beta_q, prior, max_angle)


# ---- amyloid load: stain-positive area per map cell and per detection ---------------------------------------------------------------
LOAD_MIN_CELL, LOAD_MAX_SIDE, LOAD_FLAG_NONFINITE = 16, 1 << 24, 1       # include/amyloid_yolo.h, THE LOAD RULE
LOAD_MAX_CELLS = 1 << 26                                                 # 24 bytes per cell on the device


def _thres_bin(thres, what):
    """an optical density -> THE LOAD RULE's ``thres_bin``, as :meth:`StainStats.positive_fraction` moves it to a bin edge"""
    try:
        thres = float(thres)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: thres {thres!r} is no optical density >= 0") from None
    if not 0.0 <= thres < math.inf:       # a NaN fails both comparisons
        raise ValueError(f"{what}: thres {thres!r} is no optical density >= 0")
    return min(int(round(thres * 64.0)), STAIN_BINS)


def _check_cell_pass(what, raster, shrink, cell, bg_level, max_pixels=None):
    """the host checks of a pass over the cells of the burden grid (:func:`stain_load`, :func:`focus_map`) -> (H, W, cell, bg_level)"""
    if shrink not in (1, 2):
        raise ValueError(f"{what}: shrink {shrink!r} is neither 1 nor 2")
    if getattr(raster, "ndim", 0) != 3 or raster.shape[2] != 3 or raster.dtype != np.uint8:
        raise ValueError(f"{what}: raster must be a uint8 [H,W,3] array")
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    if H < 1 or W < 1:
        raise ValueError(f"{what}: raster {tuple(raster.shape)} has no (halved) pixel")
    if max(H, W) > LOAD_MAX_SIDE or (max_pixels is not None and H * W >= max_pixels):
        raise ValueError(f"{what}: a (halved) slide of {H} x {W} exceeds {LOAD_MAX_SIDE} pixels per side"
                         + ("" if max_pixels is None else f" or 2**{max_pixels.bit_length() - 1} pixels"))
    cell = _whole(cell, LOAD_MIN_CELL, 2 ** 31 - 1, f"{what}: cell")
    gy, gx, _ = tile_grid(H, W, cell)
    if gy * gx > LOAD_MAX_CELLS:
        raise ValueError(f"{what}: {gy} x {gx} cells exceed {LOAD_MAX_CELLS}; choose a larger cell")
    return H, W, cell, _whole(bg_level, 0, 256, f"{what}: bg_level")


def _check_load(what, raster, shrink, cell, bg_level, stain, basis):
    """the host checks :func:`stain_load` and ``quantify_region(load=True)`` share -> (H, W, cell, bg_level)"""
    checked = _check_cell_pass(what, raster, shrink, cell, bg_level)
    if isinstance(stain, bool) or stain not in (0, 1):
        raise ValueError(f"{what}: stain {stain!r} is neither 0 nor 1")
    if not isinstance(basis, StainBasis):
        raise ValueError(f"{what}: basis must be a wsi.StainBasis")
    return checked


def _check_rows(what, rows):
    if rows is not None and (len(getattr(rows, "shape", ())) != 2 or rows.shape[1] != 7):
        raise ValueError(f"{what}: rows must be [M,7] or None, got {tuple(getattr(rows, 'shape', ())) or type(rows).__name__}")


def _cell_box_pass(stream, gy, gx, rows, n_box_sums, call):
    """What :func:`stain_load` and :func:`focus_map` share: ``cells`` int64 [gy,gx,3] and, with ``rows`` ([M,7] or None), ``boxes`` int64
    [M,n_box_sums] and ``flags`` are zeroed once; every strip adds to them in ``call(k, j, rows, width, cells, rows, M, boxes, flags)``
    (device pointers; without a box None, 0, None, None); one read-back -> the three cell maps, ``boxes``, ``flags`` (None without rows)"""
    from .stats import _slide_array
    cells = torch.zeros(gy, gx, 3, device=stream.dev, dtype=torch.int64)
    box_args = (None, 0, None, None)
    if rows is not None:
        rows = _slide_array(rows, 7, stream.dev)
        M = int(rows.shape[0])
        boxes = torch.zeros(M, n_box_sums, device=stream.dev, dtype=torch.int64)
        flags = torch.zeros(1, device=stream.dev, dtype=torch.int32)
        if M:
            box_args = (ptr(rows), M, ptr(boxes), ptr(flags))
    stream.each(lambda k, j, valid, width: call(k, j, valid, width, ptr(cells), *box_args))
    c = cells.cpu().numpy()
    maps = tuple(np.ascontiguousarray(c[:, :, i]) for i in range(3))
    return maps + ((None, None) if rows is None else (boxes.cpu().numpy(), int(flags.item())))


def stain_load(raster, rows=None, cell=128, shrink=1, bg_level=220, thres=0.15, stain=1, basis=H_DAB):
    """Amyloid load of a slide (``ay_stain_load_u8``, THE LOAD RULE in ``include/amyloid_yolo.h``): per cell of the grid
    ``tile_grid(H, W, cell)`` -- :func:`burden_map`'s -- the tissue pixels, the pixels whose concentration of ``stain`` (0 or 1;
    default 1, DAB on ``H_DAB``) reaches the threshold, and the sum of their bins; with ``rows`` the same inside every box.

    The raster goes ONCE through the strips of a :class:`StripStream`, at full resolution, without a probe: the exact rule, the
    2x2 means of ``shrink=2`` included.  The tables are ``StainMap.identity(basis)``'s (only ``od`` and ``D`` are read); the outputs
    are zeroed once, every strip adds to them on the device and they are read back once.  ``cell >= 16``; (halved) sides up to 2^24.

    ``thres`` is an optical density; it moves to a bin edge as in :meth:`StainStats.positive_fraction`, ``j = min(round(thres * 64),
    512)``, and a pixel is positive iff it is tissue and its bin is ``>= j`` (``j == 512``: none).  The threshold applies to the
    slide's OWN concentrations: for a threshold on the scale a :class:`StainMap` normalises to, pass ``thres / stain_map.gains[s]``.

    ``rows``: None, or ``[M, 7]`` as :func:`detect_region` returns them (concatenated; pixels of the (halved) slide; a tensor or
    array on the host or the device).  Only the four coordinates are read.  A box owns the pixels whose centre lies in ``[x1, x2) x
    [y1, y2)``, clamped to the slide; overlapping boxes each count their own pixels; a row with a coordinate that is not finite is
    flagged and gets zeros.  One box runs on one wavefront: made for detections, correct for any rectangle.

    Returns a dict: ``tissue``, ``positive``, ``bin_sum`` NumPy int64 ``[Gy, Gx]``; ``load`` float64 ``positive / tissue``, NaN where
    a cell has no tissue; ``total_load`` (``positive.sum() / tissue.sum()``, NaN without tissue: on the same ``bg_level``, ``stain``
    and ``thres`` exactly ``stain_stats(raster, probe_stride=1).positive_fraction(stain, thres)[0]``); ``thres`` as it took effect
    (``j / 64``); with ``rows`` also ``boxes`` int64 ``[M, 4]`` = (pixels, tissue, positive, bin_sum) -- :func:`box_morphometry` turns
    them into areas -- and ``flags`` (bit 1: a coordinate not finite)."""
    H, W, cell, bg_level = _check_load("stain_load", raster, shrink, cell, bg_level, stain, basis)
    j = _thres_bin(thres, "stain_load")
    _check_rows("stain_load", rows)
    T = min(1536, H)
    stream = StripStream(raster, T, T, shrink)
    params = StainMap.identity(basis).params
    gy, gx, _ = tile_grid(H, W, cell)
    L = _lib.lib()
    tissue, positive, bin_sum, boxes, flags = _cell_box_pass(stream, gy, gx, rows, 4, lambda k, jy, valid, width, cells, *box_args: check(
        L.ay_stain_load_u8(*stream.args(k, valid, width), jy * T, 0, H, W, bg_level, ptr(params), int(stain), j, cell, cells, *box_args,
                           _lib.stream_ptr()), "ay_stain_load_u8"))
    n_t, n_p = int(tissue.sum()), int(positive.sum())
    out = {"tissue": tissue, "positive": positive, "bin_sum": bin_sum,
           "load": positive.astype(np.float64) / np.where(tissue > 0, tissue, np.nan),
           "total_load": float(n_p) / n_t if n_t else math.nan, "thres": j / 64.0}
    if rows is not None:
        out["boxes"], out["flags"] = boxes, flags
    return out


def box_morphometry(boxes, mpp=None):
    """Per-detection morphometry from :func:`stain_load`'s ``boxes`` ``[M, 4]`` = (pixels, tissue, positive, bin_sum); host
    arithmetic in float64 -> a dict of ``[M]`` arrays:
    ``area_px`` the positive pixels; ``fill = positive / pixels``; ``mean_od = (bin_sum / positive + 0.5) / 64``, the mean optical
    density of the positive pixels at the centres of their 1/64-OD bins (bin 511 holds everything from 8 OD on: it saturates); with
    ``mpp`` (microns per pixel of the (halved) slide) ``area_um2 = area_px * mpp**2`` and ``equiv_diameter_um = 2 * sqrt(area_um2 /
    pi)``, the diameter of the disc of that area.  NaN where a box has no positive pixel (``fill``: where it owns no pixel)."""
    b = np.asarray(boxes)
    if b.ndim != 2 or b.shape[1] != 4 or b.dtype.kind not in "iu" or (b < 0).any():
        raise ValueError(f"box_morphometry: boxes must be [M, 4] non-negative integers, got {b.dtype} {b.shape}")
    if mpp is not None and not 0.0 < float(mpp) < math.inf:
        raise ValueError(f"box_morphometry: mpp {mpp!r} is no positive number of microns per pixel")
    pixels, positive, bin_sum = (b[:, i].astype(np.float64) for i in (0, 2, 3))
    some = np.where(positive > 0, positive, np.nan)
    out = {"area_px": some, "fill": positive / np.where(pixels > 0, pixels, np.nan), "mean_od": (bin_sum / some + 0.5) / 64.0}
    if mpp is not None:
        out["area_um2"] = some * float(mpp) ** 2
        out["equiv_diameter_um"] = 2.0 * np.sqrt(out["area_um2"] / math.pi)
    return out


# ---- plaque segmentation: the stained component under every detection ------------------------------------------------------------------
SEG_COLS, SEG_MAX_SIDE, SEG_MAX_MARGIN = 20, 255, 127                    # include/amyloid_yolo.h, THE SEGMENT RULE
SEG_NONFINITE, SEG_EMPTY, SEG_LARGE, SEG_NOT_RESIDENT, SEG_INTERNAL = 1, 2, 4, 8, 16


def _check_segment(what, raster, shrink, bg_level, thres, core_thres, stain, basis, margin, min_area):
    """the host checks :func:`segment_boxes` and ``quantify_region(segment=True)`` share -> (H, W, bg_level, thres_bin, core_bin,
    margin, min_area)"""
    H, W, _, bg_level = _check_load(what, raster, shrink, LOAD_MAX_SIDE, bg_level, stain, basis)       # one cell: no grid here
    j = _thres_bin(thres, what)
    core = STAIN_BINS if core_thres is None else _thres_bin(core_thres, f"{what}: core_thres")
    if core < j:
        raise ValueError(f"{what}: core_thres {core_thres!r} lies below thres {thres!r}")
    return (H, W, bg_level, j, core, _whole(margin, 0, SEG_MAX_MARGIN, f"{what}: margin"),
            _whole(min_area, 1, 2 ** 31 - 1, f"{what}: min_area"))


def _segment_owner_rows(rows, H, W, margin):
    """THE SEGMENT RULE's owner row of every row, on the host in float32 by the rule's steps: ``wy0`` with a window, else 0"""
    r = np.asarray(rows, np.float32).reshape(-1, 7)[:, :4]
    finite = np.isfinite(r).all(1)
    r = np.where(finite[:, None], r, np.float32(0))
    edge = lambda v, n: np.minimum(np.maximum(np.ceil(v - np.float32(0.5)), np.float32(0)), np.float32(n)).astype(np.int64)
    lo_x, lo_y, hi_x, hi_y = edge(r[:, 0], W), edge(r[:, 1], H), edge(r[:, 2], W), edge(r[:, 3], H)
    return np.where(finite & (lo_x < hi_x) & (lo_y < hi_y), np.maximum(lo_y - margin, 0), 0)


def segment_boxes(raster, rows, margin=8, shrink=1, bg_level=220, thres=0.15, core_thres=None, stain=1, basis=H_DAB, min_area=1,
                  strip=2048):
    """The stained object under every detection (``ay_box_segments_u8``, THE SEGMENT RULE in ``include/amyloid_yolo.h``): per row of
    ``rows`` the 8-connected component of stain-positive pixels that reaches into the box, out of a WINDOW, the box grown by
    ``margin`` (0 .. 127) pixels on every side and cut to the slide.

    Pixel classes are :func:`stain_load`'s: a pixel is positive iff it is tissue at ``bg_level`` and its bin of ``stain`` (on
    ``basis``) reaches ``thres`` (an optical density, moved to a bin edge); it is CORE iff it also reaches ``core_thres``
    (``None``: no pixel is core; below ``thres``: ``ValueError``).  A component is a candidate iff it has a pixel in the box proper and
    at least ``min_area`` pixels; the largest candidate is selected, among equals the one with the lowest raster index in the window.
    Neighbouring plaques that poke into the box, and speckle, are other components; what the box cut off is part of this one.

    ``rows``: ``[M, 7]`` as :func:`detect_region` returns them (concatenated; pixels of the (halved) slide; on the host or the device);
    only the four coordinates are read.  A window of more than 255 pixels a side is flagged ``SEG_LARGE`` and not segmented.

    Strips: with ``T = min(strip, H)`` the strips are ``T - 254`` rows apart (``strip`` an integer ``>= 255``; a slide with ``H < 255``
    is one strip), strip ``j`` owns the rows whose window starts in ``[j * step, (j + 1) * step)``, the last through ``H``, and every
    window of at most 255 rows lies wholly in the strip that owns it: the result does not depend on ``strip``.  The owner rows are
    computed on the host, and ONLY THE STRIPS THAT OWN A ROW ARE STAGED AND UPLOADED, at full width.

    Returns a dict: ``segments`` NumPy int32 ``[M, 20]`` (status, window, positives, candidates, and of the selected component area,
    core pixels, bin sum, perimeter, coordinate sums, tight box, window sides touched, pixels inside the box: the table in the
    header; :func:`plaque_morphometry` turns them into numbers), ``flags`` (the OR of the statuses), ``thres`` and ``core_thres`` as
    they took effect (``core_thres`` 8.0: none), ``strips`` = (visited, total).  ``M == 0``: empty arrays, no launch."""
    H, W, bg_level, j, core, margin, min_area = _check_segment("segment_boxes", raster, shrink, bg_level, thres, core_thres, stain, basis,
                                                               margin, min_area)
    _check_rows("segment_boxes", rows)
    if rows is None:
        raise ValueError("segment_boxes: rows must be [M,7]")
    strip = _whole(strip, SEG_MAX_SIDE, 2 ** 31 - 1, "segment_boxes: strip")
    T = min(strip, H)
    step = T - (SEG_MAX_SIDE - 1) if H >= SEG_MAX_SIDE else T
    total = tile_grid(H, 1, T, T - step)[0]
    M = int(rows.shape[0])
    out = {"segments": np.zeros((M, SEG_COLS), np.int32), "flags": 0, "thres": j / 64.0, "core_thres": core / 64.0, "strips": (0, total)}
    if M == 0:
        return out
    host_rows = rows.detach().cpu().numpy() if torch.is_tensor(rows) else rows
    owners = np.minimum(_segment_owner_rows(host_rows, H, W, margin) // step, total - 1)
    visit = [int(v) for v in np.unique(owners)]
    stream = StripStream(raster, T, step, shrink, [(v, 0, raster.shape[1]) for v in visit])
    from .stats import _slide_array
    rows = _slide_array(rows, 7, stream.dev)
    params = StainMap.identity(basis).params
    seg = torch.zeros(M, SEG_COLS, device=stream.dev, dtype=torch.int32)
    flags = torch.zeros(1, device=stream.dev, dtype=torch.int32)
    L = _lib.lib()
    stream.each(lambda k, v, valid, width: check(
        L.ay_box_segments_u8(*stream.args(k, valid, width), v * step, 0, H, W, v * step, H if v == total - 1 else (v + 1) * step, bg_level,
                             ptr(params), int(stain), j, core, margin, min_area, ptr(rows), M, ptr(seg), ptr(flags), _lib.stream_ptr()),
        "ay_box_segments_u8"))
    out["segments"], out["flags"], out["strips"] = seg.cpu().numpy(), int(flags.item()), (len(visit), total)
    return out


def plaque_morphometry(segments, mpp=None, slide_hw=None):
    """Per-detection morphometry of the selected components from :func:`segment_boxes`' ``segments`` ``[M, 20]``; host arithmetic in
    float64 -> a dict of ``[M]`` arrays, NaN (``truncated``: False) where the status is not 0 or nothing was selected:
    ``area_px``; ``core_fraction = core / area``; ``mean_od = (bin_sum / area + 0.5) / 64`` (bin centres, as
    :func:`box_morphometry`); ``centroid_x = wx0 + sum_x / area + 0.5`` and ``centroid_y`` likewise, in slide coordinates with pixel
    centres at halves; ``tight_box`` ``[M, 4]`` = (x1, y1, x2, y2), the high edges exclusive; ``perimeter_px``, the crack length: the
    pixel edges between the component and what is not it; ``compactness = 16 * area / perimeter**2``: 1 for a square and about pi / 4
    for a digital disc -- THIS IS NOT A EUCLIDEAN CIRCULARITY: the crack length of a digital disc is that of its bounding square;
    ``outside_fraction = 1 - in_box / area``: how much of the plaque the detector's box missed; ``truncated``: the component touches
    a side of its window that is not a border of the slide (without ``slide_hw`` = (H, W): any side), so the window cut it and the
    numbers are lower bounds; ``candidates``.  With ``mpp`` (microns per pixel of the (halved) slide) also ``area_um2`` and
    ``equiv_diameter_um = 2 * sqrt(area_um2 / pi)``."""
    s = np.asarray(segments)
    if s.ndim != 2 or s.shape[1] != SEG_COLS or s.dtype.kind not in "iu":
        raise ValueError(f"plaque_morphometry: segments must be [M, {SEG_COLS}] integers, got {s.dtype} {s.shape}")
    if mpp is not None and not 0.0 < float(mpp) < math.inf:
        raise ValueError(f"plaque_morphometry: mpp {mpp!r} is no positive number of microns per pixel")
    s = s.astype(np.int64)
    ok = (s[:, 0] == 0) & (s[:, 7] > 0)
    f = lambda col: np.where(ok, s[:, col], 0).astype(np.float64)
    area = np.where(ok, s[:, 7], np.nan).astype(np.float64)
    sides = s[:, 17].copy()
    if slide_hw is not None:
        Hs, Ws = (_whole(v, 1, 2 ** 31 - 1, "plaque_morphometry: slide_hw") for v in slide_hw)
        sides &= ~(np.where(s[:, 1] == 0, 1, 0) | np.where(s[:, 2] == 0, 2, 0) | np.where(s[:, 1] + s[:, 3] == Ws, 4, 0)
                   | np.where(s[:, 2] + s[:, 4] == Hs, 8, 0))
    with np.errstate(invalid="ignore", divide="ignore"):
        out = {"area_px": area, "core_fraction": f(8) / area, "mean_od": (f(9) / area + 0.5) / 64.0,
               "centroid_x": f(1) + f(11) / area + 0.5, "centroid_y": f(2) + f(12) / area + 0.5,
               "tight_box": np.where(ok[:, None], s[:, 13:17], np.nan).astype(np.float64), "perimeter_px": np.where(ok, s[:, 10], np.nan).astype(np.float64),
               "compactness": 16.0 * area / np.where(ok, s[:, 10], np.nan).astype(np.float64) ** 2, "outside_fraction": 1.0 - f(18) / area,
               "truncated": ok & (sides != 0), "candidates": np.where(ok, s[:, 6], np.nan).astype(np.float64)}
    if mpp is not None:
        out["area_um2"] = area * float(mpp) ** 2
        out["equiv_diameter_um"] = 2.0 * np.sqrt(out["area_um2"] / math.pi)
    return out


# ---- focus map: sharpness per map cell and per detection ------------------------------------------------------------------------------
FOCUS_MIN_CELL, FOCUS_MAX_SIDE, FOCUS_FLAG_NONFINITE = 16, 1 << 24, 1    # include/amyloid_yolo.h, THE FOCUS RULE: THE LOAD RULE's
FOCUS_MAX_PIXELS = 1 << 43                                               # H * W below it: s2 fits int64


def _check_focus(what, raster, shrink, cell, bg_level):
    """the host checks :func:`focus_map` and ``quantify_region(focus=True)`` share -> (H, W, cell, bg_level)"""
    return _check_cell_pass(what, raster, shrink, cell, bg_level, FOCUS_MAX_PIXELS)


def _sharpness(n, s1, s2):
    """THE FOCUS RULE's host step: the variance of the Laplacian ``s2 / n - (s1 / n)**2`` in float64, NaN where ``n == 0``"""
    n = np.where(np.asarray(n) > 0, n, np.nan).astype(np.float64)
    return np.asarray(s2, np.float64) / n - (np.asarray(s1, np.float64) / n) ** 2


def focus_map(raster, rows=None, cell=128, shrink=1, bg_level=220, strip=1536):
    """Image sharpness of a slide (``ay_focus_u8``, THE FOCUS RULE in ``include/amyloid_yolo.h``): per cell of the grid
    ``tile_grid(H, W, cell)`` -- :func:`burden_map`'s -- the variance of the 4-neighbour Laplacian of the luma over the EVALUATED
    pixels: those that are tissue at ``bg_level`` with all four edge neighbours, so that a tissue / glass edge never counts as
    sharpness; with ``rows`` the same inside every box (the pixels :func:`stain_load` gives it).

    The raster goes ONCE through the strips of a :class:`StripStream` at full resolution; a pixel needs the rows above and below
    it, so consecutive strips share two rows: with ``T = min(strip, H)`` strip ``j`` starts at row ``j * (T - 2)`` and owns the centre
    rows ``[j * (T - 2) + 1, j * (T - 2) + T - 1)``, clipped to what it holds, and every row ``1 .. H - 2`` is owned exactly once:
    the result does not depend on ``strip`` (an integer ``>= 3``).  The outputs are zeroed once, every strip adds to them on the
    device and they are read back once.  ``cell >= 16``; (halved) sides up to 2^24 and fewer than 2^43 pixels.  A slide with ``H < 3``
    or ``W < 3`` has no evaluated pixel: zeros, without a launch.

    Returns a dict: ``n``, ``s1``, ``s2`` NumPy int64 ``[Gy, Gx]`` (evaluated pixels, the sum of the Laplacian, the sum of its
    squares) and ``sharpness`` float64 ``s2 / n - (s1 / n)**2``, NaN where a cell has no evaluated pixel; with ``rows`` (None, or
    ``[M, 7]`` as :func:`detect_region` returns them; only the four coordinates are read) also ``boxes`` int64 ``[M, 3]`` = (n, s1,
    s2), ``box_sharpness`` float64 ``[M]`` and ``flags`` (bit 1: a coordinate not finite; such a row gets zeros).  Sharpness depends
    on the texture of the tissue and the strength of the stain as well as on focus: see :func:`focus_summary`."""
    H, W, cell, bg_level = _check_focus("focus_map", raster, shrink, cell, bg_level)
    strip = _whole(strip, 3, 2 ** 31 - 1, "focus_map: strip")
    _check_rows("focus_map", rows)
    gy, gx, _ = tile_grid(H, W, cell)
    if H < 3 or W < 3:
        n, s1, s2 = (np.zeros((gy, gx), np.int64) for _ in range(3))
        b, f = (None, None) if rows is None else (np.zeros((int(rows.shape[0]), 3), np.int64), 0)
    else:
        stream = StripStream(raster, min(strip, H), min(strip, H) - 2, shrink)     # a two-row halo
        L = _lib.lib()

        def call(k, jy, valid, width, cells, *box_args):
            y0, held = jy * stream.step, valid // stream.shrink
            check(L.ay_focus_u8(*stream.args(k, valid, width), y0, H, W, y0 + 1, y0 + held - 1, bg_level, cell, cells, *box_args,
                                _lib.stream_ptr()), "ay_focus_u8")

        n, s1, s2, b, f = _cell_box_pass(stream, gy, gx, rows, 3, call)
    out = {"n": n, "s1": s1, "s2": s2, "sharpness": _sharpness(n, s1, s2)}
    if rows is not None:
        out["boxes"], out["box_sharpness"], out["flags"] = b, _sharpness(b[:, 0], b[:, 1], b[:, 2]), f
    return out


def focus_summary(focus, tissue=None, min_sharpness=None, min_pixels=1):
    """What a focus map says about a slide; host arithmetic on :func:`focus_map`'s dict.

    ``evaluated_fraction``: the evaluated pixels over the tissue pixels of the slide, with ``tissue`` an integer map ``[Gy, Gx]`` on
    the same grid, ``bg_level`` and raster (``stain_load(...)["tissue"]``, ``tissue_counts(raster, cell)``); NaN without ``tissue``
    or without tissue.  Thin or ragged tissue has few pixels with a whole tissue neighbourhood, and its cells say little.

    With ``min_sharpness`` also ``in_focus``, a bool map: ``n >= min_pixels`` and ``sharpness >= min_sharpness``, and
    ``in_focus_fraction``, the share of the evaluated pixels that lie in in-focus cells (NaN if none was evaluated).  With
    ``min_sharpness=None`` no classification is returned.

    NO DEFAULT THRESHOLD IS OFFERED: the variance of the Laplacian grows with the texture of the tissue and the strength of the stain
    as well as with focus, so a threshold holds for one tissue, stain protocol, scanner and ``shrink`` only.  Derive it from slides of
    that kind that are known to be sharp (for instance a low percentile of their cells' sharpness), not from this docstring."""
    n = np.asarray(focus["n"])
    sharp = np.asarray(focus["sharpness"], np.float64)
    if n.ndim != 2 or n.dtype.kind not in "iu" or sharp.shape != n.shape or (n < 0).any():
        raise ValueError(f"focus_summary: focus must be focus_map's dict (n {n.dtype} {n.shape}, sharpness {sharp.shape})")
    min_pixels = _whole(min_pixels, 1, 2 ** 62, "focus_summary: min_pixels")
    total = int(n.sum())
    out = {"evaluated_fraction": math.nan}
    if tissue is not None:
        t = np.asarray(tissue)
        if t.shape != n.shape or t.dtype.kind not in "iu" or (t < 0).any():
            raise ValueError(f"focus_summary: tissue {t.dtype} {t.shape} is no count map on the grid {n.shape}")
        n_t = int(t.sum(dtype=np.int64))
        if n_t:
            out["evaluated_fraction"] = total / n_t
    if min_sharpness is not None:
        if isinstance(min_sharpness, bool) or not 0.0 <= float(min_sharpness) < math.inf:       # a NaN fails both comparisons
            raise ValueError(f"focus_summary: min_sharpness {min_sharpness!r} is no variance >= 0")
        with np.errstate(invalid="ignore"):
            out["in_focus"] = (n >= min_pixels) & (sharp >= float(min_sharpness))                # NaN compares False
        out["in_focus_fraction"] = int(n[out["in_focus"]].sum()) / total if total else math.nan
    return out


# ---- training windows out of annotated slides ------------------------------------------------------------------------------------
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
        from .augment import AugmentRanges
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
        from .augment import transform_labels
        return transform_labels(rows, T, T, rec, min_visible=self.min_visible)

    def plan_batch(self):
        """draws the next batch (host only, no device call) -> :class:`SlideBatchPlan`"""
        from .augment import AugTable, footprint, sample_params
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
        from .augment import make_window_table
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
        from .augment import launch_windows
        if not torch.cuda.is_available():
            raise _lib.AyError("no HIP device: SlideSampler has no CPU fallback")
        dev = torch.device("cuda", torch.cuda.current_device())
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
