"""Most of a histology slide is glass: :func:`tissue_counts` (``ay_tile_tissue_u8``, THE TISSUE RULE in ``include/amyloid_yolo.h``)
counts the tissue pixels of every tile, usually on a low-resolution level, and :func:`tissue_mask` turns them into the ``tile_mask``
of :func:`~.detect.detect_region`."""
import torch

from .. import _lib
from .._lib import check, ptr
from .grid import check_bg_level, probed, tile_grid, wanted_tiles
from .stream import StripStream


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
    bg_level = check_bg_level("tissue_counts", bg_level)
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
    view, s, t, o = probed(raster, tile, shrink, overlap, probe_stride)
    return wanted_tiles(tissue_counts(view, t, s, o, bg_level), t, min_tissue)
