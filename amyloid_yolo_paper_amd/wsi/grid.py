"""The tile grid of a slide and what every pass checks before it launches: :func:`tile_grid` (``tile``, ``overlap`` -> tiles per axis and
``step``), :func:`wanted_tiles` and :func:`check_tile_mask` (THE TISSUE RULE's mask), :func:`probe_view` (the low-resolution stand-in
of a raster without a pyramid level), and the argument checks the passes share.  Imports no other module of the package."""
import math

import numpy as np
import torch

from .. import _lib


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


def probed(raster, tile, shrink, overlap, probe_stride):
    """What a pass with a ``probe_stride`` counts on -> ``(raster, shrink, tile, overlap)``: at stride 1 the raster itself (the exact
    rule, the 2x2 means of ``shrink=2`` included), else :func:`probe_view`'s view, which is not halved again"""
    if int(probe_stride) == 1:
        return raster, shrink, tile, overlap
    view, t, o = probe_view(raster, tile, shrink, overlap, probe_stride)
    return view, 1, t, o


# ---- the argument checks the passes share: each refuses before any launch; a site whose accepted values differ keeps its own check
def _whole(v, lo, hi, what):
    """``v`` as an int in ``lo .. hi``, else ``ValueError`` (bools and fractions are no counts)"""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} {v!r} is no integer in {lo} .. {hi}")
    return int(v)


def check_bg_level(what, bg_level):
    """``int(bg_level)`` in 0 .. 256 (:func:`tissue_counts`, :func:`stain_stats`, :func:`estimate_basis`: whatever ``int()`` takes; the
    passes over the cells of the burden grid take whole numbers only, through :func:`_whole`)"""
    bg_level = int(bg_level)
    if not 0 <= bg_level <= 256:
        raise ValueError(f"{what}: bg_level {bg_level} outside 0 .. 256")
    return bg_level


def check_probe_stride(what, probe_stride):
    d = int(probe_stride)
    if d < 1:
        raise ValueError(f"{what}: probe_stride {d} must be at least 1")
    return d


def check_raster(what, raster, shrink):
    """a raster with three axes and at least one (halved) pixel -> ``(H, W)`` of the (halved) slide; that it holds uint8 RGB is left
    to :class:`StripStream`'s asserts or checked by the caller"""
    if getattr(raster, "ndim", 0) != 3 or raster.shape[0] // shrink < 1 or raster.shape[1] // shrink < 1:
        raise ValueError(f"{what}: raster must be a uint8 [H,W,3] array with at least one (halved) pixel")
    return raster.shape[0] // shrink, raster.shape[1] // shrink


def check_rows(what, rows, none_ok=False):
    """``rows`` of detections are ``[M,7]`` (``none_ok``: or None)"""
    if rows is None and none_ok:
        return
    if len(getattr(rows, "shape", ())) != 2 or rows.shape[1] != 7:
        raise ValueError(f"{what}: rows must be [M,7]{' or None' if none_ok else ''}, got "
                         f"{tuple(getattr(rows, 'shape', ())) or type(rows).__name__}")


def hip_device(what):
    """the current HIP device; ``AyError`` without one (``what`` has no CPU fallback)"""
    if not torch.cuda.is_available():
        raise _lib.AyError(f"no HIP device: {what} no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())
