"""Amyloid load: :func:`stain_load` classifies every pixel of a slide (tissue, DAB-positive) and sums it per map cell and per detection
box (``ay_stain_load_u8``, THE LOAD RULE); :func:`box_morphometry` turns the box sums into areas, fill and mean optical density."""
import math

import numpy as np

from .. import _lib
from .._lib import check, ptr
from .cells import _cell_box_pass, _check_load, _thres_bin, add_area_um, check_mpp
from .colour import H_DAB, StainMap
from .grid import check_rows, tile_grid
from .stream import STRIP_ROWS, StripStream


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
    check_rows("stain_load", rows, none_ok=True)
    T = min(STRIP_ROWS, H)
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
    check_mpp("box_morphometry", mpp)
    pixels, positive, bin_sum = (b[:, i].astype(np.float64) for i in (0, 2, 3))
    some = np.where(positive > 0, positive, np.nan)
    return add_area_um({"area_px": some, "fill": positive / np.where(pixels > 0, pixels, np.nan), "mean_od": (bin_sum / some + 0.5) / 64.0}, mpp)
