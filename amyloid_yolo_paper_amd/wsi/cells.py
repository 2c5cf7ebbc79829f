"""What the passes over the cells of the burden grid and the boxes of the detections share (:func:`~.load.stain_load`,
:func:`~.focus.focus_map`, :func:`~.segment.segment_boxes`): THE LOAD RULE's limits, the host checks, the zero-once / add-per-strip /
read-once frame of a pass, and the physical units of an area."""
import math

import numpy as np
import torch

from .._lib import CONSTANTS, ptr
from ..stats import _slide_array
from .colour import STAIN_BINS, StainBasis
from .grid import _whole, check_raster, tile_grid


LOAD_MIN_CELL, LOAD_FLAG_NONFINITE = CONSTANTS["AY_LOAD_MIN_CELL"], CONSTANTS["AY_LOAD_FLAG_NONFINITE"]
LOAD_MAX_SIDE = 1 << 24                                                  # include/amyloid_yolo.h, THE LOAD RULE
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
    if getattr(raster, "ndim", 0) != 3 or raster.shape[2] != 3 or raster.dtype != np.uint8:      # a ValueError here, before StripStream's asserts
        raise ValueError(f"{what}: raster must be a uint8 [H,W,3] array")
    H, W = check_raster(what, raster, shrink)
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


def _cell_box_pass(stream, gy, gx, rows, n_box_sums, call):
    """What :func:`stain_load` and :func:`focus_map` share: ``cells`` int64 [gy,gx,3] and, with ``rows`` ([M,7] or None), ``boxes`` int64
    [M,n_box_sums] and ``flags`` are zeroed once; every strip adds to them in ``call(k, j, rows, width, cells, rows, M, boxes, flags)``
    (device pointers; without a box None, 0, None, None); one read-back -> the three cell maps, ``boxes``, ``flags`` (None without rows)"""
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


def check_mpp(what, mpp):
    """microns per pixel: None or a positive finite number (a bool passes as a number here; only the spatial statistics refuse it)"""
    if mpp is not None and not 0.0 < float(mpp) < math.inf:
        raise ValueError(f"{what}: mpp {mpp!r} is no positive number of microns per pixel")


def add_area_um(out, mpp):
    """with ``mpp``, the physical units of ``out["area_px"]``: ``area_um2`` and ``equiv_diameter_um``, the diameter of the disc of that area"""
    if mpp is not None:
        out["area_um2"] = out["area_px"] * float(mpp) ** 2
        out["equiv_diameter_um"] = 2.0 * np.sqrt(out["area_um2"] / math.pi)
    return out
