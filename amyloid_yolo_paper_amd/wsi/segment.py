"""Plaque segmentation: :func:`segment_boxes` labels the connected stain-positive component under every detection
(``ay_box_segments_u8``, THE SEGMENT RULE) and :func:`plaque_morphometry` turns its words into area, core fraction, centroid, perimeter
and compactness."""
import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from ..stats import _slide_array
from .cells import LOAD_MAX_SIDE, _check_load, _thres_bin, add_area_um, check_mpp
from .colour import H_DAB, STAIN_BINS, StainMap
from .grid import _whole, check_rows, tile_grid
from .stream import StripStream


_AY = _lib.CONSTANTS                                                      # include/amyloid_yolo.h, THE SEGMENT RULE
SEG_COLS, SEG_MAX_SIDE, SEG_MAX_MARGIN = _AY["AY_SEG_COLS"], _AY["AY_SEG_MAX_SIDE"], _AY["AY_SEG_MAX_MARGIN"]
SEG_NONFINITE, SEG_EMPTY, SEG_LARGE, SEG_NOT_RESIDENT, SEG_INTERNAL = (
    _AY["AY_SEG_NONFINITE"], _AY["AY_SEG_EMPTY"], _AY["AY_SEG_LARGE"], _AY["AY_SEG_NOT_RESIDENT"], _AY["AY_SEG_INTERNAL"])


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
    check_rows("segment_boxes", rows)
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
    check_mpp("plaque_morphometry", mpp)
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
    return add_area_um(out, mpp)
