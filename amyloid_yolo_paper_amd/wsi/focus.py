"""Focus: :func:`focus_map` sums the Laplacian of the luma over the tissue of every map cell and detection box (``ay_focus_u8``, THE
FOCUS RULE) into a sharpness map and :func:`focus_summary` reads it."""
import math

import numpy as np

from .. import _lib
from .._lib import check
from .cells import _cell_box_pass, _check_cell_pass
from .grid import _whole, check_rows, tile_grid
from .stream import StripStream


FOCUS_MIN_CELL, FOCUS_FLAG_NONFINITE = _lib.CONSTANTS["AY_FOCUS_MIN_CELL"], _lib.CONSTANTS["AY_FOCUS_FLAG_NONFINITE"]
FOCUS_MAX_SIDE = 1 << 24                                                 # include/amyloid_yolo.h, THE FOCUS RULE: THE LOAD RULE's
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
    check_rows("focus_map", rows, none_ok=True)
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
