"""Spatial statistics: :func:`spatial_stats` counts the cross-class pairs of a slide's detections within every radius and finds every
row's nearest neighbour of every class (``ay_pair_counts``, THE PAIR RULE), and turns them into Ripley's K and L, the pair correlation
and the nearest-neighbour distribution on the host.  :func:`spatial_envelope` holds the observed K and L against the band of random
labellings of the same positions (``ay_pair_counts_relabel``, THE RELABEL RULE): one pair walk for all simulations."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from ..stats import _slide_array
from .grid import _whole, check_rows, hip_device


PAIR_MAX_CLASSES, PAIR_MAX_RADII, PAIR_MAX_RADIUS_Q, PAIR_MAX_SIDE = (                          # include/amyloid_yolo.h, THE PAIR RULE
    _lib.CONSTANTS["AY_PAIR_" + n] for n in ("MAX_CLASSES", "MAX_RADII", "MAX_RADIUS_Q", "MAX_SIDE"))
PAIR_WINDOW_MIN_CELL, PAIR_WINDOW_MAX_CELLS = (                                                 # THE PAIR WINDOW RULE
    _lib.CONSTANTS["AY_PAIR_WINDOW_" + n] for n in ("MIN_CELL", "MAX_CELLS"))
PAIR_RELABEL_MAX_SIMS, PAIR_RELABEL_FLAG_LABEL = (                                              # include/amyloid_yolo_spatial_sim.h, THE RELABEL RULE
    _lib.CONSTANTS["AY_PAIR_RELABEL_" + n] for n in ("MAX_SIMS", "FLAG_LABEL"))


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


def _window_cell(what, slide_hw, cell):
    """the mask cell side of THE PAIR WINDOW RULE -> (cell, Gy, Gx); ``ValueError`` below 16 px or beyond 2**26 cells"""
    H, W = slide_hw
    cell = _whole(cell, PAIR_WINDOW_MIN_CELL, PAIR_MAX_SIDE, f"{what}: window_cell")
    gy, gx = -(-H // cell), -(-W // cell)
    if gy * gx > PAIR_WINDOW_MAX_CELLS:
        raise ValueError(f"{what}: window_cell {cell} gives {gy} x {gx} mask cells on the {H} x {W} slide, more than 2**26")
    return cell, gy, gx


def window_from_tissue(tissue, slide_hw, cell, min_tissue=0.5):
    """The mask of THE PAIR WINDOW RULE from a tissue map (:func:`tissue_counts`, ``quantify_region(...)["tissue"]``) on the grid of
    ``cell``-pixel cells over the (H, W) slide: cell (gy, gx) is IN iff ``tissue[gy, gx] >= max(1, ceil(min_tissue * n))``, n the
    pixels of the cell inside the slide (the last cells of a row and column are cut by it).  Returns a bool array [Gy, Gx]."""
    if slide_hw is None or isinstance(slide_hw, (str, bytes)) or np.ndim(slide_hw) != 1 or len(slide_hw) != 2:
        raise ValueError(f"window_from_tissue: slide_hw {slide_hw!r} is no (H, W)")
    H, W = (_whole(v, 1, PAIR_MAX_SIDE, "window_from_tissue: slide_hw") for v in slide_hw)
    cell, gy, gx = _window_cell("window_from_tissue", (H, W), cell)
    if isinstance(min_tissue, bool) or not 0.0 <= float(min_tissue) <= 1.0:       # a NaN fails both comparisons
        raise ValueError(f"window_from_tissue: min_tissue {min_tissue!r} is no fraction of a cell")
    t = tissue.detach().cpu().numpy() if torch.is_tensor(tissue) else np.asarray(tissue)
    if t.shape != (gy, gx) or t.dtype.kind not in "iu":
        raise ValueError(f"window_from_tissue: tissue {t.dtype} {t.shape} is no integer map of the {gy} x {gx} cells of {cell} px")
    hs = np.minimum(cell, H - cell * np.arange(gy, dtype=np.int64))
    ws = np.minimum(cell, W - cell * np.arange(gx, dtype=np.int64))
    need = np.maximum(1, np.ceil(float(min_tissue) * (hs[:, None] * ws[None, :]).astype(np.float64))).astype(np.int64)
    return t.astype(np.int64) >= need


def window_area(window, slide_hw, cell, roi_q=None):
    """the area of mask AND ROI in square pixels, on integers: the quarter-pixel positions of the slide that lie in an IN cell and
    inside ``roi_q`` (None: the whole slide), divided by 16"""
    H, W = slide_hw
    m = np.asarray(window) != 0
    X1, Y1, X2, Y2 = (0, 0, 4 * W - 1, 4 * H - 1) if roi_q is None else (int(v) for v in roi_q)
    S = 4 * int(cell)
    x0, y0 = S * np.arange(m.shape[1], dtype=np.int64), S * np.arange(m.shape[0], dtype=np.int64)
    nx = np.maximum(np.minimum(np.minimum(x0 + S, 4 * W) - 1, X2) - np.maximum(x0, X1) + 1, 0)      # positions of a column inside the ROI
    ny = np.maximum(np.minimum(np.minimum(y0 + S, 4 * H) - 1, Y2) - np.maximum(y0, Y1) + 1, 0)
    return int(ny @ m.astype(np.int64) @ nx) / 16.0


def pair_counts_device(rows, slide_hw, radii_q, num_classes, min_conf=0.0, roi_q=None, border=True, cell_side_q=0, window=None, window_cell=0):
    """``ay_pair_counts`` on rows that live on the device (float32 [M,7], contiguous) -> a dict of int tensors on the device, all views
    of ONE buffer ``buf`` (so that a caller reads back once): ``pairs`` int64 [C,C,B], ``centres`` int32 [C,B], ``stats`` int32
    [2C+3], ``bd`` int32 [M], ``nn`` int32 [M,C,2], and ``label`` int32 [M], the rows' ``cls_pred`` as integers (a torch copy, for
    the host formulas).  Launches only: nothing is read back here.  ``cell_side_q`` overrides the grid's
    cell side (quarter pixels, at least the largest radius); the result does not depend on it.  With ``window`` (a uint8 or bool
    device tensor [Gy, Gx], contiguous, non-zero = IN) and ``window_cell`` (its cell side in pixels) the call is
    ``ay_pair_counts_window`` (THE PAIR WINDOW RULE); ``None`` calls ``ay_pair_counts`` exactly as before."""
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
    i32p = C.POINTER(C.c_int32)
    roi_arg = None if roi_q is None else np.ascontiguousarray(roi_q, np.int32).ctypes.data_as(i32p)
    head = (ptr(rows) if M else None, M, nc, H, W, C.c_float(min_conf), rq.ctypes.data_as(i32p), B, roi_arg, int(bool(border)), int(cell_side_q))
    outs = (ptr(out["pairs"]), ptr(out["centres"]), ptr(out["nn"]) if M else None, ptr(out["bd"]) if M else None, ptr(out["stats"]))
    if window is None:
        need = int(L.ay_pair_counts_workspace_bytes(M, H, W, int(rq[-1]) if B else 0, int(cell_side_q)))
        ws = torch.empty(max(need, 16), device=rows.device, dtype=torch.uint8)
        check(L.ay_pair_counts(*head, *outs, ptr(ws), need, _lib.stream_ptr()), "ay_pair_counts")
        return out
    gy, gx = -(-H // max(int(window_cell), 1)), -(-W // max(int(window_cell), 1))
    if not torch.is_tensor(window) or window.device != rows.device or window.dtype not in (torch.uint8, torch.bool) or \
            tuple(window.shape) != (gy, gx) or not window.is_contiguous():
        raise ValueError(f"pair_counts_device: window must be a contiguous uint8 or bool tensor [{gy}, {gx}] on {rows.device}")
    mask = window.view(torch.uint8) if window.dtype == torch.bool else window       # (a bool tensor holds one byte, 0 or 1, per cell)
    need = int(L.ay_pair_counts_window_workspace_bytes(M, H, W, int(rq[-1]) if B else 0, int(cell_side_q), int(window_cell)))
    ws = torch.empty(max(need, 16), device=rows.device, dtype=torch.uint8)
    check(L.ay_pair_counts_window(*head, ptr(mask), int(window_cell), *outs, ptr(ws), need, _lib.stream_ptr()), "ay_pair_counts_window")
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


def _check_window(what, slide_hw, window, window_cell):
    """the host checks of ``spatial_stats(window=, window_cell=)`` -> (mask as the caller gave it, host bool mask, cell) or
    (None, None, 0); no device is needed"""
    if window is None and window_cell is None:
        return None, None, 0
    if window is None or window_cell is None:
        raise ValueError(f"{what}: window and window_cell go together")
    cell, gy, gx = _window_cell(what, slide_hw, window_cell)
    dev_mask = torch.is_tensor(window)
    kind = window.dtype in (torch.bool, torch.uint8) if dev_mask else np.asarray(window).dtype in (np.bool_, np.uint8)
    if not kind or tuple(window.shape if dev_mask else np.shape(window)) != (gy, gx):
        raise ValueError(f"{what}: window must be a bool or uint8 array [{gy}, {gx}]: the cells of {cell} px of the {slide_hw[0]} x "
                         f"{slide_hw[1]} slide")
    host = (window.detach().cpu().numpy() if dev_mask else np.asarray(window)) != 0
    return window, host, cell


def spatial_stats(rows, slide_hw, radii, num_classes=2, min_conf=0.0, roi=None, border=True, area=None, mpp=None, window=None, window_cell=None):
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

    ``window`` (a host or device array [Gy, Gx], bool or uint8, non-zero = IN) with ``window_cell`` (its cell side in pixels, an
    integer >= 16; ``Gy = ceil(H / cell)``, ``Gx = ceil(W / cell)``) makes the window a MASK, e.g. :func:`window_from_tissue` of a
    tissue map (THE PAIR WINDOW RULE, ``ay_pair_counts_window``): the border distance is then also measured to the nearest position
    that lies in a zero cell or outside the slide, exactly, in integers, and capped at the largest radius; the window is mask AND
    ``roi``.  A row in a zero cell is no centre and not ``inside``, but still a partner.  A wrong shape or type, a cell below 16 or one
    of the two without the other is a ``ValueError``.

    Returns a dict.  Raw: ``pairs`` int64 [C,C,B] (ordered pairs, cumulative in k: over the eligible centres of class a, the
    counted rows of class b within ``r_k``, the centre itself excluded), ``centres`` int32 [C,B], ``nn`` int32 [M,C,2] = (d2 in
    quarter pixels squared, row index) of the nearest counted row of every class within the largest radius, ties to the lowest
    index, -1 where there is none, ``nn_index`` int32 [M,C], ``nn_distance`` float64 [M,C] in pixels (NaN where there is none),
    ``bd`` int32 [M] (quarter pixels to the window's border, -1 outside and for rows not counted), ``counted`` and ``inside`` [C],
    ``below``, ``flagged``, ``flags``, ``radii`` (effective, px), ``radii_q``, ``roi_q``, ``area``; with ``window`` also
    ``window_area``: the positions of the slide in IN cells and inside ``roi``, over 16, counted on the host in integers.  Derived,
    float64 on the host, NaN wherever a denominator is 0: ``intensity[b] = inside[b] / area`` (``area`` in px**2; default: the
    window's, with ``window`` its ``window_area``; ``area=`` overrides), ``K[a,b,k] = pairs / (centres[a,k] * intensity[b])``,
    ``L = sqrt(K / pi)``, ``L_minus_r``, ``g[k] = (K_k - K_{k-1}) / (pi (r_k**2 - r_{k-1}**2))`` with ``K_{-1} = r_{-1} = 0``, and
    ``G[a,b,k]``: the share of the class-a rows with ``bd >= R_k`` whose nearest b lies within ``r_k``.  With ``mpp`` also ``radii_um`` and ``K_um2``.  Under complete spatial
    randomness ``K = pi r**2``, ``L - r = 0`` and ``g = 1``; clustering at a scale shows as larger values there.

    Limits.  Without ``window`` the window is a RECTANGLE: with ``area=`` tissue pixels on a slide whose tissue outline is ragged,
    centres near a tissue edge have part of their disc over glass, and K is biased low there; ``window=`` removes that bias, and
    comparing ``K[a][b]`` with ``K[a][a]`` on the same slide or working inside a field (``roi=``) that is all tissue stay robust
    uses.  With ``window`` the outline's RESOLUTION is the mask cell (16 px at the finest): a cell is in or out as a whole.  And the
    COST is the number of pairs within 3 x 3 grid cells of side ``r_max``: quadratic in ``r_max`` at a given density.

    Whether an observed ``K[a][b]`` means anything is :func:`spatial_envelope`'s question: the band of K and L under random
    relabelling of the classes, and a global test.  Out of scope: per-field statistics (pass a field as ``roi=``)."""
    return _spatial_run("spatial_stats", rows, slide_hw, radii, num_classes, min_conf, roi, border, area, mpp, window, window_cell)[0]


def _counted_label(rows, num_classes, min_conf):
    """THE PAIR RULE's tests on device rows [M,7], as torch launches: int32 [M], the class of every counted row and -1 for the others
    (two fp32 operations for the centre, comparisons after them: the same decisions as the kernels')"""
    cx, cy, lab = (rows[:, 0] + rows[:, 2]) * 0.5, (rows[:, 1] + rows[:, 3]) * 0.5, rows[:, 6]
    ok = torch.isfinite(cx) & torch.isfinite(cy) & (lab >= 0) & (lab < num_classes) & (lab == torch.floor(lab))
    ok &= rows[:, 4] >= float(np.float32(min_conf))                    # (the kernels take min_conf as fp32)
    return torch.where(ok, lab, torch.full_like(lab, -1.0)).to(torch.int32)


def _spatial_run(what, rows, slide_hw, radii, num_classes, min_conf, roi, border, area, mpp, window, window_cell, counted_labels=False):
    """:func:`spatial_stats` -> (its dict, labels, context).  With ``counted_labels`` the label piece of the one read-back holds the
    class of the COUNTED rows (-1 for the others) and ``labels`` is that int array [M]; ``context`` is what a second call on the same
    rows needs (:func:`spatial_envelope`)."""
    given_area = area
    H, W, nc, rq, roi_q, area = _check_spatial(what, slide_hw, radii, num_classes, roi, area, mpp)
    window, mask, cell = _check_window(what, (H, W), window, window_cell)
    check_rows(what, rows)
    min_conf = float(min_conf)
    dev = hip_device("the spatial statistics have")
    rows = _slide_array(rows, 7, dev)
    M = int(rows.shape[0])
    on_dev = None
    if mask is not None:
        w_area = window_area(mask, (H, W), cell, roi_q)
        area = w_area if given_area is None else area
        on_dev = window if torch.is_tensor(window) and window.device == rows.device else torch.from_numpy(mask.view(np.uint8)).to(rows.device)
        on_dev = on_dev.contiguous()
        dv = pair_counts_device(rows, (H, W), rq, nc, min_conf, roi_q, border, 0, on_dev, cell)
    else:
        dv = pair_counts_device(rows, (H, W), rq, nc, min_conf, roi_q, border)
    if counted_labels and M:
        dv["label"].copy_(_counted_label(rows, nc, min_conf))
    host = dv["buf"].cpu()                                              # the one read-back
    off = lambda t: (t.data_ptr() - dv["buf"].data_ptr()) // 4
    take = lambda t: host[off(t):off(t) + t.numel() * t.element_size() // 4]
    pairs = take(dv["pairs"]).view(torch.int64).view(nc, nc, len(rq)).numpy().copy()
    centres, st = take(dv["centres"]).view(nc, len(rq)).numpy().copy(), take(dv["stats"]).numpy().copy()
    bd, nn = take(dv["bd"]).numpy().copy(), take(dv["nn"]).view(M, nc, 2).numpy().copy()
    d2 = nn[:, :, 0].astype(np.float64)
    all_labels = take(dv["label"]).numpy().copy()
    labels = np.where(bd >= 0, all_labels, -1)                         # G asks rows with bd >= R_k >= 1 only: those are counted
    out = {"pairs": pairs, "centres": centres, "nn": nn, "nn_index": nn[:, :, 1].copy(), "nn_distance": np.where(d2 >= 0, np.sqrt(np.abs(d2)) / 4.0, np.nan),
           "bd": bd, "counted": st[:nc].copy(), "inside": st[nc:2 * nc].copy(), "below": int(st[2 * nc]), "flagged": int(st[2 * nc + 1]),
           "flags": int(st[2 * nc + 2]), "radii": rq / 4.0, "radii_q": rq, "roi_q": roi_q, "area": area}
    if mask is not None:
        out["window_area"] = w_area
    out.update(spatial_summaries(pairs, centres, out["inside"], bd, nn, rq, area, mpp, labels))
    context = {"rows": rows, "slide_hw": (H, W), "num_classes": nc, "radii_q": rq, "roi_q": roi_q, "border": border, "min_conf": min_conf,
               "window": on_dev, "window_cell": cell, "area": area}
    return out, all_labels, context


# ---- THE RELABEL RULE (include/amyloid_yolo_spatial_sim.h): the label table on the host, the device call, the envelopes ------------------
_MASK64 = (1 << 64) - 1
_KEY_SIM, _KEY_ROW, _KEY_MIX1, _KEY_MIX2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


def relabel_keys(seed, s, n):
    """THE RELABEL RULE's keys of simulation ``s`` for the counted rows t = 0 .. n-1: a uint64 array, all arithmetic modulo 2**64"""
    z = np.uint64((int(seed) + int(s) * _KEY_SIM) & _MASK64) + np.arange(n, dtype=np.uint64) * np.uint64(_KEY_ROW)      # (arrays wrap silently)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(_KEY_MIX1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(_KEY_MIX2)
    return z ^ (z >> np.uint64(31))


def _check_envelope(what, n_sim, seed, rank):
    """the host checks of the simulation arguments -> (n_sim, seed, rank)"""
    n_sim = _whole(n_sim, 1, PAIR_RELABEL_MAX_SIMS - 1, f"{what}: n_sim")
    rank = _whole(rank, 1, max(n_sim // 2, 1), f"{what}: rank")
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= int(seed) <= _MASK64:
        raise ValueError(f"{what}: seed {seed!r} is no integer in 0 .. 2**64 - 1")
    return n_sim, int(seed), rank


def relabel_table(labels, num_classes, n_sim, seed):
    """The label table of THE RELABEL RULE: uint8 [M, n_sim + 1].  ``labels`` int [M] is the class of every counted row, in row order,
    and -1 (or any value outside 0 .. C-1) for a row that is not counted: such a row gets 255 in every column.  Column 0 is the
    observed labelling; column s >= 1 deals the observed classes out again by the rank of the rows' keys (a pure function of
    ``(seed, s, t)``, t the row's position among the counted rows): a uniform permutation, so every column keeps the class totals.
    Host NumPy: one stable argsort of uint64 keys per simulation."""
    nc = _whole(num_classes, 1, PAIR_MAX_CLASSES, "relabel_table: num_classes")
    n_sim, seed, _ = _check_envelope("relabel_table", n_sim, seed, 1)
    lab = np.asarray(labels)
    if lab.ndim != 1 or lab.dtype.kind not in "iu":
        raise ValueError(f"relabel_table: labels {lab.dtype} {lab.shape} is no integer array [M]")
    lab = lab.astype(np.int64)
    idx = np.flatnonzero((lab >= 0) & (lab < nc))
    observed = lab[idx]
    table = np.full((len(lab), n_sim + 1), 255, np.uint8)
    table[idx, 0] = observed
    by_rank = np.sort(observed, kind="stable").astype(np.uint8)         # rank r holds the class c with cum_c <= r < cum_{c+1}
    col = np.empty(len(idx), np.uint8)
    for s in range(1, n_sim + 1):
        col[np.argsort(relabel_keys(seed, s, len(idx)), kind="stable")] = by_rank
        table[idx, s] = col
    return table


def pair_counts_relabel_device(rows, slide_hw, radii_q, num_classes, table, min_conf=0.0, roi_q=None, border=True, cell_side_q=0, window=None,
                               window_cell=0):
    """``ay_pair_counts_relabel`` on rows that live on the device (float32 [M,7], contiguous) and a label table uint8 [M, S] (a device
    tensor, or a host array that is uploaded; 1 <= S <= 1024) -> a dict of int tensors on the device, all views of ONE buffer ``buf``:
    ``sim_pairs`` int64 [S,C,C,B], ``sim_centres`` int32 [S,C,B], ``sim_inside`` int32 [S,C], ``stats`` int32 [2C+3], ``bd`` int32
    [M].  The table's stride is padded to a multiple of 64 (with 255), so that the 64 labels a wavefront reads of a row are one
    aligned line.  One call, launches only: nothing is read back here.  ``window`` / ``window_cell`` as :func:`pair_counts_device`
    takes them (THE PAIR WINDOW RULE); ``cell_side_q`` does not show in the result."""
    H, W = slide_hw
    M, nc = int(rows.shape[0]), int(num_classes)
    rq = np.ascontiguousarray(radii_q, np.int32)
    B = len(rq)
    tab = table if torch.is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table, np.uint8))
    if tab.dtype != torch.uint8 or tab.dim() != 2 or int(tab.shape[0]) != M:
        raise ValueError(f"pair_counts_relabel_device: table must be uint8 [{M}, S], got {tab.dtype} {tuple(tab.shape)}")
    S = int(tab.shape[1])
    stride = max((S + 63) & ~63, 64)
    padded = torch.full((max(M, 1), stride), 255, device=rows.device, dtype=torch.uint8)
    if M and S:
        padded[:M, :S] = tab.to(rows.device)
    L = _lib.lib()
    sizes = [2 * S * nc * nc * B, S * nc * B, S * nc, 2 * nc + 3, M]
    offs = np.concatenate([[0], np.cumsum([(n + 3) & ~3 for n in sizes])])       # every piece starts on 16 bytes
    buf = torch.empty(max(int(offs[-1]), 4), device=rows.device, dtype=torch.int32)
    piece = [buf[int(o):int(o) + n] for o, n in zip(offs[:-1], sizes)]
    out = {"buf": buf, "sim_pairs": piece[0].view(torch.int64).view(S, nc, nc, B), "sim_centres": piece[1].view(S, nc, B),
           "sim_inside": piece[2].view(S, nc), "stats": piece[3], "bd": piece[4], "labels": padded}
    i32p = C.POINTER(C.c_int32)
    roi_arg = None if roi_q is None else np.ascontiguousarray(roi_q, np.int32).ctypes.data_as(i32p)
    mask, cell = None, 0
    if window is not None:
        cell = int(window_cell)
        gy, gx = -(-H // max(cell, 1)), -(-W // max(cell, 1))
        if not torch.is_tensor(window) or window.device != rows.device or window.dtype not in (torch.uint8, torch.bool) or \
                tuple(window.shape) != (gy, gx) or not window.is_contiguous():
            raise ValueError(f"pair_counts_relabel_device: window must be a contiguous uint8 or bool tensor [{gy}, {gx}] on {rows.device}")
        mask = window.view(torch.uint8) if window.dtype == torch.bool else window
    need = int(L.ay_pair_counts_relabel_workspace_bytes(M, nc, B, H, W, int(rq[-1]) if B else 0, int(cell_side_q), cell, S))
    ws = torch.empty(max(need, 16), device=rows.device, dtype=torch.uint8)
    check(L.ay_pair_counts_relabel(ptr(rows) if M else None, M, nc, H, W, C.c_float(min_conf), rq.ctypes.data_as(i32p), B, roi_arg, int(bool(border)),
                                   int(cell_side_q), ptr(mask), cell, ptr(padded), S, stride, ptr(out["sim_pairs"]), ptr(out["sim_centres"]),
                                   ptr(out["sim_inside"]), ptr(out["bd"]) if M else None, ptr(out["stats"]), ptr(ws), need, _lib.stream_ptr()),
          "ay_pair_counts_relabel")
    return out


def envelope_summaries(sim_pairs, sim_centres, sim_inside, radii_q, area, rank):
    """The host formulas of :func:`spatial_envelope`, float64, from the counts of the S + 1 patterns (index 0: the observed one)."""
    pairs, centres, inside = np.asarray(sim_pairs, np.float64), np.asarray(sim_centres, np.float64), np.asarray(sim_inside, np.float64)
    n = len(pairs) - 1
    r = np.asarray(radii_q, np.int64) / 4.0
    with np.errstate(all="ignore"):
        intensity = inside / area if area > 0 else np.full(inside.shape, np.nan)
        den = centres[:, :, None, :] * intensity[:, None, :, None]
        K = np.where(den > 0, pairs / den, np.nan)
        LR = np.sqrt(K / math.pi) - r

        def band(v):        # the rank-th smallest and largest over the simulations, NaN where any simulation is NaN
            v = np.sort(v[1:], axis=0)                                  # (NaN sorts last)
            bad = np.isnan(v[-1])
            return np.where(bad, np.nan, v[rank - 1]), np.where(bad, np.nan, v[n - rank])

        K_lo, K_hi = band(K)
        L_lo, L_hi = band(LR)
        total = np.zeros(LR.shape[1:])
        for s in range(n + 1):                                          # in this order: the sum is the same float on every run
            total = total + LR[s]
        Lbar = total / (n + 1)
        finite = np.isfinite(LR).all(0)                                 # the radii where every pattern is finite
        T = np.where(finite[None], np.abs(LR - Lbar[None]), -np.inf).max(-1)
        some = finite.any(-1)
        T = np.where(some[None], T, np.nan)
        p_mad = np.where(some, (1 + (T[1:] >= T[0][None]).sum(0)) / (n + 1), np.nan)
        out = {"K_sim": K, "L_minus_r_sim": LR, "K_lo": K_lo, "K_hi": K_hi, "L_lo": L_lo, "L_hi": L_hi, "K_mean": K[1:].mean(0),
               "L_mean": LR[1:].mean(0), "outside": (LR[0] > L_hi) | (LR[0] < L_lo), "T": T, "p_mad": p_mad}
    return out


def spatial_envelope(rows, slide_hw, radii, num_classes=2, n_sim=99, seed=0, rank=1, min_conf=0.0, roi=None, border=True, area=None, mpp=None,
                     window=None, window_cell=None):
    """Random-labelling envelopes for :func:`spatial_stats`: is an observed ``K[a][b]`` more than its class densities predict?

    THE NULL.  The positions are FIXED and the labels EXCHANGEABLE: every simulation keeps every counted row where it is and deals the
    observed classes out again among the counted rows, uniformly at random (THE RELABEL RULE, ``include/amyloid_yolo_spatial_sim.h``;
    the class totals stay).  For ``a != b`` this tests whether the two classes are labelled independently of where they lie (do CAA
    vessels and cored plaques occur together more often than their densities predict); for ``a == b`` whether class a is a random
    subset of all objects.  It does NOT test complete spatial randomness: objects that cluster as a whole give a flat result here as
    long as the classes are mixed at random among them.  The band ``*_lo .. *_hi`` is POINTWISE: at each radius on its own a share
    ``alpha_pointwise`` of null patterns falls outside it, and over many radii far more do somewhere; it is no simultaneous band.
    ``p_mad`` is the simultaneous test.

    Arguments as :func:`spatial_stats`, with ``num_classes`` >= 2, ``n_sim`` = S in 1 .. 1023 simulations, ``seed`` in 0 .. 2**64 - 1
    (the table is a pure function of it) and ``rank`` in 1 .. max(S // 2, 1); ``ValueError`` otherwise, before any launch.  Runs
    :func:`spatial_stats` unchanged for the observed pattern, builds the label table on the host (:func:`relabel_table`: column 0 the
    observed labelling, from that call's read-back), makes ONE more call for all S + 1 labellings (``ay_pair_counts_relabel``: the
    pair walk is shared, only the class indices a pair is booked under differ) and reads back once more; the rest is float64 on the
    host.

    Returns a dict: ``observed`` (the dict of :func:`spatial_stats`), ``sim_pairs`` int64 [S+1,C,C,B], ``sim_centres`` int32
    [S+1,C,B], ``sim_inside`` int32 [S+1,C] (index 0 is the observed pattern), ``n_sim``, ``seed``, ``rank``, ``flags`` (of the
    relabel call); ``K_sim`` and ``L_minus_r_sim`` [S+1,C,C,B] with ``K_s = pairs_s / (centres_s[a,k] * inside_s[b] / area)``, NaN
    where the denominator is 0 (``K_sim[0]`` equals ``observed["K"]``); ``K_lo``, ``K_hi`` and ``L_lo``, ``L_hi`` (of ``L - r``): the
    ``rank``-th smallest and largest over the simulations 1 .. S, NaN where any simulation is NaN; ``K_mean``, ``L_mean`` over the
    simulations; ``alpha_pointwise = 2 rank / (S + 1)``; ``outside`` bool [C,C,B]: the observed ``L - r`` above ``L_hi`` or below
    ``L_lo``; and the global maximum-absolute-deviation test: with ``Lbar`` the mean of ``L_minus_r_sim`` over all S + 1 patterns,
    ``T[s,a,b] = max_k |L_minus_r_sim[s] - Lbar|`` over the radii at which every pattern is finite, and ``p_mad[a,b] = (1 + #{s >= 1:
    T_s >= T_0}) / (S + 1)``, NaN where there is no such radius.

    Out of scope: envelopes for g and G (G needs the nearest neighbours of every simulation), simulations of complete spatial
    randomness (new positions inside the window), and a label table made on the device."""
    nc = _whole(num_classes, 2, PAIR_MAX_CLASSES, "spatial_envelope: num_classes (two classes at least)")
    n_sim, seed, rank = _check_envelope("spatial_envelope", n_sim, seed, rank)
    observed, labels, cx = _spatial_run("spatial_envelope", rows, slide_hw, radii, nc, min_conf, roi, border, area, mpp, window, window_cell, True)
    table = relabel_table(labels, nc, n_sim, seed)
    dv = pair_counts_relabel_device(cx["rows"], cx["slide_hw"], cx["radii_q"], nc, table, cx["min_conf"], cx["roi_q"], cx["border"], 0, cx["window"],
                                    cx["window_cell"])
    host = dv["buf"].cpu()                                              # the second read-back
    S1, B = n_sim + 1, len(cx["radii_q"])
    off = lambda t: (t.data_ptr() - dv["buf"].data_ptr()) // 4
    take = lambda t: host[off(t):off(t) + t.numel() * t.element_size() // 4]
    out = {"observed": observed, "sim_pairs": take(dv["sim_pairs"]).view(torch.int64).view(S1, nc, nc, B).numpy().copy(),
           "sim_centres": take(dv["sim_centres"]).view(S1, nc, B).numpy().copy(), "sim_inside": take(dv["sim_inside"]).view(S1, nc).numpy().copy(),
           "n_sim": n_sim, "seed": seed, "rank": rank, "flags": int(take(dv["stats"])[2 * nc + 2]), "alpha_pointwise": 2.0 * rank / (n_sim + 1)}
    out.update(envelope_summaries(out["sim_pairs"], out["sim_centres"], out["sim_inside"], cx["radii_q"], cx["area"], rank))
    return out
