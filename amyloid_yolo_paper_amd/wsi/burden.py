"""What a slide carries: :func:`burden_map` bins the rows of a slide into class count maps (``ay_burden_bin``, THE BURDEN RULE) and
:func:`densest_fields` picks the densest microscope-sized fields of every class (``ay_field_select``, THE FIELD RULE)."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from ..stats import _slide_array
from .grid import _whole, check_rows, hip_device, tile_grid

_AY = _lib.CONSTANTS                                                            # include/amyloid_yolo.h, THE BURDEN / FIELD RULE
BURDEN_MAX_CLASSES, BURDEN_MAX_FIELDS = _AY["AY_BURDEN_MAX_CLASSES"], _AY["AY_BURDEN_MAX_FIELDS"]
BURDEN_FLAG_NONFINITE, BURDEN_FLAG_CLASS = _AY["AY_BURDEN_FLAG_NONFINITE"], _AY["AY_BURDEN_FLAG_CLASS"]
BURDEN_MAX_FIELD_SIDE = 46340                                                   # THE FIELD RULE's bound on field * cell


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
    check_rows("burden_map", rows)
    min_conf = float(min_conf)
    gy, gx, _ = tile_grid(H, W, cell)
    if nc * gy * gx > 1 << 30:
        raise ValueError(f"burden_map: {nc} classes x {gy} x {gx} cells exceed 2**30 counters; choose a larger cell")
    dev = hip_device("the burden maps have")
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
    dev = hip_device("the burden maps have")
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
