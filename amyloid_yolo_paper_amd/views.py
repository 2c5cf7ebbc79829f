"""Dihedral test-time views: a tile is run in several of the 8 orientations of the square (flips and the transpose), the decoded
rows are mapped back to the tile's own frame, the rows of all views go through ONE merge-NMS, and a detection can be required to
have the support of several views.  THE VIEW RULE and THE VOTE RULE are stated in ``include/amyloid_yolo.h``; the kernels are in
``csrc/ay_views.hip``; ``wsi.detect_region(views=...)`` is the product path.

A view id ``v`` is in 0..7: ``FX = v & 1`` (flip along x), ``FY = (v >> 1) & 1`` (flip along y), ``T = (v >> 2) & 1`` (transpose,
applied after the flips).  No CPU fallback: everything here needs the HIP library and a GPU, except :func:`check_views`."""
import ctypes as C

import torch

from . import _lib
from ._lib import check, ptr

ALL_VIEWS = (0, 1, 2, 3, 4, 5, 6, 7)
FLIPS = (0, 1, 2, 3)


def check_views(views):
    """``views`` -> tuple of ints; ``ValueError`` if it is empty, holds an id twice or holds an id outside 0..7"""
    try:
        ids = tuple(views)
    except TypeError:
        raise ValueError(f"views: need a sequence of view ids, got {views!r}") from None
    if not ids:
        raise ValueError("views: the list is empty")
    for v in ids:
        if isinstance(v, bool) or not isinstance(v, int) and not hasattr(v, "__index__"):
            raise ValueError(f"views: {v!r} is no view id")
    ids = tuple(int(v) for v in ids)
    if any(not 0 <= v <= 7 for v in ids):
        raise ValueError(f"views: ids are 0 .. 7, got {ids}")
    if len(set(ids)) != len(ids):
        raise ValueError(f"views: an id is repeated in {ids}")
    return ids


def _c_views(views):
    ids = check_views(views)
    return (C.c_int * len(ids))(*ids), len(ids)


def unview_rows_device(pred, views, img_dim):
    """``ay_unview_rows``: pred ``[n_images, N, 5+C]`` float32 on the device, image ``i`` in view ``views[i % len(views)]``; the boxes
    ``(cx, cy, w, h)`` go back to the frame of view 0 IN PLACE.  Call it before the NMS turns them into corners."""
    arr, nv = _c_views(views)
    assert pred.is_cuda and pred.dtype == torch.float32 and pred.is_contiguous() and pred.dim() == 3
    n, N, K = pred.shape
    check(_lib.lib().ay_unview_rows(ptr(pred), n, arr, nv, N, K - 5, int(img_dim), _lib.stream_ptr()), "ay_unview_rows")
    return pred


_votes_cache = {}


def view_votes_device(pred, n_views, conf_thres, vote_thres, rows, count, votes=None):
    """``ay_view_votes``: pred ``[B, n_views * N, 5+C]`` with corners in place (as the NMS leaves it), ``rows [B, max_det, 7]`` and
    ``count [B]`` of that NMS -> votes int32 ``[B, max_det]``, the bit mask of the views that support each detection.  Without
    ``votes`` the result lives in a persistent buffer per (device, B, max_det), valid until the next call."""
    B, R, K = pred.shape
    max_det = rows.shape[1]
    assert R % int(n_views) == 0
    if votes is None:
        key = (str(pred.device), B, max_det)
        votes = _votes_cache.get(key)
        if votes is None:
            votes = _votes_cache[key] = torch.empty(B, max_det, device=pred.device, dtype=torch.int32)
    check(_lib.lib().ay_view_votes(ptr(pred), B, int(n_views), R // int(n_views), K - 5, C.c_float(conf_thres), C.c_float(vote_thres),
                                   ptr(rows), ptr(count), max_det, ptr(votes), _lib.stream_ptr()), "ay_view_votes")
    return votes


def view_select_device(rows, keep, count, votes, min_views):
    """``ay_view_select``: keeps, per image and in order, the rows (and ``keep`` entries; ``keep`` may be ``None``) whose vote mask has
    at least ``min_views`` bits; IN PLACE, ``count`` updated (an image with ``count > max_det`` keeps its count)."""
    B, max_det, _ = rows.shape
    check(_lib.lib().ay_view_select(ptr(rows), ptr(keep), ptr(count), ptr(votes), B, max_det, int(min_views), _lib.stream_ptr()),
          "ay_view_select")
    return rows, keep, count


def nms_views_device(pred, views, conf_thres, nms_thres, max_det, min_views=1, vote_thres=None, *, img_dim, slot=0):
    """The post-processing of a batch of views, no host sync: pred ``[B * V, N, 5+C]`` as the forward leaves it for tile-major
    images (tile ``b`` in view ``views[j]`` is image ``b * V + j``, ``ay_ingest_region_tiles_views_u8``'s order) -> the boxes back in
    the tile's frame (in place; ``img_dim`` is the side of the network input, which the rows do not carry), the ``V * N`` rows of a
    tile through ``utils.nms_device`` as ONE image, and for ``min_views > 1`` the votes (``vote_thres=None``: ``nms_thres``) and the
    selection.  Returns ``(rows [B, max_det, 7], keep [B, max_det], count [B], cand [B])`` as ``nms_device`` does; ``keep`` indexes
    the concatenated rows (row ``j * N + r`` is row ``r`` of view ``views[j]``)."""
    from .utils import nms_device
    ids = check_views(views)
    V = len(ids)
    if not 1 <= int(min_views) <= V:
        raise ValueError(f"min_views {min_views} outside 1 .. {V}")
    n, N, K = pred.shape
    if n % V:
        raise ValueError(f"{n} images are no whole number of tiles in {V} views")
    unview_rows_device(pred, ids, img_dim)
    cat = pred.view(n // V, V * N, K)
    rows, keep, count, cand = nms_device(cat, conf_thres, nms_thres, int(max_det), slot)
    if int(min_views) > 1:
        votes = view_votes_device(cat, V, conf_thres, nms_thres if vote_thres is None else vote_thres, rows, count)
        view_select_device(rows, keep, count, votes, min_views)
    return rows, keep, count, cand
