"""Detection over a whole raster: :func:`detect_region` (abutting tiles, overlapping tiles with the slide-level seam merge, tile
masks, test-time views, stain maps; every mode takes its model calls from :meth:`RegionTileStream.batches`) and
:func:`evaluate_region`, its precision / recall / AP against the annotations of the slide."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from ..postprocess import seam_merge_device
from ..stats import slide_statistics
from ..utils import nms_device, non_max_suppression
from ..views import check_views, nms_views_device
from .colour import StainMap
from .grid import check_tile_mask
from .stream import RegionTileStream
from .tissue import tissue_mask


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
    if flags & _lib.CONSTANTS["AY_SEAM_FLAG_MAX_DET"]:
        raise _lib.AyError(f"detect_region: a tile holds more than max_det={max_det} detections; raise max_det or conf_thres")
    if flags & _lib.CONSTANTS["AY_SEAM_FLAG_CAPACITY"]:
        raise _lib.AyError(f"detect_region: more than seam_capacity={capacity} detections on the slide; raise seam_capacity")
    if M == 0:
        return []
    keep = seam_merge_device(slide_rows[:M], slide_tile[:M], seam_thres)
    kept, kept_tile = slide_rows[:M][keep].cpu(), slide_tile[:M][keep].cpu().numpy()
    # rows were appended in tile order: every tile is one run
    starts = np.flatnonzero(np.r_[True, kept_tile[1:] != kept_tile[:-1]])
    ends = np.r_[starts[1:], len(kept_tile)]
    return [(int(kept_tile[a]) // TX, int(kept_tile[a]) % TX, kept[a:b].clone()) for a, b in zip(starts, ends)]


def cat_rows(res):
    """:func:`detect_region`'s ``(ty, tx, boxes)`` result, concatenated in that order -> ``rows`` [M,7]"""
    return torch.cat([d for _, _, d in res]) if res else torch.zeros(0, 7)


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
    res = detect_region(model, raster, **detect_region_kwargs)
    rows = cat_rows(res)
    out = slide_statistics(rows, targets, iou_thres, roi)
    out["rows"] = rows
    return out
