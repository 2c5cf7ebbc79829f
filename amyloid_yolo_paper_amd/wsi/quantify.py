"""``quantify_region``: :func:`~.detect.detect_region`, then the count maps, the tissue of every map cell and the densest fields, and
on request the amyloid load, the focus map, the plaque segments and the spatial statistics next to them."""
import math

import numpy as np
import torch

from .burden import BURDEN_MAX_FIELD_SIDE, BURDEN_MAX_FIELDS, _field_sums, burden_map, densest_fields
from .cells import _check_load, _thres_bin, check_mpp
from .colour import H_DAB, StainMap, StainStats
from .detect import cat_rows, detect_region
from .focus import _check_focus, focus_map, focus_summary
from .grid import _whole, check_raster, probed
from .load import stain_load
from .segment import _check_segment, plaque_morphometry, segment_boxes
from . import spatial as _spatial
from .spatial import PAIR_MAX_CLASSES, _check_spatial, _window_cell, spatial_stats, window_from_tissue
from .tissue import tissue_counts


def quantify_region(model, raster, cell=128, field=8, top_k=5, field_min_tissue=0.5, mpp=None, min_conf=0.0, stain_stats=None,
                    dab_thres=None, load=False, focus=False, min_sharpness=None, segment=False, seg_margin=None, core_thres=None,
                    min_area=None, spatial_radii=None, spatial_window=False, spatial_min_tissue=0.5, spatial_envelope=None, spatial_seed=0,
                    spatial_rank=1, **detect_region_kwargs):
    """What a slide carries: :func:`detect_region`, then per class the count map, the tissue of every map cell and the densest fields.

    1. Runs ``detect_region(model, raster, **detect_region_kwargs)`` unchanged and concatenates its ``(ty, tx, boxes)`` result in
       that order into ``rows`` [M,7], as :func:`evaluate_region` does.
    2. The tissue map on the grid ``tile_grid(H, W, cell)``, in pixels of the (halved) slide, with the ``bg_level``, ``shrink`` and
       ``probe_stride`` (= d, default 16; it must divide ``cell``) among the keyword arguments.  ``probe_stride=1`` counts on the
       raster itself and is EXACT (THE TISSUE RULE, at the cost of one more upload of the slide).  Any other stride counts the
       tissue pixels of :func:`probe_view` (every d-th pixel, single source pixels, no averaging) and multiplies by ``d * d``: an
       ESTIMATE.  It is a multiple of ``d * d``, a cell on the slide's ragged edge can get up to ``d - 1`` rows and columns more
       than it holds, and tissue thinner than d pixels is seen by chance; over a field of ``field * cell`` pixels these errors
       are small against ``field_min_tissue``, per cell they need not be, and densities of single cells inherit them.
    3. ``burden_map(rows, (H, W), cell, C, min_conf)`` (C = the model's classes) and ``densest_fields(counts, tissue, field, top_k,
       need_tissue)`` with ``need_tissue = max(1, ceil(field_min_tissue * (field * cell)**2))``, computed once on the host like
       :func:`wanted_tiles`' bound.  ``field * cell <= 46340``.
    4. Returns a dict: ``rows``; ``counts`` int32 [C,Gy,Gx] on the device; ``tissue`` NumPy int32 [Gy,Gx]; ``fields`` NumPy int64
       [C,top_k,5] = (y0, x0, side, count, tissue_px) in pixels of the (halved) slide, in pick order, rows not filled -1;
       ``n_found`` [C]; ``totals`` [C] (rows counted per class); ``below``, ``flagged``, ``flags`` of :func:`burden_map`.  With
       ``mpp`` (microns per pixel of the halved slide) also ``density_per_mm2`` float64 [C,Gy,Gx], ``total_density_per_mm2`` [C]
       (``totals`` over the tissue of the whole map) and ``field_density_per_mm2`` [C,top_k]: ``count / (tissue_px * mpp**2 * 1e-6)``
       in float64 on the host, NaN where there is no tissue (and for rows not filled).

    5. With ``stain_stats`` (a :class:`StainStats` of this slide, :func:`stain_stats`) and ``dab_thres`` (an optical density) both
       given, also ``dab_positive_fraction`` = ``stain_stats.positive_fraction(1, dab_thres)[0]``, the share of tissue pixels whose
       stain-1 (DAB) concentration reaches the threshold (the classical "amyloid load"), and ``dab_thres`` as it took effect (a
       multiple of 1/64).  Host arithmetic on the histogram; nothing else changes, and without the two arguments the result has
       the keys it had.  A ``stain=`` among the keyword arguments reaches :func:`detect_region`; its basis must be the statistics'.
       A slide's own vectors need no argument of their own: ``est = estimate_basis(raster)``, ``stain_stats(raster,
       basis=est.basis)`` here and, for normalisation, ``stain=StainMap(stats, target, remix=True)``, whose ``basis`` is the
       source's; ``load=`` and ``segment=`` then unmix on the estimated basis by the precedence of item 6.

    6. With ``load=True`` (``dab_thres`` is then required, ``stain_stats`` stays optional; ``cell >= 16``) one more pass over the
       raster, ``stain_load(raster, rows, cell, shrink, bg_level, dab_thres, 1, basis)`` -- exact and at full resolution whatever
       ``probe_stride`` is; the basis is the statistics', else the ``stain=`` map's, else ``H_DAB`` -- adds ``load_tissue`` and
       ``load_positive`` int64 [Gy,Gx], ``load_map`` (their ratio, NaN without tissue), ``total_load``, ``box_load`` int64 [M,4] =
       (pixels, tissue, positive, bin_sum) for ``rows`` (:func:`box_morphometry` makes areas of it) and ``field_load`` float64
       [C,top_k]: positive over tissue, summed on the host over the cells of every picked field, NaN for rows not filled and for a
       field without tissue.  The threshold applies to the slide's own concentrations, with or without a ``stain=`` map.

    7. With ``focus=True`` (``cell >= 16``) one more pass over the raster, ``focus_map(raster, rows, cell, shrink, bg_level)`` -- THE
       FOCUS RULE, exact and at full resolution -- adds ``focus_n`` int64 and ``focus_sharpness`` float64 [Gy,Gx], ``box_sharpness``
       float64 [M] for ``rows`` and ``field_sharpness`` float64 [C,top_k]: the pooled variance of the Laplacian from the summed ``n``,
       ``s1``, ``s2`` of the cells of every picked field, NaN for rows not filled and for a field without an evaluated pixel.  Every
       count and load above assumes the scanner was in focus where it counted; these say where it was.  With ``min_sharpness`` (only
       with ``focus=True``; no default is offered, see :func:`focus_summary`) also ``in_focus`` bool [Gy,Gx] and
       ``in_focus_fraction``.  The fields are picked as before: sharpness is reported, never used.  Without ``focus`` the result has
       the keys it had.

    8. With ``segment=True`` (``dab_thres`` is then required, as for ``load=True``; the basis by the same precedence) one more pass,
       ``segment_boxes(raster, rows, seg_margin, shrink, bg_level, dab_thres, core_thres, 1, basis, min_area)`` (``seg_margin``
       default 8, ``core_thres`` default None, ``min_area`` default 1; any of them without ``segment=True`` is a ``ValueError``) --
       THE SEGMENT RULE; only the strips that hold a detection's window are uploaded -- adds ``segments`` int32 [M,20] and
       ``segment_flags``, ``plaque`` (:func:`plaque_morphometry` of them, with ``mpp`` and the slide's sides) and ``class_area_px``
       float64 [C,3]: the quartiles (25, 50, 75 %) of ``area_px`` per class over the rows with ``conf >= min_conf`` and a selected
       component, NaN for a class without one.  The segments are reported, never used: no detection is moved, re-scored or dropped.
       Without ``segment`` the result has the keys it had.

    9. With ``spatial_radii`` (a sequence of radii in pixels of the (halved) slide; at most 8 classes) also ``spatial`` =
       ``spatial_stats(rows, (H, W), spatial_radii, C, min_conf, area=tissue.sum(), mpp=mpp)``: the cross-class pair counts within
       every radius, Ripley's K and L, the pair correlation g and the nearest-neighbour distribution G over the whole slide, with the
       tissue pixels as the area (THE PAIR RULE; see :func:`spatial_stats` for what a ragged tissue outline does to K).  The
       arguments are checked before any launch.  Without it the result has the keys it had.  With ``spatial_window=True`` (only
       with ``spatial_radii``; ``cell >= 16``) the window is the tissue's outline and no rectangle: ``spatial_window`` =
       ``window_from_tissue(tissue, (H, W), cell, spatial_min_tissue)``, a bool map [Gy,Gx] of the cells that are IN, and ``spatial``
       = ``spatial_stats(..., window=spatial_window, window_cell=cell)`` (THE PAIR WINDOW RULE): a row is a centre at a radius only
       if its whole disc lies over IN cells, ``area`` is the window's area and ``inside`` counts the rows in IN cells, so that the
       intensity belongs to the same window.  ``spatial_window=False`` is the result as it was.  With ``spatial_envelope`` = the
       number of simulations (only with ``spatial_radii``; a model of two classes at least) also ``spatial_envelope`` =
       ``spatial_envelope(rows, (H, W), spatial_radii, C, spatial_envelope, spatial_seed, spatial_rank, min_conf, ...)`` with the
       window and area that ``spatial`` gets: the band of K and L under random relabelling of the classes and the global test
       ``p_mad`` (THE RELABEL RULE; see :func:`spatial_envelope` for what that null is).  ``None`` is the result as it was.

    The numbers are counts and areas; mapping them to CERAD categories is a clinical choice and not made here."""
    if not segment and not (seg_margin is None and core_thres is None and min_area is None):
        raise ValueError("quantify_region: seg_margin, core_thres and min_area need segment=True")
    if min_sharpness is not None:
        if not focus:
            raise ValueError("quantify_region: min_sharpness needs focus=True")
        if isinstance(min_sharpness, bool) or not 0.0 <= float(min_sharpness) < math.inf:
            raise ValueError(f"quantify_region: min_sharpness {min_sharpness!r} is no variance >= 0")
    if load:
        if dab_thres is None:
            raise ValueError("quantify_region: load=True needs dab_thres")
        _thres_bin(dab_thres, "quantify_region")
    elif segment:
        if dab_thres is None:
            raise ValueError("quantify_region: segment=True needs dab_thres")
    elif (stain_stats is None) != (dab_thres is None):
        raise ValueError("quantify_region: stain_stats and dab_thres go together")
    if stain_stats is not None:
        if not isinstance(stain_stats, StainStats):
            raise ValueError(f"quantify_region: stain_stats must be a wsi.StainStats, got {type(stain_stats).__name__}")
        stain_stats.positive_fraction(1, dab_thres)       # a bad threshold is refused before any launch
        st = detect_region_kwargs.get("stain")
        if isinstance(st, StainMap) and st.basis != stain_stats.basis:
            raise ValueError("quantify_region: stain and stain_stats were made on different bases")
    cell = _whole(cell, 1, BURDEN_MAX_FIELD_SIDE, "quantify_region: cell")
    F = _whole(field, 1, BURDEN_MAX_FIELD_SIDE, "quantify_region: field")
    K = _whole(top_k, 1, BURDEN_MAX_FIELDS, "quantify_region: top_k")
    if F * cell > BURDEN_MAX_FIELD_SIDE:
        raise ValueError(f"quantify_region: field * cell = {F * cell} exceeds {BURDEN_MAX_FIELD_SIDE} (a field's tissue must fit int32)")
    if not 0.0 <= float(field_min_tissue) <= 1.0:       # a NaN fails both comparisons
        raise ValueError(f"quantify_region: field_min_tissue {field_min_tissue!r} is no fraction of a field")
    check_mpp("quantify_region", mpp)
    d = int(detect_region_kwargs.get("probe_stride", 16))
    if d < 1 or cell % d:
        raise ValueError(f"quantify_region: probe_stride {d} must divide cell {cell}")
    shrink, bg_level = int(detect_region_kwargs.get("shrink", 1)), detect_region_kwargs.get("bg_level", 220)
    H, W = check_raster("quantify_region", raster, shrink)
    st = detect_region_kwargs.get("stain")      # the basis load= and segment= unmix on: the statistics', else the stain= map's, else H_DAB
    basis = stain_stats.basis if stain_stats is not None else st.basis if isinstance(st, StainMap) else H_DAB
    if load:        # refused before any launch, like everything above
        _check_load("quantify_region", raster, shrink, cell, bg_level, 1, basis)
    if focus:
        _check_focus("quantify_region", raster, shrink, cell, bg_level)
    if segment:
        seg_margin, min_area = 8 if seg_margin is None else seg_margin, 1 if min_area is None else min_area
        _check_segment("quantify_region", raster, shrink, bg_level, dab_thres, core_thres, 1, basis, seg_margin, min_area)
    min_conf = float(min_conf)
    need = max(1, math.ceil(float(field_min_tissue) * (F * cell) ** 2))
    if spatial_radii is not None:       # refused before any launch (and before the model is touched), like everything above
        _check_spatial("quantify_region", (H, W), spatial_radii, 1, None, None)
    if spatial_window:
        if spatial_radii is None:
            raise ValueError("quantify_region: spatial_window needs spatial_radii")
        _window_cell("quantify_region", (H, W), cell)
        if isinstance(spatial_min_tissue, bool) or not 0.0 <= float(spatial_min_tissue) <= 1.0:       # a NaN fails both comparisons
            raise ValueError(f"quantify_region: spatial_min_tissue {spatial_min_tissue!r} is no fraction of a cell")
    if spatial_envelope is not None:
        if spatial_radii is None:
            raise ValueError("quantify_region: spatial_envelope needs spatial_radii")
        _spatial._check_envelope("quantify_region", spatial_envelope, spatial_seed, spatial_rank)
    num_classes = int(model.yolo_layers[0].num_classes)
    if spatial_radii is not None:
        _whole(num_classes, 2 if spatial_envelope is not None else 1, PAIR_MAX_CLASSES, "quantify_region: the model's classes (spatial statistics)")
    rows = cat_rows(detect_region(model, raster, **detect_region_kwargs))
    view, s, t, _ = probed(raster, cell, shrink, 0, d)
    tissue = tissue_counts(view, t, s, 0, bg_level) * np.int32(d * d)
    bm = burden_map(rows, (H, W), cell, num_classes, min_conf)
    picked, n_found = densest_fields(bm["counts"], tissue, F, K, need)
    fields = np.full((num_classes, K, 5), -1, np.int64)
    filled = picked[:, :, 0] >= 0
    fields[filled] = np.stack([picked[:, :, 0].astype(np.int64) * cell, picked[:, :, 1].astype(np.int64) * cell,
                               np.full(picked.shape[:2], F * cell, np.int64), picked[:, :, 2], picked[:, :, 3]], 2)[filled]
    out = {"rows": rows, "counts": bm["counts"], "tissue": tissue, "fields": fields, "n_found": n_found, "totals": bm["counted"],
           "below": bm["below"], "flagged": bm["flagged"], "flags": bm["flags"]}
    if stain_stats is not None:
        out["dab_positive_fraction"], out["dab_thres"] = stain_stats.positive_fraction(1, dab_thres)
    if load:
        ld = stain_load(raster, rows, cell, shrink, bg_level, dab_thres, 1, basis)
        out["load_tissue"], out["load_positive"], out["load_map"] = ld["tissue"], ld["positive"], ld["load"]
        out["total_load"], out["box_load"] = ld["total_load"], ld["boxes"]
        out["field_load"] = np.full((num_classes, K), np.nan)
        for c, k, (t, p) in _field_sums(picked, filled, F, (ld["tissue"], ld["positive"])):
            if t:
                out["field_load"][c, k] = float(p) / t
    if focus:
        fm = focus_map(raster, rows, cell, shrink, bg_level)
        out["focus_n"], out["focus_sharpness"], out["box_sharpness"] = fm["n"], fm["sharpness"], fm["box_sharpness"]
        out["field_sharpness"] = np.full((num_classes, K), np.nan)
        for c, k, (n, s1, s2) in _field_sums(picked, filled, F, (fm["n"], fm["s1"], fm["s2"])):
            if n:
                out["field_sharpness"][c, k] = s2 / n - (s1 / n) ** 2
        if min_sharpness is not None:
            fs = focus_summary(fm, None, min_sharpness)
            out["in_focus"], out["in_focus_fraction"] = fs["in_focus"], fs["in_focus_fraction"]
    if segment:
        sg = segment_boxes(raster, rows, seg_margin, shrink, bg_level, dab_thres, core_thres, 1, basis, min_area)
        out["segments"], out["segment_flags"] = sg["segments"], sg["flags"]
        out["plaque"] = plaque_morphometry(sg["segments"], mpp, (H, W))
        out["class_area_px"] = np.full((num_classes, 3), np.nan)
        r = rows.detach().cpu().numpy() if torch.is_tensor(rows) else np.asarray(rows)
        with np.errstate(invalid="ignore"):
            counted = (r[:, 4] >= min_conf) & np.isfinite(out["plaque"]["area_px"])
        for c in range(num_classes):
            a = out["plaque"]["area_px"][counted & (r[:, 6] == c)]
            if len(a):
                out["class_area_px"][c] = np.percentile(a, [25.0, 50.0, 75.0])
    if spatial_window:
        out["spatial_window"] = window_from_tissue(tissue, (H, W), cell, spatial_min_tissue)
        out["spatial"] = spatial_stats(rows, (H, W), spatial_radii, num_classes, min_conf, mpp=mpp, window=out["spatial_window"], window_cell=cell)
    elif spatial_radii is not None:
        out["spatial"] = spatial_stats(rows, (H, W), spatial_radii, num_classes, min_conf, area=int(tissue.sum(dtype=np.int64)), mpp=mpp)
    if spatial_envelope is not None:       # the window and the area that `spatial` got
        how = dict(window=out["spatial_window"], window_cell=cell) if spatial_window else dict(area=int(tissue.sum(dtype=np.int64)))
        out["spatial_envelope"] = _spatial.spatial_envelope(rows, (H, W), spatial_radii, num_classes, spatial_envelope, spatial_seed, spatial_rank,
                                                            min_conf, mpp=mpp, **how)
    if mpp is not None:
        mm2 = lambda px: np.where(px > 0, px, np.nan).astype(np.float64) * float(mpp) ** 2 * 1e-6      # NaN where there is no tissue
        out["density_per_mm2"] = bm["counts"].cpu().numpy().astype(np.float64) / mm2(tissue)[None]
        out["total_density_per_mm2"] = bm["counted"].astype(np.float64) / mm2(np.int64(tissue.sum(dtype=np.int64)))
        out["field_density_per_mm2"] = np.where(filled, fields[:, :, 3], 0).astype(np.float64) / mm2(np.where(filled, fields[:, :, 4], 0))
    return out
