"""WSI -> tile streaming: detection over a whole-slide raster without the disk round trip of the
reference (``crop.py:13-25`` writes 1536-px JPEG tiles with pyvips ``dzsave``, ``detect.py:59-105`` reads them back).

A slide (any ``[H, W, 3]`` uint8 array: a NumPy memmap of a decoded level, a pyvips/openslide region fetched by the caller)
is walked in full-width strips of one tile row.  A strip is one contiguous slice of the raster: it goes to the device in a
single copy from a pinned staging buffer on a copy stream (two buffers, so strip i+1 uploads while strip i computes).  Three
layers: ``upload.Uploader`` holds that double-buffer protocol and nothing about slides; :class:`StripStream` feeds it the strips
of a raster (height, step, shrink, optionally column spans and the strips to visit) and is all the slide passes below need;
:class:`RegionTileStream` owns a strip stream and adds the tile side (views, stain, masks, batches).
``ay_ingest_region_tiles_step_u8`` cuts the row of tiles out of a strip on the device -- at ``step == tile`` dzsave's 'google' layout:
a ``tile`` grid from the top-left corner, edge tiles padded with the background 255 -- with the optional 40x -> 20x halving
(``crop.py:44-47``) and the detect-time ``/255`` + nearest resize fused in.  Detections come back in slide coordinates.

Abutting tiles split every object that straddles a seam.  With ``overlap > 0`` the tile origins are ``tile - overlap`` apart
(:func:`tile_grid`, the ``step`` of the same entry point), every object no larger than ``overlap`` is seen whole by at least one
tile, the per-tile detections stay on the device (``utils.nms_device`` -> ``ay_seam_append``) and one slide-level pass removes
the second sightings (``ay_seam_merge``; the rule is stated in ``include/amyloid_yolo.h``).

Most of a histology slide is glass.  :func:`tissue_counts` (``ay_tile_tissue_u8``, the rule in ``include/amyloid_yolo.h``) counts the
tissue pixels of every tile, usually on a low-resolution level, :func:`wanted_tiles` turns the counts into a ``tile_mask``, and with
a mask the stream never stages a strip without a wanted tile, stages of any other strip only the columns between its first and its
last wanted tile and cuts only the wanted tiles out of it (``ay_ingest_region_tiles_list_u8``, the same cut with the origins read
from a list); its batches are then filled with wanted tiles across strip boundaries.  Every mode of :func:`detect_region` takes its
model calls from one generator, :meth:`RegionTileStream.batches`.

Training reads the same rasters: :class:`SlideSampler` draws windows centred on annotations, hard cases and tissue out of annotated
slides and cuts them with the fused augmentation kernel under THE WINDOW RULE (``ay_augment_ingest_window_u8``), for
``train(source=...)``.

The modules, each re-exported here name by name (this file holds no code of its own; the five private names at the end are the ones
the tests and benchmark scripts reach as ``wsi._x``):
  ``grid``      the tile grid, the tissue mask, the probe view, the argument checks the passes share
  ``stream``    :class:`StripStream`, :class:`RegionTileStream`, the strips of a raster that is resident on the device
  ``tissue``    :func:`tissue_counts`, :func:`tissue_mask` (THE TISSUE RULE)
  ``detect``    :func:`detect_region`, :func:`evaluate_region`
  ``burden``    :func:`burden_map`, :func:`densest_fields` (THE BURDEN RULE, THE FIELD RULE)
  ``spatial``   :func:`spatial_stats`: pair counts, Ripley's K and L, g, nearest neighbours (THE PAIR RULE); :func:`window_from_tissue`:
                a tissue-shaped window for them (THE PAIR WINDOW RULE)
                :func:`spatial_envelope`, :func:`relabel_table`: the band of K and L under random labelling (THE RELABEL RULE)
  ``colour``    :class:`StainBasis`, :class:`StainStats`, :class:`StainMap`: the host side of THE STAIN RULE
  ``stain``     :func:`stain_stats`, :func:`normalize_region`: its passes
  ``basis``     :func:`estimate_basis`: the slide's own two stain vectors (THE BASIS RULE)
  ``cells``     what the passes over map cells and detection boxes share
  ``load``      :func:`stain_load`, :func:`box_morphometry` (THE LOAD RULE)
  ``segment``   :func:`segment_boxes`, :func:`plaque_morphometry` (THE SEGMENT RULE)
  ``focus``     :func:`focus_map`, :func:`focus_summary` (THE FOCUS RULE)
  ``quantify``  :func:`quantify_region`: what a slide carries, all of the above in one call
  ``sampler``   :class:`SlideSampler`, :class:`SlideBatchPlan`

No CPU fallback: the product path needs the HIP library and a GPU."""
from .basis import (BASIS_DIR_BINS, BASIS_MOMENT_WORDS, BASIS_OD_MAX, BASIS_OD_SCALE, BASIS_STRIP, StainEstimate, basis_plane,  # noqa: F401
                    basis_tables, basis_vectors, estimate_basis)
from .burden import (BURDEN_FLAG_CLASS, BURDEN_FLAG_NONFINITE, BURDEN_MAX_CLASSES, BURDEN_MAX_FIELD_SIDE, BURDEN_MAX_FIELDS, burden_map,  # noqa: F401
                     densest_fields)
from .cells import LOAD_FLAG_NONFINITE, LOAD_MAX_CELLS, LOAD_MAX_SIDE, LOAD_MIN_CELL  # noqa: F401
from .colour import H_DAB, STAIN_BINS, StainBasis, StainMap, StainStats, stain_tables  # noqa: F401
from .detect import detect_region, evaluate_region  # noqa: F401
from .focus import FOCUS_FLAG_NONFINITE, FOCUS_MAX_PIXELS, FOCUS_MAX_SIDE, FOCUS_MIN_CELL, focus_map, focus_summary  # noqa: F401
from .grid import check_tile_mask, probe_view, tile_grid, wanted_tiles  # noqa: F401
from .load import box_morphometry, stain_load  # noqa: F401
from .quantify import quantify_region  # noqa: F401
from .sampler import SlideBatchPlan, SlideSampler  # noqa: F401
from .segment import (SEG_COLS, SEG_EMPTY, SEG_INTERNAL, SEG_LARGE, SEG_MAX_MARGIN, SEG_MAX_SIDE, SEG_NONFINITE, SEG_NOT_RESIDENT,  # noqa: F401
                      plaque_morphometry, segment_boxes)
from .spatial import (PAIR_MAX_CLASSES, PAIR_MAX_RADII, PAIR_MAX_RADIUS_Q, PAIR_MAX_SIDE, PAIR_WINDOW_MAX_CELLS, PAIR_WINDOW_MIN_CELL,  # noqa: F401
                      PAIR_RELABEL_FLAG_LABEL, PAIR_RELABEL_MAX_SIMS, envelope_summaries, pair_counts_device, pair_counts_relabel_device,
                      relabel_keys, relabel_table, spatial_envelope, spatial_radii_q, spatial_roi_q, spatial_stats, spatial_summaries,
                      window_area, window_from_tissue)
from .stain import normalize_region, stain_stats  # noqa: F401
from .stream import RegionTileStream, StripStream  # noqa: F401
from .tissue import tissue_counts, tissue_mask  # noqa: F401

from .basis import _check_basis_args  # noqa: F401
from .cells import _thres_bin  # noqa: F401
from .colour import _params_to_device  # noqa: F401
from .focus import _sharpness  # noqa: F401
from .segment import _segment_owner_rows  # noqa: F401
