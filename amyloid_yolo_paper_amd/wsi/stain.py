"""The stain passes over a raster: :func:`stain_stats` unmixes the tissue pixels of a slide into hematoxylin and DAB
(``ay_stain_hist_u8``, THE STAIN RULE) and :func:`normalize_region` gives the raster mapped through a :class:`StainMap`
(``ay_stain_apply_u8``); ``detect_region(stain=...)`` cuts every tile through the same map."""
import torch

from .. import _lib
from .._lib import check, ptr
from .colour import H_DAB, STAIN_BINS, StainBasis, StainMap, StainStats
from .grid import check_bg_level, check_probe_stride, check_raster, probed
from .stream import STRIP_ROWS, StripStream


def stain_stats(raster, shrink=1, bg_level=220, probe_stride=16, basis=H_DAB):
    """Stain statistics of a slide -> :class:`StainStats`: the two concentration histograms over its TISSUE pixels (THE TISSUE RULE
    with ``bg_level``), by ``ay_stain_hist_u8``.  The probe is :func:`tissue_mask`'s: every ``probe_stride``-th pixel of the (halved)
    slide, single source pixels (:func:`probe_view`); ``probe_stride=1`` is the exact rule, the 2x2 means of ``shrink=2`` included,
    at the cost of a full upload.  The strips of a :class:`StripStream` accumulate on the device; one read-back at the end."""
    bg_level, d = check_bg_level("stain_stats", bg_level), check_probe_stride("stain_stats", probe_stride)
    if not isinstance(basis, StainBasis):
        raise ValueError("stain_stats: basis must be a wsi.StainBasis")
    raster, shrink = probed(raster, d, shrink, 0, d)[:2]
    params = StainMap.identity(basis).params
    T = min(STRIP_ROWS, max(1, raster.shape[0] // shrink))
    strips = StripStream(raster, T, T, shrink)
    L = _lib.lib()
    hist = torch.zeros(2 * STAIN_BINS + 1, device=strips.dev, dtype=torch.int64)
    strips.each(lambda k, j, valid, width: check(
        L.ay_stain_hist_u8(*strips.args(k, valid, width), bg_level, ptr(params), ptr(hist), _lib.stream_ptr()), "ay_stain_hist_u8"))
    h = hist.cpu().numpy()
    return StainStats(h[:2 * STAIN_BINS].reshape(2, STAIN_BINS), h[2 * STAIN_BINS], basis)


def normalize_region(raster, stain, shrink=1, device=False):
    """The (halved) raster through the stain map, in THE STAIN RULE's uint8 form -> uint8 ``[H // shrink, W // shrink, 3]``: a NumPy
    array, or with ``device=True`` a tensor on the device (:class:`SlideSampler` reads device rasters in place: the way to train on
    normalised slides; also for a look at the result).  Strip by strip through ``ay_stain_apply_u8``."""
    if not isinstance(stain, StainMap):
        raise ValueError(f"normalize_region: stain must be a wsi.StainMap, got {type(stain).__name__}")
    H, W = check_raster("normalize_region", raster, shrink)
    T = min(STRIP_ROWS, H)
    strips = StripStream(raster, T, T, shrink)
    L = _lib.lib()
    params = stain.params
    out = torch.empty(H, W, 3, device=strips.dev, dtype=torch.uint8)

    def apply(k, j, valid, width):
        if valid // shrink:
            check(L.ay_stain_apply_u8(*strips.args(k, valid, width), ptr(params), ptr(out[j * T:]), W * 3, _lib.stream_ptr()),
                  "ay_stain_apply_u8")

    strips.each(apply)
    return out if device else out.cpu().numpy()
