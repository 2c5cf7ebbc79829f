"""Stain basis estimation: :func:`estimate_basis` finds the slide's own two stain vectors (``ay_stain_moments_u8``,
``ay_stain_direction_hist_u8``, THE BASIS RULE) for every ``basis=`` of the package; :func:`basis_plane` and :func:`basis_vectors` are
its two host steps."""
import math

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from .colour import H_DAB, StainBasis, _params_to_device
from .grid import check_bg_level, check_probe_stride, probed
from .stream import STRIP_ROWS, ResidentStrips, StripStream


BASIS_OD_SCALE, BASIS_OD_MAX, BASIS_MOMENT_WORDS, BASIS_DIR_BINS = (                       # include/amyloid_yolo.h, THE BASIS RULE
    _lib.CONSTANTS["AY_BASIS_" + n] for n in ("OD_SCALE", "OD_MAX", "MOMENT_WORDS", "DIR_BINS"))
BASIS_STRIP = STRIP_ROWS    # rows of the (halved) slide per strip of estimate_basis: stain_stats'


def basis_tables():
    """``odq`` of THE BASIS RULE, built in float64 -> ``_lib.StainBasisParams`` (host)"""
    v = np.arange(256, dtype=np.float64)
    p = _lib.StainBasisParams()
    p.odq[:] = np.rint(-np.log10((v + 1.0) / 256.0) * BASIS_OD_SCALE).astype(np.int64).tolist()
    return p


def _angle(a, b):
    """degrees between two unit vectors"""
    return math.degrees(math.acos(min(1.0, max(-1.0, float(np.dot(a, b))))))


def basis_plane(moments):
    """THE BASIS RULE's plane from the 11 words of ``ay_stain_moments_u8`` -> ``(eq1, eq2, eigenvalues)``: int32 ``[3]`` each and the
    three eigenvalues of the covariance of the integer optical density, largest first.  ``ValueError`` with fewer than 2 selected
    pixels or a second eigenvalue that is not positive: no stain plane."""
    m = [int(v) for v in moments]
    if len(m) != BASIS_MOMENT_WORDS:
        raise ValueError(f"basis_plane: moments are {BASIS_MOMENT_WORDS} words, got {len(m)}")
    n, S = m[1], m[2:5]
    if n < 2:
        raise ValueError(f"basis_plane: {n} selected pixel(s): a slide without stained tissue has no stain plane")
    cov, at = np.empty((3, 3), np.float64), 5
    for c in range(3):
        for d in range(c, 3):
            cov[c, d] = cov[d, c] = (n * m[at] - S[c] * S[d]) / (n * (n - 1))      # exact integers, divided once
            at += 1
    w, V = np.linalg.eigh(cov)                                                      # ascending
    if not w[1] > 0.0:
        raise ValueError("basis_plane: the optical densities of the selected pixels lie on a line: no stain plane")
    e1, e2 = V[:, 2], V[:, 1]
    if e1.sum() < 0.0:
        e1 = -e1
    if e2[int(np.argmax(np.abs(e2)))] < 0.0:
        e2 = -e2
    return np.rint(BASIS_OD_SCALE * e1).astype(np.int32), np.rint(BASIS_OD_SCALE * e2).astype(np.int32), tuple(float(x) for x in w[::-1])


def basis_vectors(hist, eq1, eq2, alpha=1.0, prior=None, max_angle=None):
    """THE BASIS RULE's two vectors from the direction histogram (the first 512 words of ``ay_stain_direction_hist_u8``'s) ->
    ``(vectors, angle_to_prior, fell_back)``: float64 ``[2, 3]`` unit vectors in the order of ``prior``'s stains (default ``H_DAB``),
    their angles to the prior's in degrees BEFORE the guard, and whether the guard replaced them (``max_angle=None``: never)."""
    prior = H_DAB if prior is None else prior
    h = np.asarray(hist).reshape(-1)[:BASIS_DIR_BINS].astype(np.int64)
    n = int(h.sum())
    if n == 0:
        raise ValueError("basis_vectors: no selected pixel on the half plane of the first direction")
    cum = np.cumsum(h)
    q1, q2 = np.asarray(eq1, np.float64), np.asarray(eq2, np.float64)
    ends = []
    for K in (max(1, math.ceil(alpha * n / 100.0)), max(1, math.ceil((100.0 - alpha) * n / 100.0))):
        d = (int(np.searchsorted(cum, K, side="left")) - BASIS_DIR_BINS // 2 + 0.5) / (BASIS_DIR_BINS // 2)
        v = (1.0 - abs(d)) * q1 + d * q2
        ends.append(v / np.linalg.norm(v))
    m0, m1 = prior.M[0], prior.M[1]
    if float(np.dot(ends[0], m1) + np.dot(ends[1], m0)) > float(np.dot(ends[0], m0) + np.dot(ends[1], m1)):
        ends.reverse()
    angles = (_angle(ends[0], m0), _angle(ends[1], m1))
    fell = tuple(max_angle is not None and a > max_angle for a in angles)
    return np.stack([prior.M[s] if fell[s] else ends[s] for s in (0, 1)]), angles, fell


class StainEstimate:
    """What :func:`estimate_basis` found: ``basis`` (a :class:`StainBasis`, ready for every ``basis=`` of this module) and ``vectors``
    float64 ``[2, 3]`` (its first two rows); ``moments`` int64 ``[11]`` and ``hist`` int64 ``[512]`` as the device summed them,
    ``n_tissue``, ``n_selected`` and ``outside`` (selected pixels with ``p1 <= 0``); ``plane`` = ``(eq1, eq2)`` int32 and
    ``eigenvalues`` (largest first); ``angle_to_prior`` (degrees, a pair, before the guard) and ``fell_back`` (bools, a pair: the
    guard put the prior's vector there); ``alpha`` and ``beta`` as they took effect (``beta`` a multiple of 1/1024)."""

    def __init__(self, moments, hist, alpha, beta_q, prior, max_angle):
        moments, hist = np.asarray(moments, np.int64), np.asarray(hist, np.int64)
        self.moments, self.hist = moments, hist[:BASIS_DIR_BINS].copy()
        self.n_tissue, self.n_selected, self.outside = int(moments[0]), int(moments[1]), int(hist[BASIS_DIR_BINS])
        eq1, eq2, self.eigenvalues = basis_plane(moments)
        self.plane = (eq1, eq2)
        self.vectors, self.angle_to_prior, self.fell_back = basis_vectors(self.hist, eq1, eq2, alpha, prior, max_angle)
        self.basis = StainBasis.of_unit_vectors(self.vectors[0], self.vectors[1])      # rows 0 and 1 are `vectors`, bit for bit
        self.alpha, self.beta = float(alpha), beta_q / BASIS_OD_SCALE


def _check_basis_args(beta, alpha, prior, max_angle):
    """the host checks of :func:`estimate_basis` -> (beta_q, alpha, max_angle)"""
    if not isinstance(prior, StainBasis):
        raise ValueError("estimate_basis: prior must be a wsi.StainBasis")
    beta, alpha = float(beta), float(alpha)
    if not 0.0 <= beta <= 2.4:             # a NaN fails both comparisons
        raise ValueError(f"estimate_basis: beta {beta!r} outside 0 .. 2.4 (optical density)")
    if not 0.0 < alpha < 50.0:
        raise ValueError(f"estimate_basis: alpha {alpha!r} outside (0, 50) per cent")
    if max_angle == "half":
        max_angle = 0.5 * _angle(prior.M[0], prior.M[1])
    elif max_angle is not None:
        if isinstance(max_angle, (bool, str)) or not 0.0 < float(max_angle) <= 90.0:
            raise ValueError(f"estimate_basis: max_angle {max_angle!r} outside (0, 90] degrees")
        max_angle = float(max_angle)
    return int(np.rint(beta * BASIS_OD_SCALE)), alpha, max_angle


def estimate_basis(raster, shrink=1, bg_level=220, probe_stride=16, beta=0.15, alpha=1.0, prior=H_DAB, max_angle="half"):
    """The slide's own two stain vectors -> :class:`StainEstimate`: a Macenko-style estimate (THE BASIS RULE in
    ``include/amyloid_yolo.h``), integers only on the device.  Over the tissue pixels whose integer optical density reaches ``beta``
    in every channel, pass 1 (``ay_stain_moments_u8``) sums the moments, the host takes the plane of the two largest eigenvalues,
    pass 2 (``ay_stain_direction_hist_u8``) counts the directions inside the plane, and the ``alpha``-th and ``(100 - alpha)``-th
    percentile directions are the two vectors, assigned to the stains of ``prior`` by the better pairing.

    The probe and the strips are :func:`stain_stats`': every ``probe_stride``-th pixel of the (halved) slide, single source pixels;
    ``probe_stride=1`` is the exact rule.  Each pass goes through one :class:`StripStream` and is read back once.  The result goes
    wherever a ``basis=`` is taken -- ``stain_stats(raster, basis=est.basis)``, :func:`stain_load`, :func:`segment_boxes` -- and,
    through the statistics, into ``StainMap(stats, target, remix=True)``.

    Guard: a vector further than ``max_angle`` degrees from its prior vector is replaced by the prior's and reported in
    ``fell_back``.  The default ``"half"`` is half the angle between the prior's two vectors (``H_DAB``: about 18.6), with which the two
    results can neither swap nor coincide; ``None`` disables the guard.

    LIMIT: the extreme on the DAB side is the ``alpha``-th percentile of the selected pixels.  On a slide whose DAB-positive share
    of selected pixels is below ``alpha`` per cent that extreme is not DAB; the guard catches it or the caller lowers ``alpha`` (on
    the synthetic slide of ``tests/stain_basis_reference.py`` with 0.4 % DAB, ``alpha=1`` lands 36 degrees off and ``alpha=0.1`` 3.6).

    ``ValueError`` before any launch for ``bg_level`` outside 0 .. 256, ``probe_stride < 1``, ``beta`` outside [0, 2.4], ``alpha``
    outside (0, 50), a ``prior`` that is no :class:`StainBasis`, ``max_angle`` outside (0, 90]; after pass 1 for a slide with fewer
    than 2 selected pixels or without a plane (one colour)."""
    bg_level, d = check_bg_level("estimate_basis", bg_level), check_probe_stride("estimate_basis", probe_stride)
    beta_q, alpha, max_angle = _check_basis_args(beta, alpha, prior, max_angle)
    resident = isinstance(raster, torch.Tensor)
    if getattr(raster, "ndim", 0) != 3 or raster.shape[2] != 3 or raster.dtype != (torch.uint8 if resident else np.uint8) or (
            resident and not raster.is_cuda):
        raise ValueError("estimate_basis: raster must be a uint8 [H,W,3] NumPy array or tensor on the device")
    raster, shrink = probed(raster, d, shrink, 0, d)[:2]
    T = min(BASIS_STRIP, max(1, raster.shape[0] // shrink))
    L = _lib.lib()

    def one_pass(words, call):
        """``call(region, params, out)`` on every strip, adding to ``out``; one read-back"""
        strips = ResidentStrips(raster, T, shrink) if resident else StripStream(raster, T, T, shrink)
        with torch.cuda.device(strips.dev):
            params = _params_to_device(basis_tables(), strips.dev)
            out = torch.zeros(words, device=strips.dev, dtype=torch.int64)
            strips.each(lambda k, j, valid, width: call(strips.args(k, valid, width), ptr(params), ptr(out)))
            return out.cpu().numpy()

    moments = one_pass(BASIS_MOMENT_WORDS, lambda region, params, out: check(
        L.ay_stain_moments_u8(*region, bg_level, beta_q, params, out, _lib.stream_ptr()), "ay_stain_moments_u8"))
    eq1, eq2, _ = basis_plane(moments)
    hist = one_pass(BASIS_DIR_BINS + 2, lambda region, params, out: check(
        L.ay_stain_direction_hist_u8(*region, bg_level, beta_q, *(int(v) for v in eq1), *(int(v) for v in eq2), params, out,
                                     _lib.stream_ptr()), "ay_stain_direction_hist_u8"))
    return StainEstimate(moments, hist, alpha, beta_q, prior, max_angle)
