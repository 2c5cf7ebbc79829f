"""The host classes of THE STAIN RULE (``include/amyloid_yolo.h``): :class:`StainBasis` and ``H_DAB``, :func:`stain_tables`,
:class:`StainStats` (the two concentration histograms of a slide) and :class:`StainMap` (the gains and tables that bring a slide's stain
strengths to a target's; ``remix=True`` maps between slides whose bases differ).  No stream is imported here: the tile stream checks
its ``stain=`` against :class:`StainMap`, and the passes that fill these classes are ``stain``'s."""
import math

import numpy as np
import torch

from .. import _lib
from .grid import hip_device


STAIN_BINS = _lib.CONSTANTS["AY_STAIN_BINS"]        # include/amyloid_yolo.h, THE STAIN RULE: bins of 1/64 OD


class StainBasis:
    """Two stain OD vectors (R, G, B), each normalised to unit length; ``M`` (float64 3x3) has them as rows 0 and 1 and their
    normalised cross product as row 2 (THE STAIN RULE, ``include/amyloid_yolo.h``).  ``ValueError`` for vectors that are not three
    finite numbers, of length 0, or (nearly) parallel: the basis would be singular."""

    def __init__(self, stain0, stain1):
        rows = []
        for v in (stain0, stain1):
            v = np.asarray(v, np.float64).reshape(-1)
            if v.shape != (3,) or not np.isfinite(v).all() or not np.linalg.norm(v) > 0:
                raise ValueError(f"StainBasis: a stain vector is three finite numbers, not all 0 (got {v!r})")
            rows.append(v / np.linalg.norm(v))
        cross = np.cross(rows[0], rows[1])
        if not np.linalg.norm(cross) > 1e-6:
            raise ValueError("StainBasis: the two stain vectors are parallel: the basis is singular")
        self.M = np.stack([rows[0], rows[1], cross / np.linalg.norm(cross)])
        self.M.setflags(write=False)

    @classmethod
    def of_unit_vectors(cls, stain0, stain1):
        """the basis whose rows 0 and 1 are exactly the two given unit vectors (they are checked and not divided again)"""
        self = cls(stain0, stain1)
        rows = [np.asarray(v, np.float64).reshape(3) for v in (stain0, stain1)]
        if not all(abs(np.linalg.norm(v) - 1.0) < 1e-12 for v in rows):
            raise ValueError("StainBasis.of_unit_vectors: a vector is not of unit length")
        cross = np.cross(rows[0], rows[1])
        self.M = np.stack([rows[0], rows[1], cross / np.linalg.norm(cross)])
        self.M.setflags(write=False)
        return self

    def __eq__(self, other):
        return isinstance(other, StainBasis) and np.array_equal(self.M, other.M)

    def __hash__(self):
        return hash(self.M.tobytes())

    def __repr__(self):
        return f"StainBasis({tuple(self.M[0])}, {tuple(self.M[1])})"


H_DAB = StainBasis((0.650, 0.704, 0.286), (0.268, 0.570, 0.776))     # Ruifrok & Johnston: hematoxylin, DAB


def stain_tables(basis, gains=(1.0, 1.0), target_basis=None):
    """The tables of THE STAIN RULE, built in float64 and rounded to fp32 once -> ``_lib.StainParams`` (host).  With ``target_basis``
    the concentrations unmixed on ``basis`` are mixed again on the target's vectors: ``A = inv(M) . diag(g0, g1, 1) . M_target``; ``D``
    stays ``basis``' own.  The device reads ``A`` as a table and needs no change for it."""
    v = np.arange(256, dtype=np.float64)
    Minv = np.linalg.inv(basis.M)
    A = Minv @ np.diag([float(gains[0]), float(gains[1]), 1.0]) @ (basis if target_basis is None else target_basis).M
    k = np.arange(257, dtype=np.float64)
    T = (256.0 * 10.0 ** (-k / 64.0) - 1.0) / 255.0
    tabs = [(-np.log10((v + 1.0) / 256.0)), Minv.reshape(-1), A.reshape(-1), T]
    if not all(np.isfinite(t).all() and np.isfinite(t.astype(np.float32)).all() for t in tabs):
        raise ValueError("stain_tables: the basis and gains give tables that are not finite in fp32")
    p = _lib.StainParams()
    for name, t in zip(("od", "D", "A", "T"), tabs):
        getattr(p, name)[:] = t.astype(np.float32).tolist()
    return p


def _params_to_device(p, dev):
    host = torch.from_numpy(np.frombuffer(bytes(p), dtype=np.uint8).copy())
    return host.to(dev)


class StainStats:
    """Histograms of the two stain concentrations over the tissue pixels of a slide (:func:`stain_stats`): ``hist`` int64 ``[2,
    512]`` in bins of 1/64 OD (``hist[s, b]``: pixels with ``b / 64 <= c_s < (b + 1) / 64``, negative concentrations in bin 0, those
    from 8 OD on in bin 511), ``n_tissue`` (every row of ``hist`` sums to it) and the ``basis`` they were unmixed on."""

    def __init__(self, hist, n_tissue, basis=H_DAB):
        hist = np.asarray(hist)
        if hist.shape != (2, STAIN_BINS) or hist.dtype.kind not in "iu" or (hist < 0).any():
            raise ValueError(f"StainStats: hist must be [2, {STAIN_BINS}] non-negative integers")
        if not isinstance(basis, StainBasis):
            raise ValueError("StainStats: basis must be a wsi.StainBasis")
        self.hist, self.n_tissue, self.basis = hist.astype(np.int64), int(n_tissue), basis
        if (self.hist.sum(1) != self.n_tissue).any():
            raise ValueError(f"StainStats: every row of hist must sum to n_tissue = {self.n_tissue}")

    def strength(self, p=99.0):
        """``(q0, q1)``: per stain the upper edge ``(b* + 1) / 64`` of the first bin whose cumulative count reaches ``K = max(1,
        ceil(p * n / 100))``, the ``p``-th percentile of its concentration over the tissue.  ``ValueError`` without tissue or for
        ``p`` outside (0, 100]."""
        p = float(p)
        if not 0.0 < p <= 100.0:       # a NaN fails both comparisons
            raise ValueError(f"StainStats.strength: p {p!r} outside (0, 100]")
        if self.n_tissue == 0:
            raise ValueError("StainStats.strength: no tissue pixel: a slide without tissue has no stain strength")
        K = max(1, math.ceil(p * self.n_tissue / 100.0))
        return tuple((int(np.searchsorted(np.cumsum(self.hist[s]), K, side="left")) + 1) / 64.0 for s in (0, 1))

    def positive_fraction(self, stain=1, thres=0.15):
        """``(share, j / 64)``: the share of tissue pixels whose concentration of ``stain`` (0 or 1) is at least ``j / 64``, ``j =
        round(thres * 64)``: the threshold moves to a bin edge and comes back as it took effect.  NaN without tissue."""
        if stain not in (0, 1):
            raise ValueError(f"StainStats.positive_fraction: stain {stain!r} is neither 0 nor 1")
        thres = float(thres)
        if not 0.0 <= thres < math.inf:
            raise ValueError(f"StainStats.positive_fraction: thres {thres!r} is no optical density >= 0")
        j = min(int(round(thres * 64.0)), STAIN_BINS)
        share = float(self.hist[stain, j:].sum()) / self.n_tissue if self.n_tissue else math.nan
        return share, j / 64.0


class StainMap:
    """The colour map that brings a slide's stain strengths to a target's (THE STAIN RULE): per stain the gain ``g_s = clip(t_s / q_s,
    1 / max_gain, max_gain)`` with ``(q0, q1) = source.strength(p)`` and ``(t0, t1)`` the target: a :class:`StainStats` (its
    ``strength(p)``; it must share the source's basis) or a pair of positive finite strengths, e.g.
    ``stain_stats(training_slide).strength()``.  There is no built-in target.  ``basis``, if given, must be the source's.
    ``gains`` is the pair; ``tables`` the host struct; ``params`` the struct on the current device, uploaded on first use.

    ``remix=True`` lifts the shared basis: the target is a :class:`StainStats` on ANY basis, or a pair of strengths plus
    ``target_basis=``, and the map unmixes on the source's basis and mixes again on the target's (:func:`stain_tables` with
    ``target_basis``): the step that carries a slide with its own estimated vectors (:func:`estimate_basis`) to a reference slide
    with other vectors.  The gains are taken as before, each strength on its own basis.  ``basis`` stays the source's -- what
    :func:`quantify_region` compares with the statistics' -- and ``target_basis`` is the basis mixed on (the source's without
    ``remix``).  With equal bases ``remix=True`` gives the tables of ``remix=False``."""

    def __init__(self, source, target, p=99.0, max_gain=4.0, basis=None, remix=False, target_basis=None):
        if not isinstance(source, StainStats):
            raise ValueError(f"StainMap: source must be a wsi.StainStats, got {type(source).__name__}")
        if basis is not None and basis != source.basis:
            raise ValueError("StainMap: basis differs from the basis of the source statistics")
        if target_basis is not None and not remix:
            raise ValueError("StainMap: target_basis needs remix=True")
        if target_basis is not None and not isinstance(target_basis, StainBasis):
            raise ValueError("StainMap: target_basis must be a wsi.StainBasis")
        max_gain = float(max_gain)
        if not 1.0 <= max_gain < math.inf:
            raise ValueError(f"StainMap: max_gain {max_gain!r} must be a finite number >= 1")
        q = source.strength(p)
        if isinstance(target, StainStats):
            if not remix and target.basis != source.basis:
                raise ValueError("StainMap: source and target statistics were made on different bases")
            if target_basis is not None and target_basis != target.basis:
                raise ValueError("StainMap: target_basis differs from the basis of the target statistics")
            t, target_basis = target.strength(p), target.basis if remix else None
        else:
            try:
                t = tuple(float(v) for v in target)
            except TypeError:
                raise ValueError(f"StainMap: target must be a wsi.StainStats or a pair of strengths, got {target!r}") from None
            if len(t) != 2 or not all(0.0 < v < math.inf for v in t):
                raise ValueError(f"StainMap: target strengths must be two positive finite numbers, got {target!r}")
        self._set(source.basis, tuple(min(max(ts / qs, 1.0 / max_gain), max_gain) for ts, qs in zip(t, q)), target_basis)
        self.source, self.target, self.p, self.max_gain = source, t, float(p), max_gain

    def _set(self, basis, gains, target_basis=None):
        self.basis, self.gains, self.target_basis = basis, gains, basis if target_basis is None else target_basis
        self.tables = stain_tables(basis, gains, target_basis)
        self._params = {}

    @classmethod
    def identity(cls, basis=H_DAB):
        """gains (1, 1) on ``basis``: the map that returns every uint8 value (for tests, and for the statistics' unmixing tables)"""
        if not isinstance(basis, StainBasis):
            raise ValueError("StainMap.identity: basis must be a wsi.StainBasis")
        self = cls.__new__(cls)
        self._set(basis, (1.0, 1.0))
        self.source, self.target, self.p, self.max_gain = None, None, None, None
        return self

    @property
    def params(self):
        dev = hip_device("the stain map has")
        if dev not in self._params:
            self._params[dev] = _params_to_device(self.tables, dev)
        return self._params[dev]
