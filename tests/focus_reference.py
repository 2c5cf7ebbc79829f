"""THE FOCUS RULE of include/amyloid_yolo.h restated in NumPy int64 (TEST INFRASTRUCTURE ONLY): whole-image arrays, shifted slices and
bincount.  Nothing here comes from the product: the bytes and the tissue test are tissue_reference's, the box edges load_reference's
(the rule takes THE LOAD RULE's ownership), the grid is restated."""
import numpy as np

import load_reference as lr
import tissue_reference as tr

MIN_CELL = 16
FLAG_NONFINITE = 1
LAP_MAX = 1020


def grid(H, W, cell):
    return -(-H // cell), -(-W // cell)


def luma(img):
    """uint8 [H, W, 3] -> int64 [H, W]: (77 * b0 + 150 * b1 + 29 * b2 + 128) >> 8"""
    b = np.asarray(img).astype(np.int64)
    return (77 * b[..., 0] + 150 * b[..., 1] + 29 * b[..., 2] + 128) >> 8


def evaluate(raster, shrink=1, bg=220):
    """the whole (halved) slide -> (evaluated bool [H, W], lap int64 [H, W], 0 where not evaluated)"""
    img = tr.halve(raster) if shrink == 2 else np.asarray(raster)
    t, g = tr.tissue(raster, shrink, bg), luma(img)
    H, W = t.shape
    ev, lap = np.zeros((H, W), bool), np.zeros((H, W), np.int64)
    if H >= 3 and W >= 3:
        ev[1:-1, 1:-1] = t[1:-1, 1:-1] & t[1:-1, :-2] & t[1:-1, 2:] & t[:-2, 1:-1] & t[2:, 1:-1]
        lap[1:-1, 1:-1] = 4 * g[1:-1, 1:-1] - g[1:-1, :-2] - g[1:-1, 2:] - g[:-2, 1:-1] - g[2:, 1:-1]
    lap[~ev] = 0
    assert np.abs(lap).max(initial=0) <= LAP_MAX
    return ev, lap


def new_outputs(H, W, cell, M):
    """zeroed (cells int64 [Gy, Gx, 3], boxes int64 [M, 3], flags int64 [1])"""
    return np.zeros(grid(H, W, cell) + (3,), np.int64), np.zeros((M, 3), np.int64), np.zeros(1, np.int64)


def add_owned(ev, lap, own_y0, own_y1, cell, cells, rows, boxes, flags):
    """one call of the rule: ADDS the sums of the evaluated pixels with own_y0 <= Y < own_y1 to cells (or None) and to boxes / flags
    (rows None or empty: untouched).  A call without a pixel to evaluate adds nothing and flags nothing."""
    H, W = ev.shape
    c0, c1 = max(own_y0, 1), min(own_y1, H - 1)
    if c0 >= c1 or W < 3:
        return
    own = np.zeros_like(ev)
    own[c0:c1] = ev[c0:c1]
    if cells is not None:
        assert cell >= MIN_CELL
        gy, gx = grid(H, W, cell)
        idx = ((np.arange(H) // cell)[:, None] * gx + (np.arange(W) // cell)[None])[own]
        flat = cells.reshape(gy * gx, 3)
        flat[:, 0] += np.bincount(idx, minlength=gy * gx)
        np.add.at(flat[:, 1], idx, lap[own])
        np.add.at(flat[:, 2], idx, lap[own] ** 2)
    if rows is not None and len(rows):
        finite, e = lr.edges(rows, H, W)
        if not finite.all():
            flags[0] |= FLAG_NONFINITE
        for m in np.flatnonzero(finite):
            lo_x, lo_y, hi_x, hi_y = e[m]
            if lo_x >= hi_x or lo_y >= hi_y:
                continue
            o, v = own[lo_y:hi_y, lo_x:hi_x], lap[lo_y:hi_y, lo_x:hi_x]
            boxes[m] += (o.sum(), v[o].sum(), (v[o] ** 2).sum())


def focus(raster, shrink=1, bg=220, cell=128, rows=None, strips=None):
    """the whole slide -> (cells, boxes, flags).  `strips`: ownership ranges [(own_y0, own_y1), ...], each one call of the rule; None is
    one call that owns every row."""
    ev, lap = evaluate(raster, shrink, bg)
    H, W = ev.shape
    cells, boxes, flags = new_outputs(H, W, cell, 0 if rows is None else len(rows))
    for a, b in strips if strips is not None else [(0, H)]:
        add_owned(ev, lap, a, b, cell, cells, rows, boxes, flags)
    return cells, boxes, flags


def sharpness(n, s1, s2):
    """plain Python per entry: s2 / n - (s1 / n)**2 in float64, NaN where n == 0"""
    out = [s2_ / n_ - (s1_ / n_) ** 2 if n_ else float("nan")
           for n_, s1_, s2_ in zip(np.ravel(n).tolist(), np.ravel(s1).tolist(), np.ravel(s2).tolist())]
    return np.asarray(out, np.float64).reshape(np.shape(n))


def glass_blobs(r, seed, n=6, radius=(2, 9)):
    """a copy of raster r with discs of glass (255) punched in"""
    rng = np.random.default_rng(seed)
    out = r.copy()
    yy, xx = np.mgrid[:r.shape[0], :r.shape[1]]
    for _ in range(n):
        cy, cx, rad = rng.integers(0, r.shape[0]), rng.integers(0, r.shape[1]), rng.integers(*radius)
        out[(yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad] = 255
    return out


def texture(H, W, seed, lo=40, hi=200):
    """random bytes lo .. hi - 1 in every channel: tissue at any bg_level >= hi"""
    return np.random.default_rng(seed).integers(lo, hi, size=(H, W, 3), dtype=np.uint8)


def checkerboard(H, W):
    """pixels 0 and 255 alternating: every Laplacian is +-1020 (luma of a grey pixel is its value)"""
    v = (((np.arange(H)[:, None] + np.arange(W)[None]) & 1) * 255).astype(np.uint8)
    return np.repeat(v[:, :, None], 3, 2)
