"""THE LOAD RULE of include/amyloid_yolo.h restated in NumPy (TEST INFRASTRUCTURE ONLY): boolean images, integer bins, slicing and
bincount; the box edges as float32 NumPy operations in the order the rule writes them.  Nothing here comes from the product: the
pixel classes are tissue_reference's and stain_reference's, the grid is restated."""
import numpy as np

import stain_reference as sref
import tissue_reference as tr

F32 = np.float32
MIN_CELL = 16
FLAG_NONFINITE = 1


def thres_bin(thres):
    """an optical density -> the rule's integer threshold, min(round(thres * 64), 512)"""
    return min(int(round(float(thres) * 64.0)), sref.BINS)


def grid(H, W, cell):
    return -(-H // cell), -(-W // cell)


def classes(region, shrink, bg, params, stain):
    """-> (tissue bool [h, w], bin q int64 [h, w]) of the (halved) image of a region"""
    img = sref.image(region, shrink)
    return tr.tissue(region, shrink, bg), sref.bins(sref.concentrations(img, params)[..., stain])


def edges(rows, H, W):
    """rows [M, >= 4] -> (finite bool [M], int64 [M, 4] = lo_x, lo_y, hi_x, hi_y; zeros for a row that is not finite)"""
    r = np.asarray(rows, F32).reshape(-1, np.shape(rows)[-1])[:, :4]
    finite = np.isfinite(r).all(1)
    r = np.where(finite[:, None], r, F32(0))
    assert r.dtype == F32
    out = np.zeros((len(r), 4), np.int64)
    for k, n in ((0, W), (1, H), (2, W), (3, H)):
        e = np.minimum(np.maximum(np.ceil(r[:, k] - F32(0.5)), F32(0)), F32(n))
        assert e.dtype == F32
        out[:, k] = e.astype(np.int64)
    out[~finite] = 0
    return finite, out


def owned_pixels(rows, H, W):
    """the closed form of a box's `pixels` once every strip has been seen: (hi_x - lo_x) * (hi_y - lo_y), 0 for an inverted box"""
    _, e = edges(rows, H, W)
    return np.maximum(e[:, 2] - e[:, 0], 0) * np.maximum(e[:, 3] - e[:, 1], 0)


def new_outputs(H, W, cell, M):
    """zeroed (cells int64 [Gy, Gx, 3], boxes int64 [M, 4], flags int64 [1])"""
    return np.zeros(grid(H, W, cell) + (3,), np.int64), np.zeros((M, 4), np.int64), np.zeros(1, np.int64)


def add_region(region, shrink, origin_y, origin_x, H, W, bg, params, stain, j, cell, cells, rows, boxes, flags):
    """one call of the rule on a region whose (halved) image has its top-left at (origin_y, origin_x) of the H x W slide: ADDS to
    cells (or None) and to boxes / flags (rows None or empty: untouched)"""
    t, q = classes(region, shrink, bg, params, stain)
    add_classes(t, q, origin_y, origin_x, H, W, j, cell, cells, rows, boxes, flags)


def add_classes(t, q, origin_y, origin_x, H, W, j, cell, cells, rows, boxes, flags):
    """add_region on the pixel classes (t, q) of the region's (halved) image (a test that sweeps j and cell computes them once)"""
    h, w = t.shape
    if h == 0 or w == 0:
        return
    assert origin_y >= 0 and origin_x >= 0 and origin_y + h <= H and origin_x + w <= W
    pos = t & (q >= j)
    if cells is not None:
        assert cell >= MIN_CELL
        gy, gx = grid(H, W, cell)
        idx = (((origin_y + np.arange(h)) // cell)[:, None] * gx + ((origin_x + np.arange(w)) // cell)[None]).ravel()
        flat = cells.reshape(gy * gx, 3)
        flat[:, 0] += np.bincount(idx[t.ravel()], minlength=gy * gx)
        flat[:, 1] += np.bincount(idx[pos.ravel()], minlength=gy * gx)
        flat[:, 2] += np.bincount(idx[pos.ravel()], weights=q.ravel()[pos.ravel()], minlength=gy * gx).astype(np.int64)   # < 2^53: exact
    if rows is not None and len(rows):
        finite, e = edges(rows, H, W)
        if not finite.all():
            flags[0] |= FLAG_NONFINITE
        for m in np.flatnonzero(finite):
            ax, bx = max(e[m, 0], origin_x) - origin_x, min(e[m, 2], origin_x + w) - origin_x
            ay, by = max(e[m, 1], origin_y) - origin_y, min(e[m, 3], origin_y + h) - origin_y
            if ax >= bx or ay >= by:
                continue
            boxes[m, 0] += (bx - ax) * (by - ay)
            boxes[m, 1] += t[ay:by, ax:bx].sum()
            boxes[m, 2] += pos[ay:by, ax:bx].sum()
            boxes[m, 3] += q[ay:by, ax:bx][pos[ay:by, ax:bx]].sum()


def load(raster, shrink, bg, params, stain, j, cell, rows=None, cuts=None):
    """the whole slide -> (cells, boxes, flags).  `cuts`: rows of the (halved) slide at which it is cut into strips (each strip one
    call of the rule); None is one call."""
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    cells, boxes, flags = new_outputs(H, W, cell, 0 if rows is None else len(rows))
    bounds = [0] + list(cuts or []) + [H]
    for a, b in zip(bounds[:-1], bounds[1:]):
        add_region(raster[a * shrink:b * shrink], shrink, a, 0, H, W, bg, params, stain, j, cell, cells, rows, boxes, flags)
    return cells, boxes, flags


def morphometry(boxes, mpp=None):
    """plain loops over the rows of boxes [M, 4] -> dict of float64 lists"""
    nan = float("nan")
    out = {"area_px": [], "fill": [], "mean_od": []}
    if mpp is not None:
        out["area_um2"], out["equiv_diameter_um"] = [], []
    for pixels, _, positive, bin_sum in np.asarray(boxes).tolist():
        out["fill"].append(positive / pixels if pixels else nan)
        out["area_px"].append(float(positive) if positive else nan)
        out["mean_od"].append((bin_sum / positive + 0.5) / 64.0 if positive else nan)
        if mpp is not None:
            out["area_um2"].append(positive * mpp ** 2 if positive else nan)
            out["equiv_diameter_um"].append(2.0 * (positive * mpp ** 2 / np.pi) ** 0.5 if positive else nan)
    return out


def random_boxes(n, H, W, seed, cuts=()):
    """n rows [n, 7] fp32: boxes of detection size scattered over the slide and beyond its borders, a few centred on the strip cuts,
    fractional coordinates; they overlap each other freely"""
    rng = np.random.default_rng(seed)
    cx, cy = rng.uniform(-20, W + 20, n), rng.uniform(-20, H + 20, n)
    for k, c in enumerate(cuts):
        cy[k::11] = c + rng.uniform(-2, 2, len(cy[k::11]))
    hw, hh = rng.uniform(0.3, 45, n), rng.uniform(0.3, 45, n)
    rows = np.zeros((n, 7), F32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3] = cx - hw, cy - hh, cx + hw, cy + hh
    rows[:, 4:6] = rng.uniform(0.5, 1, (n, 2))
    rows[:, 6] = rng.integers(0, 2, n)
    return rows
