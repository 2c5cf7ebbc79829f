"""NumPy restatement of THE PAIR WINDOW RULE of include/amyloid_yolo.h (TEST INFRASTRUCTURE ONLY): the border distance of
minus-sampling measured to the edge of a MASK on cells.  By brute force: the squared distance from every row to the clipped rectangle
of EVERY OUT cell and to the four half-planes outside the slide, int64, then `wbd` by integer comparison against a table of squares;
the pairs by the brute-force loop of spatial_reference with this eligibility.

Nothing here comes from the product; the positions, the conversions and the host formulas are spatial_reference's."""
import math

import numpy as np

from spatial_reference import positions, radii_q, roi_q, summaries  # noqa: F401  (re-exported for the tests)

MIN_CELL = 16
CHUNK = 512


def grid_of(H, W, cell):
    return -(-H // cell), -(-W // cell)


def d2_out(qx, qy, mask, cell, H, W):
    """int64 [M]: the squared distance from (qx, qy) to the nearest OUT position: outside the slide, or in a zero cell of the mask"""
    mask = np.asarray(mask)
    assert cell >= MIN_CELL and mask.shape == grid_of(H, W, cell), (mask.shape, grid_of(H, W, cell))
    qx, qy = np.asarray(qx, np.int64), np.asarray(qy, np.int64)
    S = 4 * cell
    best = np.minimum(np.minimum(qx + 1, 4 * W - qx), np.minimum(qy + 1, 4 * H - qy)) ** 2            # the four half-planes
    out = np.argwhere(mask == 0)
    for lo in range(0, len(out), CHUNK):
        gy, gx = out[lo:lo + CHUNK, 0][None, :], out[lo:lo + CHUNK, 1][None, :]
        x0, x1 = gx * S, np.minimum(gx * S + S, 4 * W) - 1                                              # the cell, cut by the slide
        y0, y1 = gy * S, np.minimum(gy * S + S, 4 * H) - 1
        dx = np.maximum(np.maximum(x0 - qx[:, None], qx[:, None] - x1), 0)
        dy = np.maximum(np.maximum(y0 - qy[:, None], qy[:, None] - y1), 0)
        best = np.minimum(best, (dx * dx + dy * dy).min(1, initial=np.int64(1) << 62))
    return best


def wbd_of(d2, r_max):
    """the largest integer d in -1 .. r_max with d * d < d2, by comparison against the squares"""
    squares = np.arange(int(r_max) + 1, dtype=np.int64) ** 2
    return (np.searchsorted(squares, np.asarray(d2, np.int64), side="left") - 1).astype(np.int64)       # the number of d with d*d < d2, less one


def window_bd(qx, qy, mask, cell, H, W, r_max):
    return wbd_of(d2_out(qx, qy, mask, cell, H, W), r_max)


def window_bd_by_positions(qx, qy, mask, cell, H, W, r_max):
    """a second formulation for TINY slides: every OUT position of the lattice within r_max + 1 of the slide, one by one"""
    mask = np.asarray(mask)
    S, m = 4 * cell, int(r_max) + 1
    xs, ys = np.arange(-m, 4 * W + m, dtype=np.int64), np.arange(-m, 4 * H + m, dtype=np.int64)
    X, Y = np.meshgrid(xs, ys)
    inside = (X >= 0) & (X <= 4 * W - 1) & (Y >= 0) & (Y <= 4 * H - 1)
    out = ~inside
    out[inside] = mask[Y[inside] // S, X[inside] // S] == 0
    px, py = X[out], Y[out]
    res = []
    for x, y in zip(np.asarray(qx, np.int64), np.asarray(qy, np.int64)):
        d2 = int(((px - x) ** 2 + (py - y) ** 2).min())
        d = -1
        while d < r_max and (d + 1) * (d + 1) < d2:
            d += 1
        res.append(d)
    return np.array(res, np.int64)


def rect_bd(qx, qy, H, W, roi=None):
    X1, Y1, X2, Y2 = (0, 0, 4 * W - 1, 4 * H - 1) if roi is None else (int(v) for v in roi)
    assert X1 <= X2 and Y1 <= Y2
    return np.minimum(np.minimum(qx - X1, X2 - qx), np.minimum(qy - Y1, Y2 - qy))


def pair_counts_window(rows, H, W, C, min_conf, rq, mask, cell, roi=None, border=True):
    """THE PAIR WINDOW RULE by brute force -> pairs int64 [C,C,B], centres int32 [C,B], nn int32 [M,C,2], bd int32 [M], stats int32
    [2C+3]: the outputs of spatial_reference.pair_counts"""
    rq = np.asarray(rq, np.int64)
    assert 1 <= len(rq) <= 32 and rq[0] >= 1 and rq[-1] <= 32767 and (np.diff(rq) > 0).all() and 1 <= C <= 8
    qx, qy, cls, below, flagged, bits = positions(rows, H, W, C, min_conf)
    M, B = len(cls), len(rq)
    counted = cls >= 0
    dist = np.minimum(rect_bd(qx, qy, H, W, roi), window_bd(qx, qy, mask, cell, H, W, rq[-1]))
    eligible = counted[:, None] & (dist[:, None] >= (rq[None, :] if border else 0 * rq[None, :]))
    bd = np.where(counted & (dist >= 0), dist, -1).astype(np.int32)
    stats = np.zeros(2 * C + 3, np.int32)
    for c in range(C):
        stats[c] = (cls == c).sum()
        stats[C + c] = ((cls == c) & (dist >= 0)).sum()
    stats[2 * C:] = below, flagged, bits
    centres = np.stack([eligible[cls == a].sum(0) for a in range(C)]).astype(np.int32).reshape(C, B)
    r2 = rq * rq
    pairs, nn = np.zeros((C, C, B), np.int64), np.full((M, C, 2), -1, np.int32)
    idx = np.flatnonzero(counted)                                    # ascending: the first minimum below is the lowest row index
    px, py, pc = qx[idx], qy[idx], cls[idx]
    far = np.int64(1) << 62
    for lo in range(0, len(idx), CHUNK):
        me = idx[lo:lo + CHUNK]
        d2 = (qx[me][:, None] - px[None, :]) ** 2 + (qy[me][:, None] - py[None, :]) ** 2
        d2[np.arange(len(me)), lo + np.arange(len(me))] = far                                       # j != i
        for b in range(C):
            db = np.where(pc[None, :] == b, d2, far)
            for k in range(B):                                                                      # equality counts
                n = (db <= r2[k]).sum(1)
                for a in range(C):
                    pairs[a, b, k] += n[eligible[me, k] & (cls[me] == a)].sum()
            j = db.argmin(1)
            best = db[np.arange(len(me)), j]
            hit = best <= r2[-1]
            nn[me[hit], b, 0], nn[me[hit], b, 1] = best[hit], idx[j[hit]]
    return pairs, centres, nn, bd, stats


def window_area(mask, cell, H, W, roi=None):
    """the positions of the slide in IN cells and inside the ROI, over 16: cell by cell"""
    X1, Y1, X2, Y2 = (0, 0, 4 * W - 1, 4 * H - 1) if roi is None else (int(v) for v in roi)
    S, n = 4 * cell, 0
    for gy, gx in np.argwhere(np.asarray(mask) != 0):
        nx = min(min(gx * S + S, 4 * W) - 1, X2) - max(gx * S, X1) + 1
        ny = min(min(gy * S + S, 4 * H) - 1, Y2) - max(gy * S, Y1) + 1
        n += max(int(nx), 0) * max(int(ny), 0)
    return n / 16.0


def window_from_tissue(tissue, H, W, cell, min_tissue=0.5):
    tissue = np.asarray(tissue)
    Gy, Gx = grid_of(H, W, cell)
    assert tissue.shape == (Gy, Gx)
    out = np.zeros((Gy, Gx), bool)
    for gy in range(Gy):
        for gx in range(Gx):
            n = min(cell, H - gy * cell) * min(cell, W - gx * cell)
            out[gy, gx] = int(tissue[gy, gx]) >= max(1, math.ceil(min_tissue * n))
    return out


# ---- the cases of the tests ---------------------------------------------------------------------------------------------------------
SLIDE_H, SLIDE_W, CLASSES, CELL = 770, 1030, 2, 16               # 49 x 65 cells, the last row and column cut (2 and 6 px)
RADII_PX = (6, 12, 24, 48, 96)
SIZES = [1, 63, 64, 65, 257, 1025]


def blob_mask(Gy, Gx, seed, holes=6):
    """a tissue-like mask: an ellipse with a wavy outline that touches the slide's edge at the left, with `holes` round holes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:Gy, 0:Gx].astype(np.float64)
    cy, cx = 0.5 * Gy, 0.42 * Gx
    ang = np.arctan2(y - cy, x - cx)
    rad = 1.0 + 0.12 * np.sin(3 * ang + rng.uniform(0, 6)) + 0.08 * np.sin(7 * ang + rng.uniform(0, 6))
    m = ((y - cy) / (0.46 * Gy)) ** 2 + ((x - cx) / (0.47 * Gx)) ** 2 <= rad ** 2
    for _ in range(holes):
        hy, hx, hr = rng.uniform(0.2, 0.8) * Gy, rng.uniform(0.15, 0.7) * Gx, rng.uniform(0.03, 0.07) * min(Gy, Gx)
        m &= (y - hy) ** 2 + (x - hx) ** 2 > hr ** 2
    return m.astype(np.uint8)


def ragged_rows(M, seed, H=SLIDE_H, W=SLIDE_W, C=CLASSES, bad=0.05):
    """M boxes: two thirds around 12 parents (offspring sigma 50 px), a third uniform over the slide and 20 px beyond it; about `bad`
    of the rows flagged (NaN coordinate, a label that is no class) or below 0.5"""
    rng = np.random.default_rng(seed)
    parents = rng.uniform([0.15 * W, 0.15 * H], [0.75 * W, 0.85 * H], (12, 2))
    xy = parents[rng.integers(0, 12, M)] + rng.normal(0, 50, (M, 2))
    loose = rng.uniform(size=M) < 1 / 3
    xy[loose] = rng.uniform(-20, [W + 20, H + 20], (int(loose.sum()), 2))
    wh = rng.uniform(4, 30, (M, 2))
    rows = np.concatenate([xy - wh / 2, xy + wh / 2, rng.uniform(0.5, 1, (M, 2)), rng.integers(0, C, (M, 1))], 1).astype(np.float32)
    for i in np.flatnonzero(rng.uniform(size=M) < bad):
        k = i % 3
        if k == 0:
            rows[i, i % 4] = np.nan
        elif k == 1:
            rows[i, 6] = (-1, C, 0.5)[i % 3]
        else:
            rows[i, 4] = rng.uniform(0, 0.5)
    return rows


def check_not_idle(M, res, rect, wbd, rbd, cls, r_max):
    """asserted on the RESTATEMENT's output, before a kernel is looked at, for every ragged case with M >= 257: the mask matters.
    res, rect: the outputs with the mask and with an all-IN mask (the rectangle's pairs and centres); wbd, rbd: the mask's and the
    rectangle's distances per row (the rectangle's capped like the mask's, which asks more than the uncapped comparison)"""
    if M < 257:
        return
    pairs, centres, nn, bd, stats = res
    counted = cls >= 0
    assert (wbd[counted] < np.minimum(rbd[counted], r_max)).mean() >= 0.25, "fewer than a quarter of the counted rows are bound by the mask"
    assert (wbd[counted] < 0).mean() >= 0.05, "fewer than 5 % of the counted rows lie in OUT cells"
    assert (centres > 0).all(), centres
    assert (centres[:, -1] < rect[1][:, -1]).all(), (centres, rect[1])
    assert (pairs != rect[0]).any(axis=(0, 1)).all(), "a radius at which the mask changes no pair count"


_cache = {}


def ragged_case(M, border=True):
    """(rows, radii_q, mask, reference outputs) of the ragged case of size M, computed once and shared: treat it as read-only"""
    key = (M, border)
    if key not in _cache:
        rows, mask = ragged_rows(M, 2000 + M), blob_mask(*grid_of(SLIDE_H, SLIDE_W, CELL), seed=7)
        rq = radii_q(RADII_PX)
        res = pair_counts_window(rows, SLIDE_H, SLIDE_W, CLASSES, 0.5, rq, mask, CELL, None, border)
        if border:
            qx, qy, cls = positions(rows, SLIDE_H, SLIDE_W, CLASSES, 0.5)[:3]
            rect = pair_counts_window(rows, SLIDE_H, SLIDE_W, CLASSES, 0.5, rq, np.ones_like(mask), CELL)
            check_not_idle(M, res, rect, window_bd(qx, qy, mask, CELL, SLIDE_H, SLIDE_W, rq[-1]), rect_bd(qx, qy, SLIDE_H, SLIDE_W), cls, int(rq[-1]))
        for a in (rows, rq, mask) + res:
            a.setflags(write=False)
        _cache[key] = rows, rq, mask, res
    return _cache[key]
