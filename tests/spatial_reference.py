"""NumPy restatement of THE PAIR RULE of include/amyloid_yolo.h (TEST INFRASTRUCTURE ONLY): float32 for the centre and the multiply by
four, integers after them; the pairs by brute force over ALL pairs (int64, chunks of 512 rows), a second time as a plain Python loop
over every pair for tiny cases, a third time over a cell grid of side R_max for the sizes at which all pairs are too many
(pair_counts_binned), and the host formulas (K, L, g, G) as loops.

Nothing here comes from the product: the conversions of radii and windows are restated too."""
import math

import numpy as np

MAX_CLASSES, MAX_RADII, MAX_RADIUS_Q = 8, 32, 32767
FLAG_NONFINITE, FLAG_CLASS = 1, 2
CHUNK = 512


def radii_q(radii_px):
    return np.array([math.floor(4.0 * float(r)) for r in radii_px], np.int32)


def roi_q(roi_px, H, W):
    if roi_px is None:
        return np.array([0, 0, 4 * W - 1, 4 * H - 1], np.int32)
    x1, y1, x2, y2 = (float(v) for v in roi_px)
    return np.array([max(math.ceil(4 * x1), 0), max(math.ceil(4 * y1), 0), min(math.floor(4 * x2), 4 * W - 1), min(math.floor(4 * y2), 4 * H - 1)],
                    np.int32)


def positions(rows, H, W, C, min_conf):
    """-> qx, qy int64 [M], cls int64 [M] (-1: not counted), below, flagged, flag bits: the rule's steps per row, as a loop"""
    rows = np.asarray(rows, np.float32).reshape(-1, 7)
    M = len(rows)
    qx, qy, cls = np.zeros(M, np.int64), np.zeros(M, np.int64), np.full(M, -1, np.int64)
    below = flagged = bits = 0
    half, four, zero, min_conf = np.float32(0.5), np.float32(4.0), np.float32(0.0), np.float32(min_conf)
    with np.errstate(all="ignore"):
        for i, (x1, y1, x2, y2, conf, _, label) in enumerate(rows):
            cx, cy = (x1 + x2) * half, (y1 + y2) * half              # float32: two operations each
            flags = 0
            if not (np.isfinite(cx) and np.isfinite(cy)):
                flags |= FLAG_NONFINITE
            if not (label >= 0 and label < C and float(label) == int(label)):
                flags |= FLAG_CLASS
            if flags:
                flagged += 1
                bits |= flags
                continue
            if not conf >= min_conf:
                below += 1
                continue
            qx[i] = int(math.floor(min(max(cx * four, zero), np.float32(4 * W - 1))))
            qy[i] = int(math.floor(min(max(cy * four, zero), np.float32(4 * H - 1))))
            cls[i] = int(label)
    return qx, qy, cls, below, flagged, bits


def _head(rows, H, W, C, min_conf, rq, roi, border):
    """what both formulations share: positions, border distances, the largest eligible k, bd and stats"""
    rq = np.asarray(rq, np.int64)
    assert 1 <= len(rq) <= MAX_RADII and rq[0] >= 1 and rq[-1] <= MAX_RADIUS_Q and (np.diff(rq) > 0).all() and 1 <= C <= MAX_CLASSES
    X1, Y1, X2, Y2 = (0, 0, 4 * W - 1, 4 * H - 1) if roi is None else (int(v) for v in roi)
    assert X1 <= X2 and Y1 <= Y2
    qx, qy, cls, below, flagged, bits = positions(rows, H, W, C, min_conf)
    M = len(cls)
    dist = np.minimum(np.minimum(qx - X1, X2 - qx), np.minimum(qy - Y1, Y2 - qy))
    counted = cls >= 0
    eligible = counted[:, None] & (dist[:, None] >= (rq[None, :] if border else 0 * rq[None, :]))      # [M, B]
    bd = np.where(counted & (dist >= 0), dist, -1).astype(np.int32)
    stats = np.zeros(2 * C + 3, np.int32)
    for c in range(C):
        stats[c] = (cls == c).sum()
        stats[C + c] = ((cls == c) & (dist >= 0)).sum()
    stats[2 * C:] = below, flagged, bits
    assert stats[:C].sum() + below + flagged == M
    centres = np.stack([eligible[cls == a].sum(0) for a in range(C)]).astype(np.int32).reshape(C, len(rq))
    return rq, qx, qy, cls, eligible, bd, stats, centres


def pair_counts(rows, H, W, C, min_conf, rq, roi=None, border=True):
    """THE PAIR RULE by brute force -> pairs int64 [C,C,B], centres int32 [C,B], nn int32 [M,C,2], bd int32 [M], stats int32 [2C+3]"""
    rq, qx, qy, cls, eligible, bd, stats, centres = _head(rows, H, W, C, min_conf, rq, roi, border)
    M, B = len(cls), len(rq)
    r2 = rq * rq
    pairs, nn = np.zeros((C, C, B), np.int64), np.full((M, C, 2), -1, np.int32)
    idx = np.flatnonzero(cls >= 0)                                   # ascending: the first minimum below is the lowest row index
    px, py, pc = qx[idx], qy[idx], cls[idx]
    far = np.int64(1) << 62
    onehot = (pc[:, None] == np.arange(C)[None, :]).astype(np.float64)
    for lo in range(0, len(idx), CHUNK):
        me = idx[lo:lo + CHUNK]
        d2 = (qx[me][:, None] - px[None, :]) ** 2 + (qy[me][:, None] - py[None, :]) ** 2           # int64 [chunk, N]
        d2[np.arange(len(me)), lo + np.arange(len(me))] = far                                       # j != i
        for k in range(B):                                                                          # equality counts
            n = ((d2 <= r2[k]).astype(np.float64) @ onehot).astype(np.int64)                        # [chunk, C] partners per class (exact)
            for a in range(C):
                pairs[a, :, k] += n[eligible[me, k] & (cls[me] == a)].sum(0)
        for b in range(C):
            db = np.where(pc[None, :] == b, d2, far)
            j = db.argmin(1)
            best = db[np.arange(len(me)), j]
            hit = best <= r2[-1]
            nn[me[hit], b, 0], nn[me[hit], b, 1] = best[hit], idx[j[hit]]
    return pairs, centres, nn, bd, stats


def pair_counts_binned(rows, H, W, C, min_conf, rq, roi=None, border=True):
    """the same rule over a cell grid of side R_max (quarter pixels), for sizes at which all pairs are too many: a partner within
    R_max of a centre lies in the 3 x 3 cells around the centre's, so a cell's rows are compared with the rows of those nine cells
    only, in int64, exactly as pair_counts compares a chunk with all rows.  tests/test_spatial_cpu.py shows the two equal in every
    output."""
    rq, qx, qy, cls, eligible, bd, stats, centres = _head(rows, H, W, C, min_conf, rq, roi, border)
    M, B = len(cls), len(rq)
    r2, S = rq * rq, int(rq[-1])
    pairs, nn = np.zeros((C, C, B), np.int64), np.full((M, C, 2), -1, np.int32)
    idx = np.flatnonzero(cls >= 0)
    if len(idx) == 0:
        return pairs, centres, nn, bd, stats
    gx, gy = int(qx[idx].max()) // S + 1, int(qy[idx].max()) // S + 1
    cell = (qy[idx] // S) * gx + qx[idx] // S
    order = np.argsort(cell, kind="stable")
    sidx, start = idx[order], np.searchsorted(cell[order], np.arange(gx * gy + 1))
    far = np.int64(1) << 62
    for c in np.unique(cell):
        me = sidx[start[c]:start[c + 1]]
        y, x = divmod(int(c), gx)
        near = [sidx[start[v * gx + max(x - 1, 0)]:start[v * gx + min(x + 1, gx - 1) + 1]] for v in range(max(y - 1, 0), min(y + 1, gy - 1) + 1)]
        nb = np.sort(np.concatenate(near))                           # ascending: the first minimum below is the lowest row index
        d2 = (qx[me][:, None] - qx[nb][None, :]) ** 2 + (qy[me][:, None] - qy[nb][None, :]) ** 2   # int64 [cell, neighbourhood]
        d2[me[:, None] == nb[None, :]] = far                         # j != i
        pc = cls[nb]
        onehot = (pc[:, None] == np.arange(C)[None, :]).astype(np.float64)
        for k in range(B):                                           # equality counts
            n = ((d2 <= r2[k]).astype(np.float64) @ onehot).astype(np.int64)                        # [cell, C] partners per class (exact)
            for a in range(C):
                pairs[a, :, k] += n[eligible[me, k] & (cls[me] == a)].sum(0)
        for b in range(C):
            if not (pc == b).any():
                continue
            db = np.where(pc[None, :] == b, d2, far)
            j = db.argmin(1)
            best = db[np.arange(len(me)), j]
            hit = best <= r2[-1]
            nn[me[hit], b, 0], nn[me[hit], b, 1] = best[hit], nb[j[hit]]
    return pairs, centres, nn, bd, stats


def pair_counts_loop(rows, H, W, C, min_conf, rq, roi=None, border=True):
    """the same, one pair at a time in Python: a second, independent formulation for tiny cases"""
    rq, qx, qy, cls, eligible, bd, stats, centres = _head(rows, H, W, C, min_conf, rq, roi, border)
    M, B = len(cls), len(rq)
    pairs, nn = np.zeros((C, C, B), np.int64), np.full((M, C, 2), -1, np.int32)
    for i in range(M):
        if cls[i] < 0:
            continue
        for j in range(M):
            if j == i or cls[j] < 0:
                continue
            d2 = int(qx[i] - qx[j]) ** 2 + int(qy[i] - qy[j]) ** 2
            for k in range(B):
                if d2 <= int(rq[k]) ** 2 and eligible[i, k]:
                    pairs[cls[i], cls[j], k] += 1
            if d2 <= int(rq[-1]) ** 2 and (nn[i, cls[j], 1] < 0 or d2 < nn[i, cls[j], 0]):          # j ascends: ties keep the lowest
                nn[i, cls[j]] = d2, j
    return pairs, centres, nn, bd, stats


def summaries(pairs, centres, inside, bd, nn, cls, rq, area, mpp=None):
    """the host formulas in float64, entry by entry; NaN wherever a denominator is 0.  cls [M]: the class of every row, -1 = not
    counted"""
    C, B = centres.shape
    r = [int(q) / 4.0 for q in rq]
    nan = float("nan")
    intensity = np.array([float(inside[b]) / area if area > 0 else nan for b in range(C)])
    K, L, LR, g, G = (np.full((C, C, B), nan) for _ in range(5))
    for a in range(C):
        for b in range(C):
            for k in range(B):
                den = float(centres[a, k]) * intensity[b]
                if den > 0:
                    K[a, b, k] = float(pairs[a, b, k]) / den
                    L[a, b, k] = math.sqrt(K[a, b, k] / math.pi)
                    LR[a, b, k] = L[a, b, k] - r[k]
                prev_K, prev_r = (K[a, b, k - 1], r[k - 1]) if k else (0.0, 0.0)
                g[a, b, k] = (K[a, b, k] - prev_K) / (math.pi * (r[k] ** 2 - prev_r ** 2))
                mine = [i for i in range(len(cls)) if cls[i] == a and bd[i] >= rq[k]]
                if mine:
                    G[a, b, k] = sum(1 for i in mine if 0 <= nn[i, b, 0] <= int(rq[k]) ** 2) / len(mine)
    out = {"intensity": intensity, "K": K, "L": L, "L_minus_r": LR, "g": g, "G": G}
    if mpp is not None:
        out["radii_um"], out["K_um2"] = np.array(r) * mpp, K * mpp ** 2
    return out


# ---- the cases of the tests ---------------------------------------------------------------------------------------------------------
SLIDE_H, SLIDE_W, CLASSES = 3072, 4096, 3
RADII_PX = (8, 16, 32, 64, 128, 256)
SIZES = [1, 2, 63, 64, 65, 257, 4097]
STRIP = 600          # px: the left strip holds class 1 only, the right strip class 0 only (every class then has rows without it near)


def clustered_rows(M, seed, H=SLIDE_H, W=SLIDE_W, C=CLASSES, fractional=True, bad=0.05):
    """M boxes with sides 8 .. 60 px: three quarters around 40 parents (offspring sigma 40 px), a quarter uniform over the slide and
    30 px beyond it; classes uniform, except in two strips at the left and right edge that hold one class each (so that every class
    has rows with no partner of it within the largest radius: an `nn` miss); about `bad` of the rows flagged (NaN / inf coordinate,
    class -1, C, 0.5 or NaN) or below 0.5 (NaN confidence included), as burden_reference.random_rows makes them"""
    rng = np.random.default_rng(seed)
    parents = rng.uniform([STRIP, 0], [W - STRIP, H], (40, 2))
    xy = parents[rng.integers(0, 40, M)] + rng.normal(0, 40, (M, 2))
    loose = rng.uniform(size=M) < 0.25
    xy[loose] = rng.uniform(-30, [W + 30, H + 30], (int(loose.sum()), 2))
    wh = rng.uniform(8, 60, (M, 2))
    box = np.concatenate([xy - wh / 2, xy + wh / 2], 1)
    if not fractional:
        box = np.round(box)
    cls = rng.integers(0, C, M)
    if C >= 2:
        cls[xy[:, 0] < STRIP] = 1
        cls[xy[:, 0] > W - STRIP] = 0
    rows = np.concatenate([box, rng.uniform(0.5, 1, (M, 2)), cls[:, None]], 1).astype(np.float32)
    kind = rng.integers(0, 8, M)
    for i in np.flatnonzero(rng.uniform(size=M) < bad):
        k = kind[i]
        if k == 0:
            rows[i, rng.integers(0, 4)] = np.nan
        elif k == 1:
            rows[i, rng.integers(0, 4)] = np.inf * (1 if i % 2 else -1)
        elif k == 2:
            rows[i, 6] = (-1, C, 0.5, np.nan)[i % 4]
        elif k == 3:
            rows[i, 4] = np.nan
        else:
            rows[i, 4] = rng.uniform(0, 0.5)
    return rows


def check_not_idle(M, res, border=True):
    """asserted on the RESTATEMENT's output, before a kernel is looked at, for every random case with M >= 257: the pair table is
    filled, the border rule both kept and dropped centres, every class has a nearest-neighbour hit and a miss, and some rows are
    flagged and some below"""
    pairs, centres, nn, bd, stats = res
    C = centres.shape[0]
    if M < 257:
        return
    assert (pairs == 0).mean() <= 0.10, f"{(pairs == 0).sum()} of {pairs.size} pair entries are 0"
    if border:
        assert (centres[:, 0] > centres[:, -1]).all() and (centres[:, -1] > 0).all(), centres
    counted = (nn[:, :, 1] >= 0).any(1) | (bd >= 0)
    for b in range(C):
        assert (nn[:, b, 1] >= 0).any(), f"class {b}: no nn hit"
        assert (nn[counted, b, 1] < 0).any(), f"class {b}: no nn miss"
    assert stats[2 * C] > 0 and stats[2 * C + 1] > 0, stats


_cache = {}


def clustered_case(M, border=True):
    """(rows, radii_q, reference outputs) of the clustered case of size M, computed once and shared: treat it as read-only"""
    key = (M, border)
    if key not in _cache:
        rows = clustered_rows(M, 1000 + M)
        rq = radii_q(RADII_PX)
        res = pair_counts(rows, SLIDE_H, SLIDE_W, CLASSES, 0.5, rq, None, border)
        check_not_idle(M, res, border)
        for a in (rows, rq) + res:
            a.setflags(write=False)
        _cache[key] = rows, rq, res
    return _cache[key]


def lattice_rows(n, step, C=2, side=6.0, x0=40.0, y0=40.0):
    """n x n boxes of `side` px whose centres stand on an integer lattice `step` px apart from (x0, y0); classes in a checkerboard"""
    out = []
    for iy in range(n):
        for ix in range(n):
            cx, cy = x0 + ix * step, y0 + iy * step
            out.append([cx - side / 2, cy - side / 2, cx + side / 2, cy + side / 2, 0.9, 1.0, (ix + iy) % C])
    return np.array(out, np.float32)


def points(xy_px, cls=0, side=4.0):
    """rows whose centres are the given (x, y) in pixels (multiples of 1/8 px so that the centre is exact), boxes of `side` px"""
    xy = np.asarray(xy_px, np.float64).reshape(-1, 2)
    c = np.broadcast_to(np.asarray(cls, np.float64), (len(xy),))
    h = side / 2
    return np.stack([xy[:, 0] - h, xy[:, 1] - h, xy[:, 0] + h, xy[:, 1] + h, np.full(len(xy), 0.9), np.ones(len(xy)), c], 1).astype(np.float32)
