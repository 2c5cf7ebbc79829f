"""NumPy restatement of THE BURDEN RULE and THE FIELD RULE of include/amyloid_yolo.h (TEST INFRASTRUCTURE ONLY): float32 for the
centre, integers after it; the field sums as plain loops over cells, the selection as the sequential loop of the rule.

Nothing here comes from the product: the grid is restated too."""
import math

import numpy as np

MAX_CLASSES, MAX_FIELDS = 64, 64
FLAG_NONFINITE, FLAG_CLASS = 1, 2


def grid(H, W, cell):
    return -(-H // cell), -(-W // cell)


def burden_bin(rows, H, W, cell, C, min_conf):
    """-> counts int32 [C, Gy, Gx], stats int32 [C + 3] = counted per class, below, flagged, flag bits; a loop over the rows"""
    rows = np.asarray(rows, np.float32).reshape(-1, 7)
    gy, gx = grid(H, W, cell)
    counts, stats = np.zeros((C, gy, gx), np.int32), np.zeros(C + 3, np.int32)
    half, min_conf = np.float32(0.5), np.float32(min_conf)
    with np.errstate(all="ignore"):
        for x1, y1, x2, y2, conf, _, label in rows:
            cx, cy = (x1 + x2) * half, (y1 + y2) * half              # float32: two operations each
            flags = 0
            if not (np.isfinite(cx) and np.isfinite(cy)):
                flags |= FLAG_NONFINITE
            if not (label >= 0 and label < C and float(label) == int(label)):
                flags |= FLAG_CLASS
            if flags:
                stats[C + 1] += 1
                stats[C + 2] |= flags
                continue
            if not conf >= min_conf:
                stats[C] += 1
                continue
            px = min(int(math.floor(min(max(cx, np.float32(0)), np.float32(W - 1)))), W - 1)
            py = min(int(math.floor(min(max(cy, np.float32(0)), np.float32(H - 1)))), H - 1)
            counts[int(label), py // cell, px // cell] += 1
            stats[int(label)] += 1
    return counts, stats


def field_sums_loops(plane, F):
    """[Gy - F + 1, Gx - F + 1] sums of the F x F blocks (empty if the grid holds no field): a loop over the F x F cells of a field,
    every field at once (cell (dy, dx) of field (fy, fx) is plane[fy + dy, fx + dx])"""
    plane = np.asarray(plane).astype(np.int64)
    gy, gx = plane.shape
    ny, nx = max(gy - F + 1, 0), max(gx - F + 1, 0)
    if ny == 0 or nx == 0:
        return np.zeros((0, 0), np.int64)
    out = np.zeros((ny, nx), np.int64)
    for dy in range(F):
        for dx in range(F):
            out += plane[dy:dy + ny, dx:dx + nx]
    return out


def field_sums_sat(plane, F):
    """the same sums from a summed-area table: a second formulation"""
    gy, gx = plane.shape
    ny, nx = max(gy - F + 1, 0), max(gx - F + 1, 0)
    if ny == 0 or nx == 0:
        return np.zeros((0, 0), np.int64)
    sat = np.zeros((gy + 1, gx + 1), np.int64)
    sat[1:, 1:] = np.cumsum(np.cumsum(plane.astype(np.int64), 0), 1)
    return sat[F:, F:] - sat[:-F, F:] - sat[F:, :-F] + sat[:-F, :-F]


def field_select(counts, tissue, F, need_tissue, K, sums=field_sums_loops, trace=None):
    """-> fields int32 [C, K, 4] = (fy, fx, n, t), n_found int32 [C]: the rule's rounds, one after the other.
    ``trace`` (a dict) collects what the GPU test asserts about its cases before the kernel is looked at: ``ties`` (rounds whose
    maximum two open eligible fields share), ``ineligible`` (rounds in which an open ineligible field reaches the eligible
    maximum) and, via :func:`suppression_acted`, picks that differ from the K largest fields."""
    counts = np.asarray(counts)
    C = counts.shape[0]
    fields, n_found = np.full((C, K, 4), -1, np.int32), np.zeros(C, np.int32)
    t = None if tissue is None else sums(np.asarray(tissue), F)
    for c in range(C):
        n = sums(counts[c], F)
        if n.size == 0:
            continue
        nx = n.shape[1]
        eligible = np.ones(n.shape, bool) if t is None else t >= need_tissue
        picks = []
        for k in range(K):
            open_ = np.ones(n.shape, bool)
            for py, px in picks:                                # |fy - py| < F and |fx - px| < F
                open_[max(py - F + 1, 0):py + F, max(px - F + 1, 0):px + F] = False
            cand = np.where(open_ & eligible, n, -1).ravel()
            best = int(cand.argmax())                           # the first maximum: the lowest linear index
            if cand[best] <= 0:
                break
            if trace is not None:
                trace["ties"] = trace.get("ties", 0) + int((cand == cand[best]).sum() > 1)
                barred = np.where(open_ & ~eligible, n, -1)
                trace["ineligible"] = trace.get("ineligible", 0) + int(barred.max() >= cand[best])
            fy, fx = best // nx, best % nx
            picks.append((fy, fx))
            fields[c, k] = fy, fx, cand[best], 0 if t is None else t[fy, fx]
        n_found[c] = len(picks)
    return fields, n_found


def suppression_acted(counts, tissue, F, need_tissue, fields, n_found, sums=field_sums_loops):
    """number of classes whose picked counts differ from the largest counts of the eligible fields taken without the overlap rule"""
    acted = 0
    t = None if tissue is None else sums(np.asarray(tissue), F)
    for c in range(len(n_found)):
        n = sums(np.asarray(counts)[c], F)
        if n.size == 0 or n_found[c] == 0:
            continue
        pool = np.sort((n if t is None else np.where(t >= need_tissue, n, -1)).ravel())[::-1]
        acted += int(list(pool[:n_found[c]]) != list(fields[c, :n_found[c], 2]))
    return acted


def need_tissue(fraction, F, cell):
    return max(1, math.ceil(fraction * (F * cell) ** 2))


# ---- the cases of the tests ---------------------------------------------------------------------------------------------------------
def random_rows(M, H, W, C, seed, fractional, bad=0.05):
    """M boxes of 8..47 px with centres up to 30 px outside the slide; about `bad` of them flagged (NaN / inf coordinate, class -1, C,
    0.5 or NaN) or below 0.5 (NaN confidence included)"""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(-30, [W + 30, H + 30], (M, 2))
    wh = rng.uniform(8, 47, (M, 2))
    box = np.concatenate([xy - wh / 2, xy + wh / 2], 1)
    if not fractional:
        box = np.round(box)
    rows = np.concatenate([box, rng.uniform(0.5, 1, (M, 2)), rng.integers(0, C, (M, 1))], 1).astype(np.float32)
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


def random_planes(gy, gx, C, seed):
    """counts (rand < 0.15) * randint(1, 4) and tissue randint(0, 64^2 + 1) * (rand < 0.8), as the field test states them"""
    rng = np.random.default_rng(seed)
    counts = ((rng.uniform(size=(C, gy, gx)) < 0.15) * rng.integers(1, 4, (C, gy, gx))).astype(np.int32)
    tissue = (rng.integers(0, 64 * 64 + 1, (gy, gx)) * (rng.uniform(size=(gy, gx)) < 0.8)).astype(np.int32)
    return counts, tissue


FIELD_CASES = [(1, 1, 1, 1), (8, 8, 8, 3), (7, 40, 8, 3), (33, 65, 8, 5), (33, 65, 2, 64), (200, 130, 33, 5)]   # (Gy, Gx, F, K)


def field_case(gy, gx, F, K, C):
    counts, tissue = random_planes(gy, gx, C, 1000 * gy + 10 * gx + F + C)
    if (gy, gx) == (1, 1):
        counts[:] = 1
        tissue[:] = 64 * 64
    return counts, tissue, need_tissue(0.4, F, 64)
