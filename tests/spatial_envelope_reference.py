"""NumPy restatement of THE RELABEL RULE of include/amyloid_yolo_spatial_sim.h (TEST INFRASTRUCTURE ONLY): the keys twice (uint64
arrays, Python integers), the label table, the counts of every simulation from ONE brute-force enumeration of all ordered pairs (int64)
with a bincount per simulation -- and, for tiny cases, a second time by the rule's definition: spatial_reference.pair_counts on rows
whose class column is replaced by the table's column -- and the envelope and p_mad formulas as plain loops.

Nothing here comes from the product."""
import math

import numpy as np

import spatial_reference as sr
import spatial_window_reference as swr

MAX_SIMS, FLAG_LABEL = 1024, 4
K_SIM, K_ROW, K_MIX1, K_MIX2 = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
MASK = (1 << 64) - 1


def key_int(seed, s, t):
    """the key of (seed, s, t) in Python integers"""
    z = (seed + s * K_SIM + t * K_ROW) & MASK
    z = ((z ^ (z >> 30)) * K_MIX1) & MASK
    z = ((z ^ (z >> 27)) * K_MIX2) & MASK
    return z ^ (z >> 31)


def keys(seed, s, n):
    """the keys of t = 0 .. n-1 as a uint64 array (array arithmetic wraps modulo 2**64)"""
    u = np.uint64
    z = np.full(n, (seed + s * K_SIM) & MASK, np.uint64) + np.arange(n, dtype=np.uint64) * u(K_ROW)
    z = (z ^ (z >> u(30))) * u(K_MIX1)
    z = (z ^ (z >> u(27))) * u(K_MIX2)
    return z ^ (z >> u(31))


def table(cls, C, n_sim, seed):
    """cls int [M] (-1: not counted) -> uint8 [M, n_sim + 1]: column 0 the observed classes, column s the classes dealt out by the
    rank of the keys; 255 for rows that are not counted"""
    cls = np.asarray(cls, np.int64)
    idx = np.flatnonzero((cls >= 0) & (cls < C))
    N = len(idx)
    out = np.full((len(cls), n_sim + 1), 255, np.uint8)
    out[idx, 0] = cls[idx]
    cum = np.concatenate([[0], np.cumsum([(cls[idx] == c).sum() for c in range(C)])])
    for s in range(1, n_sim + 1):
        order = np.argsort(keys(seed, s, N), kind="stable")
        rank = np.empty(N, np.int64)
        rank[order] = np.arange(N)
        out[idx, s] = np.searchsorted(cum, rank, side="right") - 1       # the c with cum_c <= rank < cum_{c+1}
    return out


def _geometry(rows, H, W, C, min_conf, rq, roi, border, mask, cell):
    """positions, observed classes, the largest eligible k of every row (-1: none), bd and the observed stats"""
    if mask is None:
        rq, qx, qy, cls, eligible, bd, stats, _ = sr._head(rows, H, W, C, min_conf, rq, roi, border)
    else:
        rq = np.asarray(rq, np.int64)
        qx, qy, cls, below, flagged, bits = sr.positions(rows, H, W, C, min_conf)
        counted = cls >= 0
        dist = np.minimum(swr.rect_bd(qx, qy, H, W, roi), swr.window_bd(qx, qy, mask, cell, H, W, rq[-1]))
        eligible = counted[:, None] & (dist[:, None] >= (rq[None, :] if border else 0 * rq[None, :]))
        bd = np.where(counted & (dist >= 0), dist, -1).astype(np.int32)
        stats = np.zeros(2 * C + 3, np.int32)
        for c in range(C):
            stats[c], stats[C + c] = (cls == c).sum(), ((cls == c) & (dist >= 0)).sum()
        stats[2 * C:] = below, flagged, bits
    assert (np.diff(eligible.astype(np.int64), axis=1) <= 0).all()      # the eligible k are a prefix
    return rq, qx, qy, cls, eligible.sum(1) - 1, bd, stats


def all_pairs(qx, qy, cls, rq):
    """every ordered pair (i, j), i != j, of counted rows within the largest radius: (i, j, first bin), by brute force (int64)"""
    idx = np.flatnonzero(cls >= 0)
    r2 = np.asarray(rq, np.int64) ** 2
    I, J, KF = [], [], []
    for lo in range(0, len(idx), sr.CHUNK):
        me = idx[lo:lo + sr.CHUNK]
        d2 = (qx[me][:, None] - qx[idx][None, :]) ** 2 + (qy[me][:, None] - qy[idx][None, :]) ** 2
        d2[np.arange(len(me)), lo + np.arange(len(me))] = np.int64(1) << 62
        a, b = np.nonzero(d2 <= r2[-1])
        I.append(me[a]), J.append(idx[b]), KF.append(np.searchsorted(r2, d2[a, b], side="left"))      # the radii with R_k^2 < d2
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.int64)
    return cat(I), cat(J), cat(KF)


def sim_counts(rows, H, W, C, min_conf, rq, tab, roi=None, border=True, mask=None, cell=None):
    """THE RELABEL RULE's counts -> sim_pairs int64 [S,C,C,B], sim_centres int32 [S,C,B], sim_inside int32 [S,C], bd int32 [M],
    stats int32 [2C+3] (observed classes; FLAG_LABEL where a counted row has a table value >= C)"""
    rq, qx, qy, cls, kmax, bd, stats = _geometry(rows, H, W, C, min_conf, rq, roi, border, mask, cell)
    tab = np.asarray(tab, np.uint8)
    assert tab.ndim == 2 and len(tab) == len(cls)
    S, B = tab.shape[1], len(rq)
    I, J, KF = all_pairs(qx, qy, cls, rq)
    keep = KF <= kmax[I]                                                # the centre is eligible at the pair's first bin
    I, J, KF = I[keep], J[keep], KF[keep]
    counted = np.flatnonzero(cls >= 0)
    sim_pairs, sim_centres, sim_inside = np.zeros((S, C, C, B), np.int64), np.zeros((S, C, B), np.int32), np.zeros((S, C), np.int32)
    stats = stats.copy()
    for s in range(S):
        lab = tab[:, s].astype(np.int64)
        if (lab[counted] >= C).any():
            stats[2 * C + 2] |= FLAG_LABEL
        ok = (lab[I] < C) & (lab[J] < C)
        cell_ab = (lab[I][ok] * C + lab[J][ok]) * (B + 1)
        up = np.bincount(cell_ab + KF[ok], minlength=C * C * (B + 1))             # +1 at the first bin
        down = np.bincount(cell_ab + kmax[I][ok] + 1, minlength=C * C * (B + 1))  # -1 behind the centre's last
        sim_pairs[s] = np.cumsum((up - down).reshape(C, C, B + 1), axis=2)[:, :, :B]
        for a in range(C):
            mine = counted[lab[counted] == a]
            sim_centres[s, a] = [(kmax[mine] >= k).sum() for k in range(B)]
            sim_inside[s, a] = (bd[mine] >= 0).sum()
    return sim_pairs, sim_centres, sim_inside, bd, stats


def sim_counts_by_definition(rows, H, W, C, min_conf, rq, tab, roi=None, border=True, mask=None, cell=None):
    """the rule's definition, for tiny cases: per simulation the plain rule on rows whose class column is the table's column (a value
    >= C makes the row flagged there: no centre, no partner, not inside)"""
    rows = np.asarray(rows, np.float32).reshape(-1, 7)
    cls = sr.positions(rows, H, W, C, min_conf)[2]
    tab = np.asarray(tab, np.uint8)
    assert tab.ndim == 2 and len(tab) == len(rows)
    out = []
    for s in range(tab.shape[1]):
        r = rows.copy()
        r[cls >= 0, 6] = tab[cls >= 0, s]
        res = sr.pair_counts(r, H, W, C, min_conf, rq, roi, border) if mask is None else swr.pair_counts_window(r, H, W, C, min_conf, rq, mask, cell, roi, border)
        out.append((res[0], res[1], res[4][C:2 * C]))
    return tuple(np.stack([o[k] for o in out]) for k in range(3))


def envelope_loops(sim_pairs, sim_centres, sim_inside, rq, area, rank):
    """K, L - r, the pointwise band, the means, `outside`, T and p_mad, entry by entry in float64"""
    S1, C, _, B = sim_pairs.shape
    n = S1 - 1
    nan = float("nan")
    r = [int(q) / 4.0 for q in rq]
    K, LR = np.full((S1, C, C, B), nan), np.full((S1, C, C, B), nan)
    for s in range(S1):
        for a in range(C):
            for b in range(C):
                intensity = float(sim_inside[s, b]) / area if area > 0 else nan
                for k in range(B):
                    den = float(sim_centres[s, a, k]) * intensity
                    if den > 0:
                        K[s, a, b, k] = float(sim_pairs[s, a, b, k]) / den
                        LR[s, a, b, k] = math.sqrt(K[s, a, b, k] / math.pi) - r[k]
    out = {name: np.full((C, C, B), nan) for name in ("K_lo", "K_hi", "L_lo", "L_hi", "K_mean", "L_mean")}
    out.update(K_sim=K, L_minus_r_sim=LR, outside=np.zeros((C, C, B), bool), T=np.full((S1, C, C), nan), p_mad=np.full((C, C), nan))
    for a in range(C):
        for b in range(C):
            usable = []
            for k in range(B):
                for name, v in (("K", K), ("L", LR)):
                    sims = [float(v[s, a, b, k]) for s in range(1, S1)]
                    out[name + "_mean"][a, b, k] = sum(sims) / n
                    if not any(math.isnan(x) for x in sims):
                        out[name + "_lo"][a, b, k], out[name + "_hi"][a, b, k] = sorted(sims)[rank - 1], sorted(sims)[n - rank]
                obs = LR[0, a, b, k]
                out["outside"][a, b, k] = bool(obs > out["L_hi"][a, b, k] or obs < out["L_lo"][a, b, k])
                if all(math.isfinite(LR[s, a, b, k]) for s in range(S1)):
                    usable.append(k)
            if usable:
                bar = {}
                for k in usable:
                    acc = 0.0
                    for s in range(S1):
                        acc += float(LR[s, a, b, k])
                    bar[k] = acc / S1
                for s in range(S1):
                    out["T"][s, a, b] = max(abs(float(LR[s, a, b, k]) - bar[k]) for k in usable)
                out["p_mad"][a, b] = (1 + sum(1 for s in range(1, S1) if out["T"][s, a, b] >= out["T"][0, a, b])) / S1
    return out


def envelope(rows, H, W, C, radii_px, n_sim, seed, rank=1, min_conf=0.0):
    """the whole reference on the slide's rectangle: table, counts, formulas (area = H * W)"""
    rq = sr.radii_q(radii_px)
    cls = sr.positions(rows, H, W, C, min_conf)[2]
    sp, sc, si, _, _ = sim_counts(rows, H, W, C, min_conf, rq, table(cls, C, n_sim, seed))
    return envelope_loops(sp, sc, si, rq, float(H * W), rank)


# ---- the cases of the tests ---------------------------------------------------------------------------------------------------------
SIM_SIZES = [1, 63, 64, 65, 130]           # both sides of a 64-lane chunk
ROW_SIZES = [0, 1, 2, 257, 4097]
_cache = {}


def clustered_sims(M):
    """(rows, radii_q, table [M, 131], counts of all 131 patterns) on spatial_reference.clustered_rows, computed once per M and shared
    (read-only).  The first S columns are a case of S patterns: a column's counts do not depend on the others."""
    if M not in _cache:
        rows, rq = sr.clustered_rows(M, 1000 + M), sr.radii_q(sr.RADII_PX)
        cls = sr.positions(rows, sr.SLIDE_H, sr.SLIDE_W, sr.CLASSES, 0.5)[2]
        tab = table(cls, sr.CLASSES, max(SIM_SIZES), 1234 + M)
        res = sim_counts(rows, sr.SLIDE_H, sr.SLIDE_W, sr.CLASSES, 0.5, rq, tab)
        if M >= 257:       # the inputs must not let a test pass idly
            sr.check_not_idle(M, sr.pair_counts(rows, sr.SLIDE_H, sr.SLIDE_W, sr.CLASSES, 0.5, rq))
            assert ((res[0][1:] != res[0][0]).any(axis=(1, 2, 3))).mean() >= 0.5, "fewer than half the simulations differ from the observed pairs"
            kmax = _geometry(rows, sr.SLIDE_H, sr.SLIDE_W, sr.CLASSES, 0.5, rq, None, True, None, None)[4][cls >= 0]
            assert ((kmax >= 0) & (kmax < len(rq) - 1)).any() and (kmax < 0).any(), "no centre with a limit below the last radius, or none eligible nowhere"
        for a in (rows, rq, tab) + res:
            a.setflags(write=False)
        _cache[M] = rows, rq, tab, res
    return _cache[M]


def first(res, S):
    """the first S patterns of a case's counts"""
    return res[0][:S], res[1][:S], res[2][:S], res[3], res[4]


def square_points(xy, cls, side=6.0):
    """rows of `side`-px square boxes centred at xy"""
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    h = side / 2
    return np.stack([xy[:, 0] - h, xy[:, 1] - h, xy[:, 0] + h, xy[:, 1] + h, np.full(len(xy), 0.9), np.ones(len(xy)),
                     np.asarray(cls, np.float64)], 1).astype(np.float32)


def attraction_rows():
    """60 class-0 points uniform in [40, 984]^2, two class-1 points within +-10 px of each, and 60 more class-1 points uniform"""
    rng = np.random.default_rng(1)
    p0 = rng.uniform(40, 984, (60, 2))
    near = np.repeat(p0, 2, 0) + rng.uniform(-10, 10, (120, 2))
    loose = rng.uniform(40, 984, (60, 2))
    return square_points(np.concatenate([p0, near, loose]), [0] * 60 + [1] * 180)


def random_label_rows():
    """240 uniform points with labels drawn independently"""
    rng = np.random.default_rng(1)
    return square_points(rng.uniform(40, 984, (240, 2)), rng.integers(0, 2, 240))
