"""THE SEGMENT RULE of include/amyloid_yolo.h restated in NumPy (TEST INFRASTRUCTURE ONLY): load_reference's pixel classes and box
edges, a plain flood fill over a stack for the components, loops over pixels for the sums.  Nothing here comes from the product.
Ownership and residency are modelled as well, so that the rule can be called strip by strip."""
import numpy as np

import load_reference as lr

F32 = np.float32
COLS, MAX_SIDE, MAX_MARGIN = 20, 255, 127
NONFINITE, EMPTY, LARGE, NOT_RESIDENT, INTERNAL = 1, 2, 4, 8, 16
NEIGHBOURS8 = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def windows(rows, H, W, margin):
    """rows [M, >= 4] -> (kind int64 [M]: 0, NONFINITE, EMPTY or LARGE; edges int64 [M, 4] = lo_x, lo_y, hi_x, hi_y; win int64 [M, 4] =
    wx0, wy0, ww, wh, zeros without a window; owner int64 [M])"""
    assert 0 <= margin <= MAX_MARGIN
    finite, e = lr.edges(rows, H, W)
    M = len(e)
    kind, win = np.zeros(M, np.int64), np.zeros((M, 4), np.int64)
    for m in range(M):
        if not finite[m]:
            kind[m] = NONFINITE
        elif e[m, 0] >= e[m, 2] or e[m, 1] >= e[m, 3]:
            kind[m] = EMPTY
        else:
            wx0, wx1 = max(e[m, 0] - margin, 0), min(e[m, 2] + margin, W)
            wy0, wy1 = max(e[m, 1] - margin, 0), min(e[m, 3] + margin, H)
            win[m] = wx0, wy0, wx1 - wx0, wy1 - wy0
            if wx1 - wx0 > MAX_SIDE or wy1 - wy0 > MAX_SIDE:
                kind[m] = LARGE
    return kind, e, win, win[:, 1].copy()


def components(mask):
    """8-connected components of a bool image by a plain flood fill -> int32 labels, 0 for background, components numbered 1, 2, ..
    in the raster order of their first pixels (so that the lowest label holds the lowest raster index)"""
    h, w = mask.shape
    lab = np.zeros((h, w), np.int32)
    n = 0
    for y0, x0 in zip(*np.nonzero(mask)):
        if lab[y0, x0]:
            continue
        n += 1
        lab[y0, x0] = n
        stack = [(int(y0), int(x0))]
        while stack:
            y, x = stack.pop()
            for dy, dx in NEIGHBOURS8:
                v, u = y + dy, x + dx
                if 0 <= v < h and 0 <= u < w and mask[v, u] and not lab[v, u]:
                    lab[v, u] = n
                    stack.append((v, u))
    return lab, n


def window_words(pos, core, q, box, min_area):
    """words 5 .. 19 of a normal row: pos, core bool and q int [wh, ww] of the window, box = (x0, y0, x1, y1) the box proper in window
    coordinates"""
    wh, ww = pos.shape
    out = np.zeros(15, np.int64)
    out[0] = pos.sum()
    lab, n = components(pos)
    inside = np.zeros_like(pos)
    inside[box[1]:box[3], box[0]:box[2]] = True
    areas = np.bincount(lab.ravel(), minlength=n + 1)
    in_box = np.zeros(n + 1, bool)
    in_box[lab[inside & pos]] = True
    cand = in_box & (areas >= min_area)
    cand[0] = False
    out[1] = cand.sum()
    if not out[1]:
        return out
    best = int(np.argmax(np.where(cand, areas, -1)))         # among equals the first label: the lowest raster index
    best_area = int(areas[best])
    comp = lab == best
    ys, xs = np.nonzero(comp)
    padded = np.zeros((wh + 2, ww + 2), bool)                # outside the window counts as "not in the component"
    padded[1:-1, 1:-1] = comp
    perimeter = sum(int((comp & ~padded[1 + dy:1 + dy + wh, 1 + dx:1 + dx + ww]).sum()) for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)))
    sides = (1 if comp[:, 0].any() else 0) | (2 if comp[0].any() else 0) | (4 if comp[:, -1].any() else 0) | (8 if comp[-1].any() else 0)
    out[2:] = [best_area, (comp & core).sum(), q[comp].sum(), perimeter, xs.sum(), ys.sum(), xs.min(), ys.min(), xs.max() + 1, ys.max() + 1,
               sides, (comp & inside).sum(), 0]
    return out


def add_classes(t, q, origin_y, origin_x, H, W, own, j, core_j, margin, min_area, rows, out, flags):
    """one call of the rule on the pixel classes (t, q) of a region's (halved) image at (origin_y, origin_x) of the H x W slide, told
    the owner rows own = (own_y0, own_y1): WRITES the rows of `out` [M, 20] it owns, ORs their statuses into flags[0]"""
    h, w = t.shape
    assert origin_y >= 0 and origin_x >= 0 and origin_y + h <= H and origin_x + w <= W
    assert 0 <= j <= core_j <= 512 and min_area >= 1 and 0 <= own[0] <= own[1] <= H
    pos = t & (q >= j)
    core = pos & (q >= core_j)
    kind, e, win, owner = windows(rows, H, W, margin)
    for m in range(len(e)):
        if not own[0] <= owner[m] < own[1]:
            continue
        out[m] = 0
        out[m, 0], out[m, 1:5] = kind[m], win[m]
        if kind[m] == 0:
            wx0, wy0, ww, wh = win[m]
            if wx0 < origin_x or wx0 + ww > origin_x + w or wy0 < origin_y or wy0 + wh > origin_y + h:
                out[m, 0] = NOT_RESIDENT
            else:
                sl = (slice(wy0 - origin_y, wy0 - origin_y + wh), slice(wx0 - origin_x, wx0 - origin_x + ww))
                box = (e[m, 0] - wx0, e[m, 1] - wy0, e[m, 2] - wx0, e[m, 3] - wy0)
                words = window_words(pos[sl], core[sl], q[sl], box, min_area)
                words[8:12] += (wx0, wy0, wx0, wy0) if words[2] else (0, 0, 0, 0)       # the tight box in slide pixels
                out[m, 5:] = words
        flags[0] |= out[m, 0]


def strip_plan(H, strip):
    """wsi.segment_boxes' strips, restated: [(y0, y1, own_y0, own_y1)]: T = min(strip, H) rows, T - 254 apart; a slide with H < 255 is
    one strip; strip j owns the owner rows [j * step, (j + 1) * step), the last through H"""
    assert strip >= MAX_SIDE
    if H < MAX_SIDE:
        return [(0, H, 0, H)]
    T = min(strip, H)
    step = T - (MAX_SIDE - 1)
    n = max(1, -(-(H - (MAX_SIDE - 1)) // step))
    return [(k * step, min(k * step + T, H), k * step, H if k == n - 1 else (k + 1) * step) for k in range(n)]


def segment(raster, shrink, bg, params, stain, j, core_j, margin, min_area, rows, plan=None):
    """the whole slide -> (out int64 [M, 20], flags int64 [1]).  plan: [(y0, y1, own_y0, own_y1)], the rows [y0, y1) of the (halved)
    slide that a call holds and the owner rows it is told; None is one call that holds and owns everything.  Rows that no call owns
    keep -1 in every word."""
    H, W = raster.shape[0] // shrink, raster.shape[1] // shrink
    out, flags = np.full((len(rows), COLS), -1, np.int64), np.zeros(1, np.int64)
    t, q = lr.classes(raster[:H * shrink], shrink, bg, params, stain)
    for y0, y1, a, b in plan or [(0, H, 0, H)]:
        add_classes(t[y0:y1], q[y0:y1], y0, 0, H, W, (a, b), j, core_j, margin, min_area, rows, out, flags)
    return out, flags


def morphometry(seg, mpp=None, slide_hw=None):
    """plain loops over the rows of seg [M, 20] -> dict of lists"""
    nan = float("nan")
    keys = ["area_px", "core_fraction", "mean_od", "centroid_x", "centroid_y", "perimeter_px", "compactness", "outside_fraction"]
    out = {k: [] for k in keys + ["tight_box", "truncated", "candidates"] + (["area_um2", "equiv_diameter_um"] if mpp is not None else [])}
    for s in np.asarray(seg).tolist():
        ok = s[0] == 0 and s[7] > 0
        area = s[7]
        vals = [float(area), s[8] / area, (s[9] / area + 0.5) / 64.0, s[1] + s[11] / area + 0.5, s[2] + s[12] / area + 0.5, float(s[10]),
                16.0 * area / s[10] ** 2, 1.0 - s[18] / area] if ok else [nan] * 8
        for k, v in zip(keys, vals):
            out[k].append(v)
        out["tight_box"].append([float(v) for v in s[13:17]] if ok else [nan] * 4)
        out["candidates"].append(float(s[6]) if ok else nan)
        sides = s[17]
        if ok and slide_hw is not None:                      # a window side that is a border of the slide truncates nothing
            Hs, Ws = slide_hw
            sides &= ~((1 if s[1] == 0 else 0) | (2 if s[2] == 0 else 0) | (4 if s[1] + s[3] == Ws else 0) | (8 if s[2] + s[4] == Hs else 0))
        out["truncated"].append(bool(ok and sides))
        if mpp is not None:
            out["area_um2"].append(area * mpp ** 2 if ok else nan)
            out["equiv_diameter_um"].append(2.0 * (area * mpp ** 2 / np.pi) ** 0.5 if ok else nan)
    return out


# ---- inputs the CPU and the GPU tests share ----------------------------------------------------------------------------------------
POSITIVE, CORE, NEGATIVE, GLASS = (150, 110, 70), (90, 55, 30), (150, 150, 200), (255, 255, 255)
BG, THRES_BIN, CORE_BIN = 220, 10, 64                        # with H_DAB the four colours give the bins 44, 69, 0 and no tissue


def paint(pos, core=None, glass=None, shrink=1):
    """bool images [h, w] -> a uint8 raster [h * shrink, w * shrink, 3] in the four colours (2x2 blocks of one colour for shrink 2: the
    means are the colours)"""
    r = np.empty(pos.shape + (3,), np.uint8)
    r[:] = NEGATIVE
    r[pos] = POSITIVE
    if core is not None:
        r[pos & core] = CORE
    if glass is not None:
        r[glass & ~pos] = GLASS
    return np.repeat(np.repeat(r, shrink, 0), shrink, 1)


def smooth_field(H, W, seed, radius):
    """white noise through three box filters of side 2 * radius + 1 (edges replicated): blobs of about that size"""
    f = np.random.default_rng(seed).random((H, W))
    for _ in range(3):
        for axis in (0, 1):
            n = f.shape[axis]
            pad = np.concatenate([np.repeat(np.take(f, [0], axis), radius, axis), f, np.repeat(np.take(f, [n - 1], axis), radius, axis)], axis)
            c = np.concatenate([np.zeros_like(np.take(pad, [0], axis)), np.cumsum(pad, axis)], axis)
            f = np.take(c, np.arange(2 * radius + 1, n + 2 * radius + 1), axis) - np.take(c, np.arange(n), axis)
    return f


def blob_raster(H, W, seed, shrink=1, radius=5):
    """a (halved) H x W slide whose positive set has sizeable blobs with cores, speckle between them and some glass; two equal 3x3
    blobs alone on a negative patch in the top-left corner for a tie -> (raster, the row over the two)"""
    f = smooth_field(H, W, seed, radius)
    pos, core, glass = f > np.quantile(f, 0.66), f > np.quantile(f, 0.9), f < np.quantile(f, 0.06)
    pos |= np.random.default_rng(seed + 1).random((H, W)) < 0.004
    pos[:18, :26], glass[:18, :26] = False, False            # the tie row's window at margin 8 sees nothing else
    pos[3:6, 3:6] = pos[3:6, 10:13] = True
    return paint(pos, core, glass, shrink), np.asarray([[1.0, 1.0, 15.0, 8.0, 0.9, 0.9, 0.0]], F32)



def row(x1, y1, x2, y2, conf=0.9, cls=0.0):
    return [x1, y1, x2, y2, conf, 0.9, cls]


def spiral(n):
    """a one-pixel path that winds inwards with one-pixel gaps: ONE component whose path is about n * n / 2 pixels long"""
    m = np.zeros((n, n), bool)
    x = y = d = 0
    m[0, 0] = True
    inside = lambda u, v: 0 <= u < n and 0 <= v < n
    while True:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d]
        moved = False
        while inside(x + dx, y + dy) and not m[y + dy, x + dx] and not (inside(x + 2 * dx, y + 2 * dy) and m[y + 2 * dy, x + 2 * dx]):
            x, y, moved = x + dx, y + dy, True
            m[y, x] = True
        if not moved:
            return m
        d = (d + 1) % 4


def serpentine(n):
    m = np.zeros((n, n), bool)
    m[0::2] = True
    m[1::4, n - 1] = True
    m[3::4, 0] = True
    return m


def comb(n):
    m = np.zeros((n, n), bool)
    m[0], m[:, 0::2] = True, True
    return m


WORST = ("full", "checkerboard", "every other", "spiral", "serpentine", "comb", "diagonal", "two equal blobs", "empty")
WORST_MARGIN = 100


def worst_slide():
    """the worst windows side by side on a 255 x (9 * 255) slide: row k is a box in the middle of pattern k whose window, at margin
    100, is exactly the pattern; one more row has a window of 256 columns: LARGE -> (pos bool, rows fp32)"""
    n = MAX_SIDE
    yy, xx = np.mgrid[0:n, 0:n]
    blobs = np.zeros((n, n), bool)
    blobs[110:120, 102:112] = blobs[125:135, 140:150] = True         # 100 pixels each, both in the box proper: the first wins
    pats = {"full": np.ones((n, n), bool), "checkerboard": (xx + yy) % 2 == 0, "every other": (xx % 2 == 0) & (yy % 2 == 0),
            "spiral": spiral(n), "serpentine": serpentine(n), "comb": comb(n), "diagonal": xx == yy, "two equal blobs": blobs,
            "empty": np.zeros((n, n), bool)}
    pos = np.concatenate([pats[k] for k in WORST], 1)
    rows = [row(k * n + 100.0, 100.0, k * n + 155.0, 155.0) for k in range(len(WORST))] + [row(100.0, 100.0, 156.0, 155.0)]
    return pos, np.asarray(rows, F32)


HAND_MARGIN = 3


def hand_slide():
    """small shapes on a 64 x 96 slide, one per 16 x 16 cell so that no window (margin 3) sees another's -> (pos, core, rows, names)"""
    pos, core = np.zeros((64, 96), bool), np.zeros((64, 96), bool)
    rows, names = [], []
    def case(name, r, pixels, cores=()):
        for x, y in pixels:
            pos[y, x] = True
        for x, y in cores:
            core[y, x] = True
        rows.append(r), names.append(name)
    block = lambda x0, y0, w, h: [(x, y) for y in range(y0, y0 + h) for x in range(x0, x0 + w)]
    case("one pixel", row(20, 4, 23, 7), [(21, 5)])
    case("2x2", row(36, 4, 40, 8), block(37, 5, 2, 2), [(37, 5)])
    case("diagonal pair", row(52, 4, 56, 8), [(53, 5), (54, 6)])
    case("L", row(68, 3, 74, 9), block(69, 4, 1, 4) + block(70, 7, 3, 1))
    case("ring", row(20, 19, 27, 26), [p for p in block(21, 20, 5, 5) if p not in block(22, 21, 3, 3)], [(21, 20), (25, 24)])
    case("tie", row(36, 20, 44, 24), block(37, 21, 2, 2) + block(41, 21, 2, 2))
    case("only in the margin", row(52, 20, 56, 24), block(57, 21, 2, 2))
    case("one pixel in the box", row(68, 20, 72, 24), block(71, 21, 4, 1) + block(72, 22, 3, 1))
    case("two sizes", row(20, 36, 29, 43), block(21, 37, 3, 3) + block(25, 37, 4, 4) + [(28, 42)])
    case("nothing", row(36, 36, 44, 44), [])
    case("top-left corner", row(-5, -5, 6, 6), block(0, 0, 3, 3))
    case("top-right corner", row(90, -9, 102, 5), block(93, 0, 3, 2))
    case("bottom-left corner", row(-1e9, 59, 5, 1e9), block(0, 61, 2, 3))
    case("bottom-right corner", row(91.5, 59.5, 96, 64), block(92, 60, 4, 4), block(94, 62, 2, 2))
    case("not finite", row(float("nan"), 1, 5, 5), [])
    case("inverted", row(30, 40, 20, 50), [])
    return pos, core, np.asarray(rows, F32), names


RANDOM_MARGIN = 8


def random_case(shrink, extra=None):
    """the random test's inputs -> (raster, rows, short): a blob raster of 300 x 260 (halved) pixels; the tie row first, then 260
    random boxes of detection size (some across the rows 100, 101 and 250, where the tests cut), then `extra`; `short`: a region of
    the rows [0, short) lacks rows that some windows need"""
    H, W = 300, 260
    raster, tie = blob_raster(H, W, 40 + shrink, shrink)
    rows = [tie, lr.random_boxes(260, H, W, 7 + shrink, cuts=(100, 101, 250))] + ([] if extra is None else [np.asarray(extra, F32)])
    return raster, np.concatenate(rows), H - 20


def assert_random_counts(out, flags):
    """what the random inputs must show on the reference alone, before anything is compared with it"""
    ok = out[:, 0] == 0
    assert (ok & (out[:, 7] > 0)).sum() >= 100 and (ok & (out[:, 6] >= 2)).sum() >= 20 and (ok & (out[:, 17] != 0)).sum() >= 10
    assert (ok & (out[:, 8] > 0)).sum() >= 20 and (ok & (out[:, 7] > 0) & (out[:, 18] < out[:, 7])).sum() >= 20     # cores; parts outside the box
    assert (ok & (np.maximum(out[:, 3], out[:, 4]) > 96)).sum() >= 10 and (ok & (np.maximum(out[:, 3], out[:, 4]) <= 96)).sum() >= 100
    assert out[0, 5:8].tolist() == [18, 2, 9] and out[0, 13:17].tolist() == [3, 3, 6, 6]      # a tie: two candidates of 9, the first wins
    assert not flags[0] & (NOT_RESIDENT | INTERNAL)
