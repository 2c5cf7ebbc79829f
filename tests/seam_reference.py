"""CPU restatement of the slide-level seam-merge rule (TEST INFRASTRUCTURE ONLY -- never imported by the product), and the
generators of the inputs the seam tests share.

The rule (include/amyloid_yolo.h, section "slide-level seam merge"): rows [M,7] fp32 (x1, y1, x2, y2, conf, cls_conf, cls_pred) and
tile_id [M].  score = conf * cls_conf in fp32; i ranks before j iff score_i > score_j, or equal and i < j;
ov(i, j) = inter / min(area_i, area_j) in fp32 with the +1 pixel convention; walking the rows in rank order, row i is dropped iff
a row that ranks before it AND WAS KEPT has the same cls_pred, a different tile_id and ov > seam_thres.

Every operation is one NumPy float32 operation (IEEE, no contraction), in the order the rule states them."""
import numpy as np

F32 = np.float32
ONE = F32(1)


def scores(rows):
    rows = np.asarray(rows, F32).reshape(-1, 7)
    return rows[:, 4] * rows[:, 5]


def rank_order(rows):
    """indices in rank order: descending score, ties by ascending index (a stable sort of the negated score)"""
    return np.argsort(-scores(rows), kind="stable")


def ov(box, boxes):
    """ov of one box [4] against boxes [n,4] -> [n] float32"""
    box, boxes = np.asarray(box, F32), np.asarray(boxes, F32).reshape(-1, 4)
    iw = np.minimum(box[2], boxes[:, 2]) - np.maximum(box[0], boxes[:, 0]) + ONE
    ih = np.minimum(box[3], boxes[:, 3]) - np.maximum(box[1], boxes[:, 1]) + ONE
    inter = np.maximum(iw, F32(0)) * np.maximum(ih, F32(0))
    area = (box[2] - box[0] + ONE) * (box[3] - box[1] + ONE)
    areas = (boxes[:, 2] - boxes[:, 0] + ONE) * (boxes[:, 3] - boxes[:, 1] + ONE)
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter / np.minimum(area, areas)


def seam_merge(rows, tile_id, seam_thres=0.5):
    """The plain restatement: every row against all rows kept so far.  -> keep [M] bool"""
    rows = np.asarray(rows, F32).reshape(-1, 7)
    tile_id = np.asarray(tile_id).reshape(-1)
    M = rows.shape[0]
    keep = np.zeros(M, bool)
    thres = F32(seam_thres)
    kept = np.empty(M, np.int64)
    n = 0
    for i in rank_order(rows):
        k = kept[:n]
        cand = k[(rows[k, 6] == rows[i, 6]) & (tile_id[k] != tile_id[i])]
        if cand.size == 0 or not (ov(rows[i, :4], rows[cand, :4]) > thres).any():
            keep[i] = True
            kept[n] = i
            n += 1
    return keep


def seam_merge_binned(rows, tile_id, seam_thres=0.5):
    """The same rule with the kept rows held per grid cell (cell side = the largest box side + 1, so that two boxes that share a
    pixel have their centres in neighbouring cells): a row is tested against the kept rows of the 3x3 cells around its own.
    For inputs too large for :func:`seam_merge`; shown equal to it by the tests before it is used as a yardstick."""
    rows = np.asarray(rows, F32).reshape(-1, 7)
    tile_id = np.asarray(tile_id).reshape(-1)
    M = rows.shape[0]
    keep = np.zeros(M, bool)
    if M == 0:
        return keep
    r64 = rows.astype(np.float64)
    side = np.maximum(r64[:, 2] - r64[:, 0], r64[:, 3] - r64[:, 1]) + 1.0
    c = float(side.max()) + 1.0
    cx = np.floor((r64[:, 0] + r64[:, 2]) * 0.5 / c).astype(np.int64)
    cy = np.floor((r64[:, 1] + r64[:, 3]) * 0.5 / c).astype(np.int64)
    cells = {}
    thres = F32(seam_thres)
    for i in rank_order(rows):
        near = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near += cells.get((cy[i] + dy, cx[i] + dx), ())
        dropped = False
        if near:
            k = np.asarray(near)
            cand = k[(rows[k, 6] == rows[i, 6]) & (tile_id[k] != tile_id[i])]
            dropped = cand.size > 0 and bool((ov(rows[i, :4], rows[cand, :4]) > thres).any())
        if not dropped:
            keep[i] = True
            cells.setdefault((cy[i], cx[i]), []).append(i)
    return keep


def kept_behind_dropped(rows, tile_id, keep, seam_thres=0.5):
    """number of KEPT rows that have a stronger partner (earlier rank, same class, other tile, ov > thres) -- necessarily a dropped
    one: the rows a non-greedy 'drop whatever a stronger row overlaps' rule would lose.  O(M * neighbours) through the same cells."""
    rows = np.asarray(rows, F32).reshape(-1, 7)
    tile_id = np.asarray(tile_id).reshape(-1)
    order = rank_order(rows)
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    r64 = rows.astype(np.float64)
    c = float((np.maximum(r64[:, 2] - r64[:, 0], r64[:, 3] - r64[:, 1]) + 1.0).max()) + 1.0
    cx = np.floor((r64[:, 0] + r64[:, 2]) * 0.5 / c).astype(np.int64)
    cy = np.floor((r64[:, 1] + r64[:, 3]) * 0.5 / c).astype(np.int64)
    cells = {}
    for i in range(len(rows)):
        cells.setdefault((cy[i], cx[i]), []).append(i)
    n = 0
    thres = F32(seam_thres)
    for i in np.flatnonzero(keep):
        near = []
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                near += cells.get((cy[i] + dy, cx[i] + dx), ())
        k = np.asarray(near)
        cand = k[(rank[k] < rank[i]) & (rows[k, 6] == rows[i, 6]) & (tile_id[k] != tile_id[i])]
        if cand.size and (ov(rows[i, :4], rows[cand, :4]) > thres).any():
            n += 1
    return n


def score_ties(rows):
    """number of rows that share their score with another row"""
    _, inv, cnt = np.unique(scores(rows), return_inverse=True, return_counts=True)
    return int((cnt[inv] > 1).sum())


def row(x1, y1, x2, y2, conf, cls_conf=1.0, cls=0.0):
    return [x1, y1, x2, y2, conf, cls_conf, cls]


def hand_cases():
    """name -> (rows, tile_id, seam_thres, expected keep): the cases that pin the restatement itself"""
    A = row(100, 100, 149, 149, 0.9)
    return {
        # one object seen by two tiles: the weaker sighting goes
        "two_sightings": ([A, row(102, 101, 151, 150, 0.8)], [0, 1], 0.5, [True, False]),
        # the same two boxes reported by ONE tile: the per-tile NMS has already dealt with them
        "same_tile": ([A, row(102, 101, 151, 150, 0.8)], [3, 3], 0.5, [True, True]),
        "different_class": ([A, row(102, 101, 151, 150, 0.8, cls=1.0)], [0, 1], 0.5, [True, True]),
        # chain A > B > C: ov(A,B) = ov(B,C) = 30/50 above, ov(A,C) = 10/50 below the threshold -> B dropped, C kept
        "chain": ([row(0, 0, 49, 49, 0.9), row(20, 0, 69, 49, 0.8), row(40, 0, 89, 49, 0.7)], [0, 1, 0], 0.5, [True, False, True]),
        # equal scores: the lower index wins
        "equal_scores": ([row(102, 101, 151, 150, 0.75), row(100, 100, 149, 149, 0.75)], [1, 0], 0.5, [True, False]),
        # a box cut in half by a tile edge against the whole one: IoU = 0.5 (not above 0.5), ov = 1 -> dropped
        "half_cut": ([row(0, 0, 99, 99, 0.9), row(50, 0, 99, 99, 0.6)], [0, 1], 0.5, [True, False]),
    }


def corner_case():
    """one plaque at a grid corner, seen by four tiles (whole by one, clipped by three) + an unrelated box"""
    rows = [row(170, 170, 209, 209, 0.875, 0.5), row(170, 170, 191, 209, 0.75, 0.5), row(170, 170, 209, 191, 0.625, 0.5),
            row(170, 170, 191, 191, 0.5, 0.5), row(20, 30, 60, 70, 0.25, 0.5)]
    return np.asarray(rows, F32), np.asarray([3, 0, 2, 1, 0], np.int32)


def staircase(n=320):
    """chain of n boxes alternating between two tiles, descending scores, each overlapping only its two neighbours
    (50-px boxes 20 px apart: ov = 30/50 with the neighbour, 10/50 with the one after): kept, dropped, kept, ..."""
    rows = [row(20 * k, 7 * k, 20 * k + 49, 7 * k + 49, (4 * n - k) / (4.0 * n), 1.0) for k in range(n)]
    # the vertical shift of 7 px lowers ov to 30*43/2500 = 0.516 (neighbour) and 10*36/2500 = 0.144 (next but one)
    return np.asarray(rows, F32), (np.arange(n) % 2).astype(np.int32)


def far_row(n_obj=150, seed=4):
    """a small slide + one object 10^6 px away seen by two tiles (the last two rows, the stronger first): the extent of the centres
    is far more than the cell cap allows at the histogram's side, so the side is doubled until the grid fits"""
    rows, tile_id = synthetic_slide(n_obj, 2, 2, seed=seed)
    far = [row(1000000, 1000000, 1000039, 1000039, 0.875, 1.0), row(1000002, 1000001, 1000039, 1000041, 0.75, 1.0)]
    return np.concatenate([rows, np.asarray(far, F32)]), np.concatenate([tile_id, np.asarray([100, 101], np.int32)])


def one_cell(n=72):
    """concentric boxes of several sizes (every centre is (500.5, 300.5): the extent is 0, the grid 1 x 1), two classes, tile ids
    alternating; ov of two concentric boxes is 1"""
    half = (3, 5, 9, 14, 22)
    rows = []
    for i in range(n):
        a, b = half[i % 5], half[(i // 5) % 5]
        rows.append(row(500 - a, 300 - b, 501 + a, 301 + b, (8 + (5 * i) % 8) / 16.0, (8 + (3 * i) % 9) / 16.0, (i // 2) % 2))
    return np.asarray(rows, F32), (np.arange(n) % 2).astype(np.int32)


def borders():
    """20 pairs of sightings (rows 2k and 2k + 1, tiles 0 and 1) 96 px apart; the centres of a pair lie on a multiple of 32 px from
    the smallest centre (row 0's, the grid origin) or half a pixel to either side of it, on each axis: where the cell of a centre
    flips.  Sides 17 .. 31 px, so that the chosen cell side is 32."""
    inner = [(-0.5, 0.0), (-0.5, 0.5), (0.0, 0.5), (0.0, -0.5), (0.5, -0.5), (0.0, 0.0)]   # offsets of the two centres from the multiple
    edge = [(0.0, 0.5), (0.5, 0.0), (0.0, 0.0)]                                             # nothing left of (above) the origin
    rows = []
    for k in range(20):
        mx, my = 3 * (k % 5), 3 * (k // 5)
        dx = edge[k % 3] if mx == 0 else inner[k % 6]
        dy = edge[(k // 5) % 3] if my == 0 else inner[(k + k // 5) % 6]
        for s in (0, 1):
            box = []
            for origin, m, d, w in ((1000, mx, dx[s], 17 + (3 * k + 7 * s) % 15), (2000, my, dy[s], 17 + (5 * k + 4 * s) % 15)):
                c2 = int(2 * (origin + 32 * m + d))      # twice the centre: integer corners need a side of the other parity
                if (c2 + w) % 2 == 0:
                    w += 1 if w < 31 else -1
                box.append(((c2 - (w - 1)) // 2, (c2 + (w - 1)) // 2))
            conf = (15 - s) / 16.0 if k % 2 == 0 else (14 + s) / 16.0     # the stronger sighting first, or second
            rows.append(row(box[0][0], box[1][0], box[0][1], box[1][1], conf, 1.0, k % 2))
    return np.asarray(rows, F32), (np.arange(40) % 2).astype(np.int32)


def every_row_oversize():
    """twelve rows a few hundred px wide: too few for the histogram rule to size the cells by, so all of them are oversize"""
    rows = []
    for o, (x, y, w, h) in enumerate([(0, 0, 300, 400), (200, 100, 350, 350), (1000, 50, 250, 300), (1020, 400, 240, 280)]):
        rows.append(row(x, y, x + w - 1, y + h - 1, (15 - o) / 16.0, 1.0, o % 2))                     # whole
        rows.append(row(x + w // 2, y + 2, x + w, y + h - 2, (11 - o) / 16.0, 0.75, o % 2))           # the right half, by the next tile
        rows.append(row(x + 1, y + h // 3, x + w - 2, y + h + 1, (9 + o) / 16.0, 0.5, o % 2))         # the lower two thirds, by the tile below
    return np.asarray(rows, F32), np.asarray([t for o in range(4) for t in (o, o + 1, o + 4)], np.int32)


def geometry_cases():
    """name -> (rows, tile_id): extents and box sizes at which the centre grid takes another path"""
    return {"far_row": far_row(), "one_cell": one_cell(), "borders": borders(), "every_row_oversize": every_row_oversize()}


def synthetic_slide(n_obj, grid_y, grid_x, tile=192, overlap=48, seed=0, big=0):
    """Objects on a slide covered by a grid of overlapping tiles; every tile reports the clipped view of each object it sees (at
    least 4 px of it on either axis), its corners jittered by up to 2 px.  Integer pixel coordinates, conf (below 1) a multiple of 1/16 and
    cls_conf a multiple of 1/16: the score (a multiple of 1/256), inter and the areas are exact in fp32, so ov is one correctly
    rounded division on both sides and no case sits on the threshold by rounding.  Rows in tile order.  ``big`` appends that
    many boxes as large as a tile.  -> rows [M,7] float32, tile_id [M] int32"""
    rng = np.random.Generator(np.random.PCG64(seed))
    step = tile - overlap
    H, W = (grid_y - 1) * step + tile, (grid_x - 1) * step + tile
    side = rng.integers(8, 48, n_obj)
    x1 = rng.integers(0, W - side)
    y1 = rng.integers(0, H - side)
    x2, y2 = x1 + side - 1, y1 + side - 1
    cls = rng.integers(0, 2, n_obj)
    out_rows, out_tile = [], []
    # tiles that see object o: ty with ty*step <= y2 - 3 and ty*step + tile - 1 >= y1 + 3
    for o in range(n_obj):
        ty_lo, ty_hi = max(0, -(-(y1[o] + 3 - tile + 1) // step)), min(grid_y - 1, (y2[o] - 3) // step)
        tx_lo, tx_hi = max(0, -(-(x1[o] + 3 - tile + 1) // step)), min(grid_x - 1, (x2[o] - 3) // step)
        for ty in range(ty_lo, ty_hi + 1):
            for tx in range(tx_lo, tx_hi + 1):
                oy, ox = ty * step, tx * step
                j = rng.integers(-2, 3, 4)
                bx1, by1 = max(x1[o], ox) + j[0], max(y1[o], oy) + j[1]
                bx2, by2 = min(x2[o], ox + tile - 1) + j[2], min(y2[o], oy + tile - 1) + j[3]
                conf, cls_conf = rng.integers(8, 16) / 16.0, rng.integers(8, 17) / 16.0
                out_rows.append((ty * grid_x + tx, bx1, by1, bx2, by2, conf, cls_conf, cls[o]))
    for b in range(big):
        ty, tx = int(rng.integers(0, grid_y)), int(rng.integers(0, grid_x))
        oy, ox = ty * step, tx * step
        out_rows.append((ty * grid_x + tx, ox + 3, oy + 5, ox + tile - 4, oy + tile - 2, 1.0, 1.0, b % 2))   # stronger than every object row
    a = np.asarray(sorted(out_rows, key=lambda r: r[0]), np.float64).reshape(-1, 8)   # stable: tile order, objects in order within
    return a[:, 1:].astype(F32), a[:, 0].astype(np.int32)
