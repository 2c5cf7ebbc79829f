"""THE SLIDE MATCH RULE (include/amyloid_yolo.h) restated in NumPy float32 the way the reference writes its matching
(utils/utils.py:154-190): drop what the ROI ignores, sort the rows by rank, then walk them one after the other with a list of the
targets already detected, each row against ALL targets (no grid, no atomics, no keys).  Also the seeded cases the CPU and the
GPU tests share."""
import numpy as np

f32 = np.float32


def scores(rows):
    return (rows[:, 4] * rows[:, 5]).astype(f32)


def rank_order(rows):
    """row indices by descending conf * cls_conf, ties by ascending index"""
    return np.argsort(-scores(rows), kind="stable")


def centre_outside(boxes, roi):
    """boxes [n,4] (x1, y1, x2, y2): True where the centre lies outside the closed rectangle"""
    if roi is None:
        return np.zeros(len(boxes), bool)
    rx1, ry1, rx2, ry2 = (f32(v) for v in roi)
    cx = (boxes[:, 0] + boxes[:, 2]) * f32(0.5)
    cy = (boxes[:, 1] + boxes[:, 3]) * f32(0.5)
    with np.errstate(invalid="ignore"):
        return ~((cx >= rx1) & (cx <= rx2) & (cy >= ry1) & (cy <= ry2))


def bbox_iou(box, tb):
    """bbox_iou(x1y1x2y2=True) of utils/utils.py: one box [4] against tb [n,4], float32, +1 pixel convention"""
    one = f32(1.0)
    ix1, iy1 = np.maximum(box[0], tb[:, 0]), np.maximum(box[1], tb[:, 1])
    ix2, iy2 = np.minimum(box[2], tb[:, 2]), np.minimum(box[3], tb[:, 3])
    inter = np.maximum(ix2 - ix1 + one, f32(0)) * np.maximum(iy2 - iy1 + one, f32(0))
    a1 = (box[2] - box[0] + one) * (box[3] - box[1] + one)
    a2 = (tb[:, 2] - tb[:, 0] + one) * (tb[:, 3] - tb[:, 1] + one)
    return (inter / (a1 + a2 - inter + f32(1e-16))).astype(f32)


def match_slide(rows, targets, iou_thres=0.5, roi=None):
    """-> dict of tp uint8 [K,M], best_iou f32 [M], best_target int32 [M], claim int32 [K,T], row_ignored, target_ignored bool,
    eligible, claimed int32 [K]"""
    rows = np.asarray(rows, f32).reshape(-1, 7)
    targets = np.asarray(targets, f32).reshape(-1, 5)
    thres = [f32(v) for v in np.atleast_1d(np.asarray(iou_thres, np.float64))]
    M, T, K = len(rows), len(targets), len(thres)
    row_ignored, target_ignored = centre_outside(rows[:, :4], roi), centre_outside(targets[:, 1:], roi)
    keep_t = np.flatnonzero(~target_ignored)          # the annotations of this "image", in their order
    annotations = targets[keep_t]
    target_labels, target_boxes = annotations[:, 0], annotations[:, 1:]
    best_iou, best_target = np.zeros(M, f32), np.full(M, -1, np.int32)
    tp, claim = np.zeros((K, M), np.uint8), np.full((K, T), -1, np.int32)
    eligible, claimed = np.zeros(K, np.int32), np.zeros(K, np.int32)
    order = [i for i in rank_order(rows) if not row_ignored[i]]
    for i in order:                                    # what the walk below would find, reported for every row
        if len(annotations):
            iou = bbox_iou(rows[i, :4], target_boxes)
            j = int(np.argmax(iou))                    # first maximum, as torch.max
            if iou[j] > 0:
                best_iou[i], best_target[i] = iou[j], keep_t[j]
    for k, thr in enumerate(thres):
        detected_boxes = []
        for i in order:
            pred_box, pred_label = rows[i, :4], rows[i, 6]
            if len(annotations) == 0:
                break
            if pred_label not in target_labels:
                continue
            iou = bbox_iou(pred_box, target_boxes)
            box_index = int(np.argmax(iou))
            if iou[box_index] >= thr:
                eligible[k] += 1                       # (counted past the reference's early exit too: see below)
                if len(detected_boxes) < len(annotations) and box_index not in detected_boxes:
                    tp[k, i] = 1
                    detected_boxes.append(box_index)
                    claim[k, keep_t[box_index]] = i
        claimed[k] = len(detected_boxes)
    # The reference leaves its loop once every annotation is detected; no later row could become a true positive then, so walking
    # on (to count the eligible rows) changes no flag.
    return {"tp": tp, "best_iou": best_iou, "best_target": best_target, "claim": claim, "row_ignored": row_ignored,
            "target_ignored": target_ignored, "eligible": eligible, "claimed": claimed}


def lost_claims(res, k=0):
    """eligible rows that are no true positive at threshold k: their target went to a row of better rank"""
    return int(res["eligible"][k]) - int(res["tp"][k].sum())


def label_absent_rows(rows, targets, res):
    live_t = ~res["target_ignored"]
    return int((~np.isin(rows[:, 6], targets[live_t, 0]) & ~res["row_ignored"]).sum())


def check_not_idle(rows, targets, res, big=()):
    """asserted on the RESTATEMENT's output, before a kernel is looked at: at threshold 0.5 the case holds a true positive, an
    eligible row that lost its claim and a row whose label no target has; every target of `big` is claimed"""
    tp, lost, absent = int(res["tp"][1].sum()), lost_claims(res, 1), label_absent_rows(rows, targets, res)
    assert tp >= 1, "no true positive"
    if len(rows) > 1:        # (a single row cannot be a true positive, a loser and a stranger at once)
        assert lost >= 1 and absent >= 1, (lost, absent)
    for g in big:
        assert res["claim"][1][g] >= 0, g
    return tp, lost, absent


THRES = [0.3, 0.5, 0.75]
SIZES_M, SIZES_T = [1, 63, 64, 65, 1000, 5000], [1, 64, 300, 2049, 6000]
SEED_OVERRIDES = {(1, 64): 1, (1, 2049): 2}    # (the default seed gives that single row no true positive)


def case_seed(M, T):
    return SEED_OVERRIDES.get((M, T), 1000 * M + T)


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def row(x1, y1, x2, y2, conf=0.9, cls_conf=1.0, cls=0):
    return [x1, y1, x2, y2, conf, cls_conf, cls]


def random_slide(M, T, seed, fractional, classes=3):
    """T targets of 8-47 px (a third of them copies of another target, some with another class) on a square whose side grows with
    sqrt(T); M rows: four in five are jittered copies of a few of the targets (several rows per target, so that claims are
    contested), the others random boxes; one row in ten carries a label no target has; scores in eighths (many ties)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    side = 60.0 * np.sqrt(T) + 100.0
    xy = rng.uniform(0, side, (T, 2))
    wh = rng.uniform(8, 47, (T, 2))
    tb = np.concatenate([xy, xy + wh], 1)
    cls = rng.integers(0, classes, T).astype(np.float64)
    for t in rng.permutation(np.arange(1, T))[: T // 3]:
        tb[t] = tb[rng.integers(0, t)]                      # an exact copy of a target of lower index
    if not fractional:
        tb = np.round(tb)
    targets = np.concatenate([cls[:, None], tb], 1).astype(f32)
    pool = rng.permutation(T)[: max(1, min(T, M // 3))]
    rows = np.zeros((M, 7))
    for i in range(M):
        if rng.uniform() < 0.8:
            g = pool[rng.integers(0, len(pool))]
            box = tb[g] + rng.normal(0, rng.choice([0.0, 1.0, 3.0, 8.0]), 4)
            label = cls[g] if rng.uniform() < 0.8 else rng.integers(0, classes)
        else:
            p = rng.uniform(0, side, 2)
            box = np.concatenate([p, p + rng.uniform(8, 47, 2)])
            label = rng.integers(0, classes)
        if rng.uniform() < 0.1:
            label = classes                                 # no target has it
        rows[i] = [*(box if fractional else np.round(box)), rng.integers(1, 9) / 8.0, rng.integers(4, 9) / 8.0, label]
    return rows.astype(f32), targets


def geometry_case(name, seed=11):
    """-> rows, targets, indices of the targets meant for the oversize list"""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows, targets = random_slide(600, 900, seed, True)
    big = []
    if name == "oversize":       # three tile-sized annotations, rows on them, and one detection that covers the whole slide
        side = 60.0 * np.sqrt(900) + 100.0
        extra = [[0, 100, 150, 1500, 1600], [1, 700, 300, 2100, 1500], [2, 400, 900, 1700, 1800]]
        big = list(range(len(targets), len(targets) + 3))
        targets = np.concatenate([targets, np.asarray(extra, f32)])
        more = [row(*(np.asarray(e[1:]) + rng.normal(0, 6, 4)), 1.0, 1.0, e[0]) for e in extra for _ in range(2)]
        more.append(row(0, 0, side + 47, side + 47, 0.5, 1.0, 0))
        rows = np.concatenate([rows, np.asarray(more, f32)])
    elif name == "borders":      # centres on multiples of 256 from the smallest centre: a cell border for every power-of-two side
        n = 6
        cx, cy = np.meshgrid(np.arange(n) * 256.0, np.arange(n) * 256.0)
        c = np.stack([cx.ravel(), cy.ravel()], 1)
        half = rng.integers(4, 23, (n * n, 2)).astype(np.float64)      # even sides: the centres are exact
        tb = np.concatenate([c - half, c + half], 1)
        targets = np.concatenate([rng.integers(0, 3, (n * n, 1)), tb], 1).astype(f32)
        jit = rng.integers(-3, 4, (4 * n * n, 4))
        rows = np.concatenate([np.tile(tb, (4, 1)) + jit, rng.integers(1, 9, (4 * n * n, 1)) / 8.0, np.ones((4 * n * n, 1)),
                               np.tile(targets[:, :1], (4, 1))], 1).astype(f32)
        rows[::7, 6] = 3
    elif name == "one_cell":     # every target centre within 6 px of one point
        T = 200
        c = 500.0 + rng.uniform(-6, 6, (T, 2))
        half = rng.uniform(4, 8, (T, 2))
        tb = np.concatenate([c - half, c + half], 1)
        targets = np.concatenate([rng.integers(0, 3, (T, 1)), tb], 1).astype(f32)
        M = 500
        g = rng.integers(0, T, M)
        rows = np.concatenate([tb[g] + rng.normal(0, 0.7, (M, 4)), rng.integers(1, 9, (M, 1)) / 8.0, np.ones((M, 1)),
                               targets[g, :1]], 1).astype(f32)
        rows[::9, 6] = 3
    elif name == "far_target":   # one annotation a million pixels away: the grid must stay bounded, and the target is still found
        far = np.asarray([[1, 1.0e6, 1.0e6, 1.0e6 + 30, 1.0e6 + 24]], f32)
        targets = np.concatenate([targets, far])
        rows = np.concatenate([rows, np.asarray([row(1.0e6 + 1, 1.0e6, 1.0e6 + 30, 1.0e6 + 25, 0.75, 1.0, 1)], f32)])
    else:
        raise KeyError(name)
    return rows, targets, big


GEOMETRY_CASES = ["oversize", "borders", "one_cell", "far_target"]


def golden_image(outputs, targets, b):
    """image b of golden_cases.stats_inputs() as one slide: conf a strictly decreasing ramp, cls_conf 1 (rank order = row order)"""
    rows = outputs[b].copy()
    rows[:, 4] = np.linspace(1.0, 0.5, len(rows), dtype=f32)
    rows[:, 5] = 1.0
    assert (np.diff(rows[:, 4]) < 0).all()
    return rows, targets[targets[:, 0] == b][:, 1:].copy()
