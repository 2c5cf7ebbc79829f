"""NumPy restatements of the library's oldest small kernels (TEST INFRASTRUCTURE ONLY; no torch on the device, no kernel involved):
the YOLO decode, the box math, the per-tile match, the fp32 train-mode BatchNorm, ay_fold_bn, the layout converters and the fp32
graph plumbing.  tests/test_small_kernels_cpu.py asserts the conditions the GPU tests rest on from this module alone,
tests/test_gpu_small_kernels.py holds the kernels to it.

Every kernel has two restatements:
  * a FLOAT64 REFERENCE (`*_f64`): the mathematical definition from the comments of include/amyloid_yolo.h on the float32 inputs;
  * a FLOAT32 TWIN (`*_twin`): the kernel's operations one by one in its order (the library is built with -ffp-contract=off and
    IEEE division and square root, so NumPy float32 `+ - * / sqrt min max` give the kernel's bits).

The comparison rule is the project's (profiles/yolo_loss_margins.txt):
  E   = the twin against float64, relative to the class scale, measured on the CPU;
  bar = max(4 E, 2^-22): what a GPU test asserts of the kernel against float64 (the factor 4 covers another expf, documented as at
        most 1 ulp);
  where the twin uses only `+ - * / sqrt min max` and comparisons the kernel must EQUAL the twin bit for bit, and no bar applies:
  IoU mode 0, GIoU, xywh2xyxy, fold_bn, the converters, the plumbing.
Class scales: decode x, y: stride * (g + 1); decode w, h and the sigmoids: the value itself; BatchNorm y: |z - mean| invstd |gamma| +
|beta|; dz: |k| (n |d| + |db| + |xh dg|); per-channel sums: the sum of the absolute terms.

Two edges the kernels take on purpose, restated here:
  * ay_bn_train_fwd_f32 with n = B * HW = 1 has no unbiased variance (n / (n - 1)): it feeds the BIASED variance (0) to running_var;
  * the half converter SATURATES: a finite float32 beyond the half range is stored as +-65504 (MODE.FP16_OVFL, set by every kernel
    that stores halves; test_half_storage_saturates_instead_of_overflowing), where torch-CPU's `.to(float16)` gives +-inf.
    `half_bits_device_rule` is torch's conversion with that one substitution; true infinities and NaNs pass through."""
import numpy as np

from oracle import boxes_oracle as bo

F32, F64 = np.float32, np.float64
FLOOR = 2.0 ** -22
FLT_MIN = float(np.finfo(F32).tiny)


def bar(E):
    return max(4.0 * float(E), FLOOR)


def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


# ================================================================================================ decode (models.py:127-172)
# (A, C, G, B, img_dim); the last one is beyond the fused entry points' six anchors (ay_yolo_decode only)
DECODE_CASES = [(3, 3, 13, 2, 416), (3, 2, 8, 1, 256), (2, 1, 5, 3, 100), (3, 2, 13, 1, 100), (3, 80, 4, 1, 128), (1, 1, 1, 1, 32),
                (6, 3, 3, 1, 96), (16, 1, 3, 1, 96)]
DECODE_GRID_STRIDE_CASE = (16, 1, 513, 1, 4104)   # 16 * 513^2 = 4 210 704 cells: the smallest square grid above 16384 x 256 threads
ROW_OFFSET, ROW_EXTRA = 5, 7                       # rows [5, 5 + A G G) of n_total = A G G + 7
ANCHORS16 = [(10, 13), (16, 30), (33, 23), (30, 61), (62, 45), (59, 119), (116, 90), (156, 198), (373, 326), (12, 12), (20, 41),
             (45, 17), (7, 9), (81, 82), (135, 169), (344, 319)]
EXTREME = [0.0, -0.0, 1e-40, -1e-40, 87.0, -87.0, 88.5, -88.5, 89.0, -89.0, 104.0, -104.0, np.inf, -np.inf, np.nan]
EXTREME_CASE = (3, 2, 6, 1, 192)                   # K = 7 slots x 15 values = 105 planted cells of the 108
FUSED_EXTREME_CASE = (3, 3, 2, 1, 64)              # the fused entry points take the logits per channel (shift): one slot per run; K = 8


def decode_id(case):
    return "A%d_C%d_G%d_B%d_S%d" % case


def anchors_of(A):
    return [tuple(float(v) for v in a) for a in ANCHORS16[:A]]


def decode_head(case, seed=0, sigma=3.0):
    A, C, G, B, _ = case
    return rng(1000 + seed + A * 131 + C * 17 + G).normal(0.0, sigma, (B, A * (5 + C), G, G)).astype(F32)


def _cells(head, A, K):
    B, _, G, _ = head.shape
    return head.reshape(B, A, K, G, G).transpose(0, 1, 3, 4, 2)          # [B, A, gy, gx, K]


def decode_f64(head, anchors, C, img_dim):
    """out[b, a G G + gy G + gx] = ((sig(tx) + gx) s, (sig(ty) + gy) s, exp(tw) aw, exp(th) ah, sig(conf), sig(cls...)), s = img_dim / G,
    aw, ah in pixels, in float64 -> [B, A G G, 5 + C]"""
    A, K = len(anchors), 5 + C
    p = _cells(np.asarray(head, F32), A, K).astype(F64)
    B, G = p.shape[0], p.shape[2]
    s = F64(img_dim) / F64(G)
    an = np.asarray(anchors, F64)
    out = np.empty(p.shape, F64)
    with np.errstate(over="ignore", invalid="ignore"):
        sig = 1.0 / (1.0 + np.exp(-p))
        out[..., 0] = (sig[..., 0] + np.arange(G, dtype=F64).reshape(1, 1, 1, G)) * s
        out[..., 1] = (sig[..., 1] + np.arange(G, dtype=F64).reshape(1, 1, G, 1)) * s
        out[..., 2] = np.exp(p[..., 2]) * an[:, 0].reshape(1, A, 1, 1)
        out[..., 3] = np.exp(p[..., 3]) * an[:, 1].reshape(1, A, 1, 1)
    out[..., 4:] = sig[..., 4:]
    return out.reshape(B, A * G * G, K)


def decode_twin(head, anchors, C, img_dim):
    """yolo_decode_kernel's expressions in float32: stride = (float)(img_dim / G in double); aw = anchor / stride;
    ((sig + g) * stride), ((exp * aw) * stride), sig = 1 / (1 + exp(-t))"""
    A, K = len(anchors), 5 + C
    p = _cells(np.asarray(head, F32), A, K)
    B, G = p.shape[0], p.shape[2]
    s = F32(float(img_dim) / float(G))
    an = np.asarray(anchors, F32) / s
    out = np.empty(p.shape, F32)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        sig = F32(1) / (F32(1) + np.exp(-p, dtype=F32))
        out[..., 0] = (sig[..., 0] + np.arange(G, dtype=F32).reshape(1, 1, 1, G)) * s
        out[..., 1] = (sig[..., 1] + np.arange(G, dtype=F32).reshape(1, 1, G, 1)) * s
        out[..., 2] = (np.exp(p[..., 2], dtype=F32) * an[:, 0].reshape(1, A, 1, 1)) * s
        out[..., 3] = (np.exp(p[..., 3], dtype=F32) * an[:, 1].reshape(1, A, 1, 1)) * s
    out[..., 4:] = sig[..., 4:]
    return out.reshape(B, A * G * G, K)


def decode_scale(ref64, A, G, img_dim):
    """class scale per entry of [B, A G G, K]: x -> stride (gx + 1), y -> stride (gy + 1), every other entry its own value"""
    s = F64(img_dim) / F64(G)
    sc = np.abs(np.asarray(ref64, F64)).copy()
    cell = np.arange(A * G * G)
    sc[:, :, 0] = (s * (cell % G + 1))[None, :]
    sc[:, :, 1] = (s * ((cell // G) % G + 1))[None, :]
    return sc


DECODE_CLASSES = (("xy", slice(0, 2)), ("wh", slice(2, 4)), ("sig", slice(4, None)))


def decode_errors(got, ref64, A, G, img_dim):
    """{class: largest |got - ref| / scale}"""
    err = np.abs(np.asarray(got, F64) - ref64) / decode_scale(ref64, A, G, img_dim)
    return {name: float(err[:, :, sl].max()) for name, sl in DECODE_CLASSES}


def blocked_head(head, fill=np.nan):
    """nchw f32 head -> blocked f32 [B][cpad / 16][G][G][16], cpad = channels rounded up to 32; the pad lanes hold `fill`"""
    B, ch, G, _ = head.shape
    cpad = (ch + 31) // 32 * 32
    full = np.full((B, cpad, G, G), fill, F32)
    full[:, :ch] = head
    return np.ascontiguousarray(full.reshape(B, cpad // 16, 16, G, G).transpose(0, 1, 3, 4, 2))


def extreme_head():
    """(base head, planted head, plan): plan[i] = (cell, slot, value) -- every value of EXTREME in every one of the 5 + C slots, one per
    cell (cell = a G G + gy G + gx of image 0)"""
    A, C, G, B, _ = EXTREME_CASE
    K = 5 + C
    base = decode_head(EXTREME_CASE, seed=77, sigma=2.0)
    planted = base.copy()
    plan = []
    view = planted.reshape(B, A, K, G * G)
    for k in range(K):
        for j, v in enumerate(EXTREME):
            cell = k * len(EXTREME) + j
            view[0, cell // (G * G), k, cell % (G * G)] = F32(v)
            plan.append((cell, k, float(F32(v))))
    return base, planted, plan


def fused_extreme_logits(base, A, K, G, j, k):
    """per-channel logits [A K] with slot k of anchor a planted with EXTREME[(j + 5 a) % 15], and the plan (cell, slot, value) of every
    cell of the G x G grid that then shows it"""
    logits = np.asarray(base, F32).copy()
    plan = []
    for a in range(A):
        v = F32(EXTREME[(j + 5 * a) % len(EXTREME)])
        logits[a * K + k] = v
        plan += [(a * G * G + c, k, float(v)) for c in range(G * G)]
    return logits, plan


def extreme_classes(plan, anchors, img_dim, G):
    """the class of every planted entry, from float64: 'nan' | 'inf' (float64 rounds to a float32 infinity) | 'tiny' (the exact result
    is below FLT_MIN x anchor for w, h, below FLT_MIN for a sigmoid) | 'one' / 'zero' (a sigmoid that rounds to 1 / 0 in float32; 'zero'
    is also 'tiny') | 'normal'.  -> list of (cell, slot, value, class, exact float64 result of the slot's function)"""
    out = []
    for cell, k, v in plan:
        a = cell // (G * G)
        with np.errstate(over="ignore", invalid="ignore"):
            if k in (2, 3):
                anc = F64(anchors[a][k - 2])
                r = np.exp(F64(v)) * anc
                with np.errstate(over="ignore"):
                    cls = "nan" if np.isnan(r) else "inf" if np.isinf(F32(r)) else "tiny" if r < FLT_MIN * anc else "normal"
            else:
                r = 1.0 / (1.0 + np.exp(-F64(v)))
                cls = "nan" if np.isnan(r) else "one" if F32(r) == F32(1) else "zero" if F32(r) == F32(0) else "tiny" if r < FLT_MIN else "normal"
        out.append((cell, k, v, cls, float(r)))
    return out


# ================================================================================================ box math (utils/utils.py:53-59,193-232)
iou_twin = bo.bbox_iou           # +1 rule, operation for operation (ay_box.h: iou_p1)
giou_twin = bo.bbox_giou
xywh2xyxy_twin = bo.xywh2xyxy


def _corners64(b, xyxy):
    b = np.asarray(b, F32).reshape(-1, 4).astype(F64)
    if xyxy:
        return b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    return b[:, 0] - b[:, 2] / 2, b[:, 1] - b[:, 3] / 2, b[:, 0] + b[:, 2] / 2, b[:, 1] + b[:, 3] / 2


def iou_f64(b1, b2, xyxy=True):
    ax1, ay1, ax2, ay2 = _corners64(b1, xyxy)
    bx1, by1, bx2, by2 = _corners64(b2, xyxy)
    inter = np.maximum(np.minimum(ax2, bx2) - np.maximum(ax1, bx1) + 1, 0) * np.maximum(np.minimum(ay2, by2) - np.maximum(ay1, by1) + 1, 0)
    return inter / ((ax2 - ax1 + 1) * (ay2 - ay1 + 1) + (bx2 - bx1 + 1) * (by2 - by1 + 1) - inter + 1e-16)


def giou_f64(b1, b2):
    """IoU - (hull - union) / hull on corner boxes, no +1 rule, with the 1e-16 the kernel adds to union and hull"""
    ax1, ay1, ax2, ay2 = _corners64(b1, True)
    bx1, by1, bx2, by2 = _corners64(b2, True)
    inter = np.maximum(np.minimum(ax2, bx2) - np.maximum(ax1, bx1), 0) * np.maximum(np.minimum(ay2, by2) - np.maximum(ay1, by1), 0)
    uni = (ax2 - ax1) * (ay2 - ay1) + (bx2 - bx1) * (by2 - by1) - inter + 1e-16
    hull = (np.maximum(ax2, bx2) - np.minimum(ax1, bx1)) * (np.maximum(ay2, by2) - np.minimum(ay1, by1)) + 1e-16
    return inter / uni - (hull - uni) / hull


HALF_IOU_PAIR = ([0.0, 0.0, 9.0, 9.0], [0.0, 0.0, 9.0, 4.0])      # +1 rule: 10 x 5 / 10 x 10 = 0.5f exactly
BELOW_HALF_IOU_PAIR = ([0.0, 0.0, 9.0, 9.0], [0.0, 0.0, 9.0, 3.9999995])


def box_classes():
    """{name: (box1 [n, 4], box2 [n, 4])} corner boxes of the classes the issue names"""
    r = rng(11)
    def rand(n, lo, span, size):
        xy = r.uniform(lo, lo + span, (n, 2))
        wh = r.uniform(1.0, size, (n, 2))
        return np.concatenate([xy, xy + wh], 1).astype(F32)
    n = 64
    a, b = rand(n, 0, 400, 120), rand(n, 0, 400, 120)
    cls = {"random": (a, b)}
    z = a.copy(); z[::3, 2] = z[::3, 0]; z[1::3, 3] = z[1::3, 1]; z[2::3, 2:] = z[2::3, :2]
    cls["zero_size"] = (z, b)
    cls["zero_both"] = (z, z[::-1].copy())
    cls["zero_same_point"] = (z[2::3], z[2::3].copy())
    cls["inverted"] = (a[:, [2, 3, 0, 1]].copy(), b)
    t = a.copy(); t[:, 0] = a[:, 2]; t[:, 2] = a[:, 2] + 30          # shares the edge column x2 of a: inter width 1 under the +1 rule
    cls["touching"] = (a, t)
    d = a.copy(); d[:, [0, 2]] += 1000
    cls["disjoint"] = (a, d)
    cls["identical"] = (a, a.copy())
    inner = a.copy(); inner[:, :2] += 0.25 * (a[:, 2:] - a[:, :2]); inner[:, 2:] -= 0.25 * (a[:, 2:] - a[:, :2])
    cls["nested"] = (a, inner.astype(F32))
    for name, lo in (("slide_2^17", 2.0 ** 17), ("slide_2^20", 2.0 ** 20)):
        p = rand(n, lo - 200, 400, 150)
        q = p + r.uniform(-40, 40, (n, 4)).astype(F32)
        cls[name] = (p, q.astype(F32))
    return cls


def all_boxes():
    """every class one after the other: (box1 [N, 4], box2 [N, 4])"""
    c = box_classes()
    return np.concatenate([v[0] for v in c.values()]), np.concatenate([v[1] for v in c.values()])


def to_cxcywh(b):
    """corner boxes -> centre boxes whose float32 fields are what a caller would hold (the kernel and the twin start from these)"""
    b = np.asarray(b, F32)
    return np.stack([(b[:, 0] + b[:, 2]) / F32(2), (b[:, 1] + b[:, 3]) / F32(2), b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1).astype(F32)


# ================================================================================================ match (utils/utils.py:154-190)
MAX_T = 2048     # ay_match_detections: targets per image; beyond, *overflow = 1 and the first 2048 (in target order) are matched


def match_image(rows, ann, thr):
    """get_batch_statistics for one image, with the mechanisms it went through: rows [n, 7], ann [m, 5] = (class, x1, y1, x2, y2) ->
    (tp [n] float32, events).  The same walk as oracle.boxes_oracle.get_batch_statistics (asserted equal in the CPU module)."""
    rows, ann = np.asarray(rows, F32).reshape(-1, 7), np.asarray(ann, F32).reshape(-1, 5)
    tp = np.zeros(rows.shape[0], F32)
    ev = dict(skipped_label=0, early_stop=0, cross_lane_tie=0, same_lane_tie=0, at_threshold=0, below_threshold=0, already_claimed=0, nan_row=0)
    if len(ann) == 0:
        return tp, ev
    detected = set()
    thr = F32(thr)
    for i in range(rows.shape[0]):
        if len(detected) == len(ann):
            ev["early_stop"] += 1
            break
        if not (ann[:, 0] == rows[i, 6]).any():
            ev["skipped_label"] += 1
            continue
        ious = bo.bbox_iou(rows[i:i + 1, :4], ann[:, 1:])
        if np.isnan(ious).any():
            ev["nan_row"] += 1
            continue
        bi = int(ious.argmax())
        ties = np.flatnonzero(ious == ious[bi])
        if ties.size > 1 and ious[bi] >= thr:
            ev["cross_lane_tie"] += int(np.unique(ties % 64).size > 1)
            ev["same_lane_tie"] += int(np.unique(ties % 64).size < ties.size)
        ev["at_threshold"] += int(ious[bi] == thr)
        ev["below_threshold"] += int(ious[bi] < thr and ious[bi] > thr - F32(1e-3))
        if ious[bi] >= thr:
            if bi in detected:
                ev["already_claimed"] += 1
            else:
                tp[i] = 1
                detected.add(bi)
    return tp, ev


def match_batch(rows, count, targets, thr):
    """rows [B, max_det, 7], count [B] (clamped to max_det), targets [nT, 6] -> (tp [B, max_det] float32, overflow, events summed)"""
    rows, targets = np.asarray(rows, F32), np.asarray(targets, F32).reshape(-1, 6)
    B, max_det = rows.shape[:2]
    tp = np.zeros((B, max_det), F32)
    total, overflow = {}, 0
    for b in range(B):
        ann = targets[targets[:, 0] == b][:, 1:]
        if len(ann) > MAX_T:
            overflow, ann = 1, ann[:MAX_T]
        n = min(int(count[b]), max_det)
        tp[b, :n], ev = match_image(rows[b, :n], ann, thr)
        for k, v in ev.items():
            total[k] = total.get(k, 0) + v
    return tp, overflow, total


def _grid_boxes(n, side=10.0, pitch=20.0, per_row=64):
    i = np.arange(n)
    x, y = (i % per_row) * pitch, (i // per_row) * pitch
    return np.stack([x, y, x + side - 1, y + side - 1], 1).astype(F32)


def _rows(boxes, labels, conf=None):
    n = len(boxes)
    conf = np.linspace(0.99, 0.5, n) if conf is None else conf
    return np.concatenate([np.asarray(boxes, F32).reshape(n, 4), np.asarray(conf, F32).reshape(n, 1), np.full((n, 1), 0.9, F32),
                           np.asarray(labels, F32).reshape(n, 1)], 1).astype(F32)


def _pad_rows(per_image, max_det):
    B = len(per_image)
    rows = np.zeros((B, max_det, 7), F32)
    count = np.zeros(B, np.int32)
    for b, r in enumerate(per_image):
        rows[b, :len(r)] = r
        count[b] = len(r)
    return rows, count


def _targets(per_image):
    out = [np.concatenate([np.full((len(a), 1), b, F32), np.asarray(a, F32).reshape(-1, 5)], 1) for b, a in enumerate(per_image) if len(a)]
    return np.concatenate(out).astype(F32) if out else np.zeros((0, 6), F32)


def match_cases():
    """{name: dict(rows [B, max_det, 7], count [B], targets [nT, 6], thr, needs = the events that must occur in the oracle's run)}"""
    r = rng(5)
    cases = {}
    tb = _grid_boxes(12)
    lab = np.arange(12) % 3
    ann = np.concatenate([lab[:, None].astype(F32), tb], 1)

    # image 0: detections, no targets; image 1: targets, count 0; image 2: ordinary; targets of a sample index >= batch are ignored
    det = _rows(tb[::-1] + r.uniform(-1, 1, (12, 4)).astype(F32), lab[::-1])
    rows, count = _pad_rows([det, det[:0], det], 16)
    tg = np.concatenate([_targets([[], ann, ann]), np.concatenate([np.full((12, 1), 3, F32), ann], 1), np.concatenate([np.full((12, 1), 7, F32), ann], 1)])
    cases["empty_sides"] = dict(rows=rows, count=count, targets=tg, thr=0.5, needs=[])

    # count[b] > max_det clamps: rows beyond max_det do not exist, tp beyond count is 0
    rows, count = _pad_rows([det[:8], det[:5]], 8)
    count[0] = 11
    cases["count_clamp"] = dict(rows=rows, count=count, targets=_targets([ann, ann]), thr=0.5, needs=[])

    # a label absent from the image's targets: skipped, claims nothing even at IoU 1; then the same box with a present label is a TP
    d2 = _rows(np.concatenate([tb[:4], tb[:4]]), [9, 9, 9, 9, 0, 1, 2, 0])
    rows, count = _pad_rows([d2], 8)
    cases["absent_label"] = dict(rows=rows, count=count, targets=_targets([ann]), thr=0.5, needs=["skipped_label"])

    # every target claimed by the first rows: all later rows are 0 although they overlap a target exactly
    d3 = _rows(np.concatenate([tb[:3], tb[:3], tb[:3]]), np.concatenate([lab[:3]] * 3))
    rows, count = _pad_rows([d3], 9)
    cases["early_stop"] = dict(rows=rows, count=count, targets=_targets([ann[:3]]), thr=0.5, needs=["early_stop"])

    # duplicate targets at t, t + 1, t + 64, t + 65: the first index wins every time, across lanes and inside a lane
    many = _grid_boxes(140)
    t0 = 37
    for k in (1, 64, 65):
        many[t0 + k] = many[t0]
    annm = np.concatenate([np.zeros((140, 1), F32), many], 1)
    d4 = _rows(np.stack([many[t0]] * 5 + [many[3], many[100]]), np.zeros(7))
    rows, count = _pad_rows([d4], 7)
    cases["duplicates"] = dict(rows=rows, count=count, targets=_targets([annm]), thr=0.5, needs=["cross_lane_tie", "same_lane_tie", "already_claimed"])

    # IoU exactly 0.5 at iou_thres = 0.5 is a TP; just below is not
    a_box, half = HALF_IOU_PAIR
    _, below = BELOW_HALF_IOU_PAIR
    far = [100.0, 100.0, 109.0, 109.0]
    annt = np.asarray([[0] + a_box, [0] + far], F32)
    d5 = _rows(np.asarray([below, half, [100.0, 100.0, 109.0, 103.9999]], F32), [0, 0, 0])
    rows, count = _pad_rows([d5], 4)
    cases["threshold"] = dict(rows=rows, count=count, targets=_targets([annt]), thr=0.5, needs=["at_threshold", "below_threshold"])

    # a NaN detection box: no TP, no claim; the rows behind it match as if it were not there
    d6 = _rows(np.concatenate([tb[:2], tb[2:3] * np.nan, tb[2:6]]), [lab[0], lab[1], lab[2], lab[2], lab[3], lab[4], lab[5]])
    d6[1, 0] = np.nan
    rows, count = _pad_rows([d6], 8)
    cases["nan_box"] = dict(rows=rows, count=count, targets=_targets([ann]), thr=0.5, needs=["nan_row"])

    # B = 1 is every single-image case above; B = 65: a wave per image, random images, some empty
    per_rows, per_ann = [], []
    for b in range(65):
        m = int(r.integers(0, 40)) if b % 7 else 0
        tbb = _grid_boxes(m) if m else np.zeros((0, 4), F32)
        lb = r.integers(0, 3, m)
        per_ann.append(np.concatenate([lb[:, None].astype(F32), tbb], 1) if m else np.zeros((0, 5), F32))
        nd = int(r.integers(0, 24)) if b % 5 else 0
        pick = r.integers(0, max(m, 1), nd)
        db = (tbb[pick] + r.uniform(-3, 3, (nd, 4)).astype(F32)) if m else r.uniform(0, 50, (nd, 4)).astype(F32)
        per_rows.append(_rows(db, r.integers(0, 4, nd), np.sort(r.uniform(0.1, 1, nd))[::-1]) if nd else np.zeros((0, 7), F32))
    rows, count = _pad_rows(per_rows, 24)
    cases["batch65"] = dict(rows=rows, count=count, targets=_targets(per_ann), thr=0.5, needs=["skipped_label", "already_claimed"])
    return cases


def cap_case(n_targets):
    """one image with n_targets disjoint targets and one exact detection per target, in shuffled order (2048: all matched, overflow 0;
    2049: the detection of target 2048 meets no target among the first 2048, overflow 1)"""
    tb = _grid_boxes(n_targets)
    lab = np.arange(n_targets) % 2
    ann = np.concatenate([lab[:, None].astype(F32), tb], 1)
    order = rng(n_targets).permutation(n_targets)
    rows, count = _pad_rows([_rows(tb[order], lab[order])], n_targets)
    return dict(rows=rows, count=count, targets=_targets([ann]), thr=0.5, needs=[])


# ================================================================================================ fp32 BatchNorm (models.py:43-45)
BN_SHAPES = [(3, 20, 49), (1, 1, 1), (2, 3, 1), (1, 5, 255), (1, 5, 256), (1, 5, 257), (2, 7, 4099), (4, 33, 64 * 64)]   # (B, C, HW)
BN_MOMENTA = (0.0, 0.1, 1.0)
BN_EPS = 1e-5


def bn_id(shape):
    return "B%d_C%d_HW%d" % shape


def bn_inputs(shape, kind="random"):
    """z [B, C, HW], gamma, beta, running_mean, running_var [C], dy [B, C, HW]; kind: 'random' | 'cancel' (channel mean 1e4, standard
    deviation 1e-2) | 'const' (every channel one constant: variance 0) | 'zero_y' (channel mean exactly 0 with pixels at 0, beta = 0)"""
    B, C, HW = shape
    r = rng(B * 1000 + C * 10 + HW)
    z = (r.normal(0, 2, shape) + r.normal(0, 1, (1, C, 1))).astype(F32)
    gamma = (r.uniform(0.5, 1.5, C) * np.where(np.arange(C) % 4 == 3, -1, 1)).astype(F32)
    beta = r.normal(0, 1, C).astype(F32)
    if kind == "cancel":
        z = (1e4 + r.normal(0, 1e-2, shape)).astype(F32)
    elif kind == "const":
        z = np.broadcast_to(r.normal(0, 3, (1, C, 1)).astype(F32), shape).copy()
    elif kind == "zero_y":
        assert (B * HW) % 4 == 0
        pat = np.tile(np.asarray([-1.5, 0.0, 1.5, 0.0], F32), B * HW // 4).reshape(B, 1, HW)
        z = (pat * r.integers(1, 4, (1, C, 1)).astype(F32)).astype(F32)     # sums to exactly 0 in every channel
        beta = np.zeros(C, F32)
    rm, rv = r.normal(0, 1, C).astype(F32), r.uniform(0.5, 1.5, C).astype(F32)
    dy = r.normal(0, 1, shape).astype(F32)
    return z, gamma, beta, rm, rv, dy


def _stats64(z):
    zz = np.asarray(z, F32).astype(F64)
    n = zz.shape[0] * zz.shape[2]
    mean = zz.sum((0, 2)) / n
    var = ((zz - mean[None, :, None]) ** 2).sum((0, 2)) / n          # biased
    return zz, n, mean, var


def bn_fwd_f64(z, gamma, beta, rm, rv, momentum, eps, leaky):
    """train-mode BatchNorm2d + LeakyReLU(0.1) with PyTorch's running statistics (unbiased variance n / (n - 1); n = 1: biased, the
    kernel's rule) -> dict of float64 arrays and the class scales"""
    zz, n, mean, var = _stats64(z)
    g, bt, m, e = (np.asarray(v, F32).astype(F64) for v in (gamma, beta, momentum, eps))
    invstd = 1.0 / np.sqrt(var + e)
    pre = (zz - mean[None, :, None]) * invstd[None, :, None] * g[None, :, None] + bt[None, :, None]
    y = np.where(pre > 0, pre, 0.1 * pre) if leaky else pre
    unb = var * n / (n - 1) if n > 1 else var
    absmean = np.abs(zz).sum((0, 2)) / n
    return dict(y=y, save_mean=mean, save_invstd=invstd, running_mean=(1 - m) * rm.astype(F64) + m * mean,
                running_var=(1 - m) * rv.astype(F64) + m * unb,
                scale=dict(y=np.abs(zz - mean[None, :, None]) * invstd[None, :, None] * np.abs(g)[None, :, None] + np.abs(bt)[None, :, None],
                           save_mean=absmean, save_invstd=invstd, running_mean=(1 - m) * np.abs(rm.astype(F64)) + m * absmean,
                           running_var=(1 - m) * np.abs(rv.astype(F64)) + m * unb))


def bn_fwd_twin(z, gamma, beta, rm, rv, momentum, eps, leaky):
    """bn_train_fwd_kernel: float64 sums of the float32 values (mean, then the centred second moment), mean and invstd rounded to
    float32 once, then ((z - mean) * invstd) * gamma + beta, v > 0 ? v : 0.1f * v, all float32; running = (1 - m) * running + m * batch"""
    zz, n, mean_d, var_d = _stats64(z)
    z = np.asarray(z, F32)
    m = F32(momentum)
    mean = mean_d.astype(F32)
    invstd = (1.0 / np.sqrt(var_d + F64(F32(eps)))).astype(F32)
    v = (z - mean[None, :, None]) * invstd[None, :, None] * np.asarray(gamma, F32)[None, :, None] + np.asarray(beta, F32)[None, :, None]
    if leaky:
        v = np.where(v > 0, v, F32(0.1) * v)
    unb = (var_d * F64(n) / F64(n - 1)).astype(F32) if n > 1 else var_d.astype(F32)
    return dict(y=v.astype(F32), save_mean=mean, save_invstd=invstd, running_mean=(F32(1) - m) * np.asarray(rm, F32) + m * mean,
                running_var=(F32(1) - m) * np.asarray(rv, F32) + m * unb)


def bn_apply_twin(z, mean, invstd, gamma, beta, leaky):
    """the apply pass alone, from GIVEN float32 statistics: ((z - mean) * invstd) * gamma + beta, v > 0 ? v : 0.1f * v -- float32
    + - * and a comparison only, so the kernel's y equals this on the mean and invstd it saved, bit for bit"""
    v = (np.asarray(z, F32) - np.asarray(mean, F32)[None, :, None]) * np.asarray(invstd, F32)[None, :, None] \
        * np.asarray(gamma, F32)[None, :, None] + np.asarray(beta, F32)[None, :, None]
    if leaky:
        v = np.where(v > 0, v, F32(0.1) * v)
    return v.astype(F32)


def _bwd_common(dy, y, z, leaky, T):
    d = np.asarray(dy, F32).astype(T)
    if leaky:
        d = np.where(np.asarray(y, F32) > 0, d, d * T(0.1))          # !(y > 0): the slope of y <= 0, y == 0 included (and NaN)
    return d, np.asarray(z, F32).astype(T)


def bn_bwd_f64(dy, y, z, gamma, save_mean, save_invstd, leaky):
    """autograd of bn_fwd as a function of the kernel's inputs: d = dy * leaky'(y); dbeta = sum d; dgamma = sum d xh;
    dz = gamma invstd / n * (n d - dbeta - xh dgamma), xh = (z - mean) invstd"""
    d, zz = _bwd_common(dy, y, z, leaky, F64)
    n = zz.shape[0] * zz.shape[2]
    mean, invstd, g = (np.asarray(v, F32).astype(F64)[None, :, None] for v in (save_mean, save_invstd, gamma))
    xh = (zz - mean) * invstd
    db, dg = d.sum((0, 2)), (d * xh).sum((0, 2))
    k = g * invstd / n
    dz = k * (n * d - db[None, :, None] - xh * dg[None, :, None])
    return dict(dz=dz, dgamma=dg, dbeta=db,
                scale=dict(dz=np.abs(k) * (n * np.abs(d) + np.abs(db)[None, :, None] + np.abs(xh * dg[None, :, None])),
                           dgamma=np.abs(d * xh).sum((0, 2)), dbeta=np.abs(d).sum((0, 2))))


def bn_bwd_twin(dy, y, z, gamma, save_mean, save_invstd, leaky):
    """bn_train_bwd_kernel: d and d * ((z - mean) * invstd) in float32, summed in float64, rounded once; k = gamma * invstd / (float)n;
    dz = k * (((float)n * d - db) - xh * dg)"""
    d, zf = _bwd_common(dy, y, z, leaky, F32)
    n = zf.shape[0] * zf.shape[2]
    mean, invstd, g = (np.asarray(v, F32)[None, :, None] for v in (save_mean, save_invstd, gamma))
    xh = (zf - mean) * invstd
    db = d.astype(F64).sum((0, 2)).astype(F32)
    dg = (d * xh).astype(F32).astype(F64).sum((0, 2)).astype(F32)
    k = g * invstd / F32(n)
    dz = k * (F32(n) * d - db[None, :, None] - xh * dg[None, :, None])
    return dict(dz=dz.astype(F32), dgamma=dg, dbeta=db)


def channel_errors(got, ref, scale):
    """largest |got - ref| / scale PER CHANNEL (axis 1 of [B, C, HW], axis 0 of [C]); 0 / 0 counts as 0"""
    err = np.abs(np.asarray(got, F64) - ref)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(err == 0, 0.0, err / scale)
    return rel.max((0, 2)) if rel.ndim == 3 else rel


# ================================================================================================ ay_fold_bn (models.py:43 in eval mode)
def fold_bn_twin(gamma, beta, mean, var, bias, eps, n, n_pad):
    """scale = gamma / sqrtf(var + eps), shift = beta - mean * scale | scale = 1, shift = bias | scale = 1, shift = 0; exact +0 in
    [n, n_pad)"""
    scale, shift = np.zeros(n_pad, F32), np.zeros(n_pad, F32)
    if gamma is not None:
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            scale[:n] = np.asarray(gamma, F32) / np.sqrt(np.asarray(var, F32) + F32(eps), dtype=F32)
            shift[:n] = np.asarray(beta, F32) - np.asarray(mean, F32) * scale[:n]
    else:
        scale[:n] = 1
        if bias is not None:
            shift[:n] = np.asarray(bias, F32)
    return scale, shift


# ================================================================================================ layout converters
LAYOUT_SHAPES = [(2, 3, 5, 7), (1, 17, 4, 4), (3, 24, 9, 2), (1, 255, 3, 3)]      # (B, C, H, W)


def bf16_rne_bits(u):
    """uint32 float32 patterns -> uint16 bfloat16 patterns by round to nearest even in integers (NaNs: any NaN pattern, see is_nan32)"""
    u = np.asarray(u, np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def f16_rne_bits(u):
    """uint32 float32 patterns -> uint16 IEEE half patterns by round to nearest even in integers: overflow to infinity, gradual
    underflow (NaN inputs: see is_nan32)"""
    u = np.asarray(u, np.uint32).astype(np.int64)
    sign = (u >> 16) & 0x8000
    a = u & 0x7FFFFFFF
    exp, man = a >> 23, a & 0x7FFFFF
    # normal halves: rebias the exponent (127 -> 15), round the 13 dropped bits to even; a carry runs into the exponent, up to infinity
    an = a - (112 << 23)
    hn = np.minimum((an + 0xFFF + ((an >> 13) & 1)) >> 13, 0x7C00)
    # subnormal halves: value = m * 2^(exp - 150), the half unit is 2^-24 -> shift the 24-bit significand right by 126 - exp
    m = man | 0x800000
    sh = np.clip(126 - exp, 1, 40)
    hs = (m + (np.int64(1) << (sh - 1)) - 1 + ((m >> sh) & 1)) >> sh
    h = np.where(exp >= 113, hn, np.where(exp == 0, 0, hs))
    h = np.where(a >= 0x7F800000, 0x7C00, h)                       # infinity (and NaN, compared as NaN)
    return (sign | h).astype(np.uint16)


def is_nan32(u):
    return (np.asarray(u, np.uint32) & 0x7FFFFFFF) > 0x7F800000


def bf16_sweep():
    """for every bfloat16 pattern u the float32 patterns (u << 16) | {0, 1, 0x7fff, 0x8000, 0x8001, 0xffff}: 393 216 uint32"""
    hi = np.arange(65536, dtype=np.uint32) << 16
    return (hi[:, None] | np.asarray([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)[None, :]).reshape(-1)


def f16_sweep():
    """for every finite half h the float32 midpoint to its successor (65536 behind 65504) and that midpoint's two float32 neighbours,
    both signs: 190 464 uint32, the four values that round to +-inf and the subnormal range included"""
    h = np.arange(0x7C00, dtype=np.uint16)
    lo = h.view(np.float16).astype(F32)
    hi = np.append(lo[1:], F32(65536.0))
    mid = ((lo.astype(F64) + hi.astype(F64)) / 2).astype(F32)      # exact: at most 12 significant bits
    assert np.array_equal(mid.astype(F64) * 2, lo.astype(F64) + hi.astype(F64))
    pos = np.stack([np.nextafter(mid, F32(-np.inf)), mid, np.nextafter(mid, F32(np.inf))], 1).reshape(-1).astype(F32)
    return np.concatenate([pos, -pos]).view(np.uint32)


def half_bits_device_rule(src_bits, torch_bits):
    """torch-CPU `.to(float16)` bits with the converter's documented saturation: finite input, infinite result -> +-65504"""
    src_bits, out = np.asarray(src_bits, np.uint32), np.asarray(torch_bits, np.uint16).copy()
    sat = ((src_bits & 0x7FFFFFFF) < 0x7F800000) & ((out & 0x7FFF) == 0x7C00)
    out[sat] = (out[sat] & 0x8000) | 0x7BFF
    return out


def to_blocked(x, fill=0):
    """[B, C, H, W] -> [B, ceil(C / 16), H, W, 16], pad lanes `fill`"""
    B, C, H, W = x.shape
    CP = (C + 15) // 16
    full = np.full((B, CP * 16, H, W), fill, x.dtype)
    full[:, :C] = x
    return np.ascontiguousarray(full.reshape(B, CP, 16, H, W).transpose(0, 1, 3, 4, 2))


def from_blocked(xb, C):
    B, CP, H, W, _ = xb.shape
    return np.ascontiguousarray(xb.transpose(0, 1, 4, 2, 3).reshape(B, CP * 16, H, W)[:, :C])


def concat_upsample_twin(s1, up1, s2):
    """blocked 16-bit tensors as uint16 [B, P, H, W, 16]: planes of s1 (each pixel repeated 2 x 2 if up1), then the planes of s2"""
    if up1:
        s1 = s1.repeat(2, axis=2).repeat(2, axis=3)
    return np.ascontiguousarray(s1 if s2 is None else np.concatenate([s1, s2], 1))


# ================================================================================================ fp32 plumbing (models.py:86-96,244-248)
def copy_channels_twin(src, out, c0, up):
    """out[b, c0 + c, y, x] = src[b, c, y >> up, x >> up]; every other channel of `out` stays"""
    s = src.repeat(2, axis=2).repeat(2, axis=3) if up else src
    out = out.copy()
    out[:, c0:c0 + src.shape[1]] = s
    return out


def slice_accumulate_twin(dout, dsrc, c0, up):
    """dsrc[b, c, ys, xs] += ((0 + d00) + d01) + d10) + d11 over the (1 << up)^2 children of dout[b, c0 + c], float32 in that order"""
    csrc = dsrc.shape[1]
    d = np.asarray(dout, F32)[:, c0:c0 + csrc]
    if up:
        s = ((d[:, :, 0::2, 0::2] + d[:, :, 0::2, 1::2]) + d[:, :, 1::2, 0::2]) + d[:, :, 1::2, 1::2]
    else:
        s = d
    return (np.asarray(dsrc, F32) + s).astype(F32)
