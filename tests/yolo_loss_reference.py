"""Reference of the YOLO loss kernels (ay_yolo_loss_fwd_bwd, ay_yolo_loss_giou_fwd_bwd, ay_build_targets): NumPy and torch on the
CPU, TEST INFRASTRUCTURE ONLY, does not import the library.

Two layers, kept apart on purpose:
  * the ASSIGNMENT -- each target's cell, best anchor, ignore flags, last-writer winner, multi-hot classes, and the integer metrics
    (class hit, conf > 0.5, IoU > 0.5 / 0.75) -- is a set of float32 decisions and goes through oracle.boxes_oracle.decode and
    build_targets, which follow the reference's operation order in float32.  The cases keep every such decision away from its
    threshold (tests/test_yolo_loss_cpu.py asserts the margins), or exactly on it where a float32 tie is the point (`edges`);
  * the VALUES -- the fifteen sums in the layout commented above yolo_loss_pass and dL/dhead -- are computed in float64 from those
    masks, the raw head and the raw target rows, by torch double autograd of the loss the sums compose:
        L = grad_scale * ((s0 + s1 + s2 + s3) / n_obj + s4 / n_obj + 100 * s5 / n_noobj + s6 / (n_obj * C)).
`loss_reference(..., dtype=torch.float32)` is the float32 twin of the same computation, with the target values in the kernel's
float32 operation order and the sums added in the kernel's documented fixed tree.  Its only use is to measure E, how far float32
arithmetic sits from float64 (`margins`); the device bar is 4 E floored at 2^-22 of the element's scale (`bar`).

The dropped-row rule (`filter_dropped`): the kernels skip a target row whose image index, class or cell lies outside the tensor,
where the reference would raise.  The tests run the kernel on the full list and this reference on the filtered list.
"""
import dataclasses
import functools

import numpy as np
import torch
import torch.nn.functional as F

from oracle import boxes_oracle as bo
from oracle.darknet_oracle import giou_cxcywh

F32 = np.float32
ANCHORS = [(10, 13), (16, 30), (33, 23)]
EDGE_ANCHORS = [(16, 16), (16, 16), (32, 16), (8, 8)]      # (2,2), (2,2), (4,2), (1,1) grid units at stride 8
LOSS_WGS, WG = 1024, 256                                   # launch of yolo_loss_pass: at most 1024 workgroups of 256
FLOOR = 2.0 ** -22
SLOT_NAMES = ["sx", "sy", "sw", "sh", "conf_obj", "conf_noobj", "cls", "n_obj", "n_noobj", "cls_acc", "conf_obj_sum",
              "conf_noobj_sum", "conf50", "iou50_det", "iou75_det"]
COUNT_SLOTS = (7, 8, 9, 12, 13, 14)
VALUE_SLOTS = (0, 1, 2, 3, 4, 5, 6, 10, 11)
GRAD_CLASSES = ["xy", "wh", "conf_obj", "cls", "conf_noobj"]      # ids 1..5 in Ref.cls_id; 0 = must be exactly 0.0
CONF_KEEPOUT = 2.0 ** -9


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    B: int
    A: int
    C: int
    G: int
    anchors: list          # pixels
    head: np.ndarray       # [B, A*(5+C), G, G] float32
    targets: np.ndarray    # [n, 6] float32 (image, class, cx, cy, w, h), coordinates as fractions of the image
    ignore_thres: float = 0.5
    planted: tuple = ()    # saturated: (b, a, channel, gj, gi) of every planted logit

    @property
    def img_dim(self):
        return 8 * self.G

    @property
    def cells(self):
        return self.B * self.A * self.G * self.G

    @property
    def workgroups(self):
        return min((self.cells + WG - 1) // WG, LOSS_WGS)


def filter_dropped(targets, B, C, G):
    """the rows the kernels keep (yolo_targets_pass1): image index in [0, B), class in [0, C), cell in [0, G) on both axes, all
    in the kernel's float32 arithmetic (truncation like .long(); a negative cell index wraps once, like PyTorch indexing)"""
    t = np.asarray(targets, F32).reshape(-1, 6)
    b, label = np.trunc(t[:, 0]).astype(np.int64), np.trunc(t[:, 1]).astype(np.int64)
    gi = np.trunc(t[:, 2] * F32(G)).astype(np.int64)
    gj = np.trunc(t[:, 3] * F32(G)).astype(np.int64)
    gi = np.where(gi < 0, gi + G, gi)
    gj = np.where(gj < 0, gj + G, gj)
    keep = (b >= 0) & (b < B) & (label >= 0) & (label < C) & (gi >= 0) & (gi < G) & (gj >= 0) & (gj < G)
    return t[keep]


# ------------------------------------------------------------------------------------------------------------ assignment (float32)
@dataclasses.dataclass(eq=False)
class Assignment:
    tg: np.ndarray          # the filtered rows
    sa: np.ndarray          # anchors in grid units [A, 2] float32
    bt: tuple               # boxes_oracle.build_targets' 10-tuple
    win: np.ndarray         # [B, A, G, G] row of `tg` that owns each object cell, -1 elsewhere
    ious: np.ndarray        # [A, n] wh_iou of every anchor with every row
    conf: np.ndarray        # float32 sigmoid of the conf channel [B, A, G, G]
    cls: np.ndarray         # float32 sigmoid of the class channels [B, A, G, G, C]
    boxes: np.ndarray       # decoded boxes [B, A, G, G, 4], grid units

    obj = property(lambda s: s.bt[2])
    noobj = property(lambda s: s.bt[3])
    tcls = property(lambda s: s.bt[8])
    class_mask = property(lambda s: s.bt[1])
    iou_scores = property(lambda s: s.bt[0])


def winners(tg, sa, B, A, G):
    """last-writer row index per (image, best anchor, cell), with the oracle's own wh_iou, argmax and truncation"""
    n = tg.shape[0]
    gwh = tg[:, 4:6] * F32(G)
    ious = np.stack([bo.bbox_wh_iou(a, gwh) for a in sa]) if n else np.zeros((A, 0), F32)
    best = ious.argmax(0) if n else np.zeros(0, np.int64)
    b = tg[:, 0].astype(np.int64)
    gi, gj = (tg[:, 2] * F32(G)).astype(np.int64), (tg[:, 3] * F32(G)).astype(np.int64)
    win = np.full((B, A, G, G), -1, np.int64)
    win[b, best, gj, gi] = np.arange(n)
    return win, ious


def build_targets(boxes, cls, tg, sa, thres):
    """boxes_oracle.build_targets; an empty list gives the empty assignment (the oracle indexes with the rows)"""
    if tg.shape[0]:
        return tuple(np.ascontiguousarray(v) for v in bo.build_targets(boxes, cls, tg, sa, thres))
    B, A, G = boxes.shape[:3]
    z = lambda *s: np.zeros((B, A, G, G) + s, F32)
    return (z(), z(), np.zeros((B, A, G, G), bool), np.ones((B, A, G, G), bool), z(), z(), z(), z(), z(cls.shape[-1]), z())


def assign(case, ignore_thres=None, mutant=None, targets=None):
    """the float32 assignment of `case`.  mutant: None, or one of the deliberate errors that tests/test_yolo_loss_cpu.py shows the
    cases can tell from the truth: "ge_thres", "first_writer", "last_max_anchor", "one_hot"."""
    thres = case.ignore_thres if ignore_thres is None else ignore_thres
    tg = filter_dropped(case.targets if targets is None else targets, case.B, case.C, case.G)
    with np.errstate(over="ignore"):        # exp(104) of a planted logit is inf, and 1 / (1 + inf) the 0.0 it stands for
        _, boxes, aux = bo.decode(case.head, case.anchors, case.C, case.img_dim)
    sa, cls = np.asarray(aux["scaled_anchors"], F32), aux["cls"]
    n = tg.shape[0]
    if mutant == "first_writer":            # the last writer of the reversed list is the first of the list
        bt = build_targets(boxes, cls, tg[::-1], sa, thres)
        win, ious = winners(tg[::-1], sa, case.B, case.A, case.G)
        win, ious = np.where(win >= 0, n - 1 - win, -1), ious[:, ::-1]
    elif mutant == "last_max_anchor":       # the first maximum over the reversed anchors is the last over the anchors
        bt = tuple(np.ascontiguousarray(v[:, ::-1]) for v in build_targets(boxes[:, ::-1], cls[:, ::-1], tg, sa[::-1], thres))
        win, ious = winners(tg, sa[::-1], case.B, case.A, case.G)
        win, ious = np.ascontiguousarray(win[:, ::-1]), ious[::-1]
    else:
        bt = build_targets(boxes, cls, tg, sa, thres)
        win, ious = winners(tg, sa, case.B, case.A, case.G)
    if mutant == "ge_thres":
        noobj = bt[3].copy()
        b, gi, gj = tg[:, 0].astype(np.int64), (tg[:, 2] * F32(case.G)).astype(np.int64), (tg[:, 3] * F32(case.G)).astype(np.int64)
        for i in range(n):
            noobj[b[i], ious[:, i] >= F32(thres), gj[i], gi[i]] = False
        bt = bt[:3] + (noobj,) + bt[4:]
    if mutant == "one_hot":
        tcls = np.zeros_like(bt[8])
        idx = np.nonzero(bt[2])
        tcls[idx + (tg[win[idx], 1].astype(np.int64),)] = 1
        bt = bt[:8] + (tcls,) + bt[9:]
    assert np.array_equal(win >= 0, bt[2])
    return Assignment(tg, sa, bt, win, ious, aux["conf"], cls, boxes)


def decision_margins(case, asg):
    """distance of every float32 decision of the assignment and the integer metrics from its threshold"""
    inf = float("inf")
    thr = float(F32(case.ignore_thres))
    d = np.abs(asg.ious.astype(np.float64) - thr)
    obj = asg.obj
    iou = asg.iou_scores[obj].astype(np.float64)
    out = dict(wh_iou=float(d.min()) if d.size else inf,
               wh_iou_off_thres=float(d[asg.ious != F32(case.ignore_thres)].min()) if (asg.ious != F32(case.ignore_thres)).any() else inf,
               conf=float(np.abs(asg.conf.astype(np.float64) - 0.5).min()),
               iou=float(np.minimum(np.abs(iou - 0.5), np.abs(iou - 0.75)).min()) if iou.size else inf, cls_top2=inf)
    # the best-anchor argmax: gap between a target's two largest wh_iou (bit-equal values are the ties `edges` is about)
    out["anchor_gap"] = out["anchor_gap_off_tie"] = inf
    if case.A > 1 and asg.ious.size:
        two = np.sort(asg.ious.astype(np.float64), 0)[-2:]
        gap = two[1] - two[0]
        out["anchor_gap"] = float(gap.min())
        out["anchor_gap_off_tie"] = float(gap[gap > 0].min()) if (gap > 0).any() else inf
    if case.C > 1 and obj.any():
        top = np.sort(asg.cls[obj].astype(np.float64), -1)
        out["cls_top2"] = float((top[:, -1] - top[:, -2]).min())
    return out


# ------------------------------------------------------------------------------------------------- values (float64, float32 twin)
def kernel_tree_sum(dense):
    """float32 sum of one value per cell in the fixed order the kernel documents: each thread adds its cells sweep by sweep, a
    butterfly over the 64 lanes of a wave, (w0 + w1) + (w2 + w3) per workgroup, then yolo_loss_reduce's 16 chunks of
    ceil(n / 16) rows in row order and the 16 chunk sums in chunk order"""
    x = np.asarray(dense, F32).reshape(-1)
    gr = min((x.size + WG - 1) // WG, LOSS_WGS)
    T = gr * WG
    sweeps = (x.size + T - 1) // T
    x = np.concatenate([x, np.zeros(sweeps * T - x.size, F32)]).reshape(sweeps, T)
    loc = np.zeros(T, F32)
    for s in range(sweeps):
        loc = loc + x[s]
    v = loc.reshape(gr, 4, 64)
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, :, lane ^ off]
    w = v[:, :, 0]
    part = (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    per = (gr + 15) // 16
    part = np.concatenate([part, np.zeros(16 * per - gr, F32)]).reshape(16, per)
    chunk = np.zeros(16, F32)
    for r in range(per):
        chunk = chunk + part[:, r]
    t = F32(0)
    for j in range(16):
        t = F32(t + chunk[j])
    return float(t)


@dataclasses.dataclass(eq=False)
class Ref:
    sums: np.ndarray        # [15] float64 values of the sums in this precision
    abs_sums: np.ndarray    # [15] sum of |term| (the scale of a sum)
    dhead: np.ndarray       # [B, A*(5+C), G, G]
    cls_id: np.ndarray      # [B, A, 5+C, G, G] int8: element class of every gradient element (GRAD_CLASSES, 0 = exact zero)
    scale: np.ndarray       # [B, A, 5+C, G, G] float64 class scale of every gradient element
    loss: float


def loss_reference(case, asg, box_loss="mse", dtype=torch.float64, grad_scale=1.0, noobj_factor=100.0):
    B, A, Cc, G = case.B, case.A, case.C, case.G
    K = 5 + Cc
    f32 = dtype == torch.float32
    npdt = np.float32 if f32 else np.float64
    h = torch.from_numpy(case.head).to(dtype).requires_grad_(True)
    p = h.view(B, A, K, G, G).permute(0, 1, 3, 4, 2)
    obj, noobj = torch.from_numpy(asg.obj), torch.from_numpy(asg.noobj)
    n_obj, n_noobj = int(asg.obj.sum()), int(asg.noobj.sum())
    conf = torch.sigmoid(p[..., 4])
    dense = {k: torch.zeros(B, A, G, G, dtype=dtype) for k in VALUE_SLOTS}
    loss = torch.zeros((), dtype=dtype)
    ob, oa, oj, oi = np.nonzero(asg.obj)
    rows = asg.tg[asg.win[ob, oa, oj, oi]]
    tw32 = asg.bt[6][asg.obj]
    if n_obj:
        sx, sy, pw, ph = torch.sigmoid(p[..., 0][obj]), torch.sigmoid(p[..., 1][obj]), p[..., 2][obj], p[..., 3][obj]
        cls = torch.sigmoid(p[..., 5:][obj])
        aw, ah = torch.from_numpy(asg.sa[oa, 0]).to(dtype), torch.from_numpy(asg.sa[oa, 1]).to(dtype)
        gi, gj = torch.from_numpy(oi).to(dtype), torch.from_numpy(oj).to(dtype)
        if f32:   # the kernel's order: gx = r * G rounded to float32, tx = gx - floor(gx), tw = logf(gw / aw + 1e-16f)
            g = torch.from_numpy(rows[:, 2:6] * F32(G))
            tx, ty, tw, th = (torch.from_numpy(asg.bt[k][asg.obj]) for k in (4, 5, 6, 7))
        else:     # the cell is the float32 decision; the offset in it is exact
            g = torch.from_numpy(rows[:, 2:6].astype(np.float64) * G)
            tx, ty = g[:, 0] - gi, g[:, 1] - gj
            tw, th = torch.log(g[:, 2] / aw + 1e-16), torch.log(g[:, 3] / ah + 1e-16)
        if box_loss == "giou":
            pb = torch.stack((sx + gi, sy + gj, torch.exp(pw) * aw, torch.exp(ph) * ah), 1)
            box = [1.0 - giou_cxcywh(pb, g)]
        else:
            box = [(sx - tx) ** 2, (sy - ty) ** 2, (pw - tw) ** 2, (ph - th) ** 2]
        t4 = F.binary_cross_entropy(conf[obj], torch.ones(n_obj, dtype=dtype), reduction="none")
        t6 = F.binary_cross_entropy(cls, torch.from_numpy(asg.tcls[asg.obj]).to(dtype), reduction="none")
        loss = loss + (sum(t.sum() for t in box) + t4.sum()) / n_obj + t6.sum() / (n_obj * Cc)
        t6c = t6.detach()
        t6s = torch.zeros(n_obj, dtype=dtype)
        for k in range(Cc):     # one thread adds a cell's class terms in class order
            t6s = t6s + t6c[:, k]
        for k, t in list(enumerate(box)) + [(4, t4), (6, t6s), (10, conf[obj])]:
            dense[k][obj] = t.detach()
    if n_noobj:
        t5 = F.binary_cross_entropy(conf[noobj], torch.zeros(n_noobj, dtype=dtype), reduction="none")
        loss = loss + noobj_factor * t5.sum() / n_noobj
        dense[5][noobj] = t5.detach()
        dense[11][noobj] = conf[noobj].detach()
    loss = loss * grad_scale
    if n_obj or n_noobj:
        loss.backward()
        dhead = h.grad.numpy()
    else:
        dhead = np.zeros(case.head.shape, npdt)
    sums, abs_sums = np.zeros(15), np.zeros(15)
    for k in VALUE_SLOTS:
        d = dense[k].numpy()
        sums[k] = kernel_tree_sum(d) if f32 else float(d.sum(dtype=np.float64))
        abs_sums[k] = float(np.abs(d).sum(dtype=np.float64))
    conf50 = asg.conf > F32(0.5)
    det = conf50[asg.obj] * (asg.class_mask[asg.obj] > 0)
    sums[7], sums[8], sums[9] = n_obj, n_noobj, float(asg.class_mask[asg.obj].sum())
    sums[12] = float(conf50.sum())
    sums[13] = float(((asg.iou_scores[asg.obj] > F32(0.5)) & det).sum())
    sums[14] = float(((asg.iou_scores[asg.obj] > F32(0.75)) & det).sum())
    # element classes and their scales
    cls_id = np.zeros((B, A, K, G, G), np.int8)
    scale = np.zeros((B, A, K, G, G), np.float64)
    s_obj = grad_scale / max(n_obj, 1)
    cls_id[:, :, 4][asg.noobj] = 5
    scale[:, :, 4][asg.noobj] = grad_scale * 100.0 / max(n_noobj, 1)
    if n_obj:
        cls_id[ob, oa, 0, oj, oi] = cls_id[ob, oa, 1, oj, oi] = 1
        cls_id[ob, oa, 2, oj, oi] = cls_id[ob, oa, 3, oj, oi] = 2
        cls_id[ob, oa, 4, oj, oi] = 3
        scale[ob, oa, 0, oj, oi] = scale[ob, oa, 1, oj, oi] = scale[ob, oa, 4, oj, oi] = s_obj
        hv = case.head.reshape(B, A, K, G, G).astype(np.float64)
        th32 = asg.bt[7][asg.obj]
        scale[ob, oa, 2, oj, oi] = s_obj * np.maximum(1.0, np.abs(hv[ob, oa, 2, oj, oi]) + np.abs(tw32))
        scale[ob, oa, 3, oj, oi] = s_obj * np.maximum(1.0, np.abs(hv[ob, oa, 3, oj, oi]) + np.abs(th32))
        for k in range(Cc):
            cls_id[ob, oa, 5 + k, oj, oi] = 4
            scale[ob, oa, 5 + k, oj, oi] = s_obj
    return Ref(sums, abs_sums, dhead, cls_id, scale, float(loss.detach()))


def grad_errors(got, ref):
    """largest |got - ref.dhead| / scale per element class, and the count of non-zero elements where the class is 0"""
    d = np.abs(np.asarray(got, np.float64).reshape(ref.cls_id.shape) - ref.dhead.astype(np.float64).reshape(ref.cls_id.shape))
    out = {}
    for i, n in enumerate(GRAD_CLASSES, 1):
        m = ref.cls_id == i
        out[n] = float((d[m] / ref.scale[m]).max()) if m.any() else 0.0
    stray = int(np.count_nonzero(np.asarray(got).reshape(ref.cls_id.shape)[ref.cls_id == 0]))
    return out, stray


def sum_errors(got, ref):
    """|got - ref.sums| / sum |term| for the nine loss and metric sums"""
    return {SLOT_NAMES[k]: (abs(float(got[k]) - ref.sums[k]) / ref.abs_sums[k] if ref.abs_sums[k] else abs(float(got[k]) - ref.sums[k]))
            for k in VALUE_SLOTS}


def bar(E):
    """the device bar for one class: 4 E (a few ulp of expf / logf either way, the kernel's own summation tree), floored at 2^-22"""
    return max(4.0 * E, FLOOR)


@functools.lru_cache(maxsize=None)
def reference(name, box_loss="mse", ignore_thres=None):
    """(case, assignment, float64 reference, E per gradient class, E per sum) -- computed once per process and shared"""
    c = case(name)
    asg = assign(c, ignore_thres)
    if name == "saturated":
        # float64 has no saturation: the semantics under test is float32 autograd's (the twin), and E is that of the same head
        # before planting, where float32 and float64 mean the same thing
        plain = unplanted(c)
        pa = assign(plain)
        r64, r32 = loss_reference(plain, pa, box_loss), loss_reference(plain, pa, box_loss, torch.float32)
        ref = loss_reference(c, asg, box_loss, torch.float32)
    else:
        r64, r32 = loss_reference(c, asg, box_loss), loss_reference(c, asg, box_loss, torch.float32)
        ref = r64
    Eg, stray = grad_errors(r32.dhead, r64)
    assert stray == 0
    return c, asg, ref, Eg, sum_errors(r32.sums, r64)


# ------------------------------------------------------------------------------------------------------------------- case builders
def _head(rng, B, A, Cc, G):
    """normal(0, 1); w/h logits clipped to +-8; conf logits kept CONF_KEEPOUT away from 0 (sign kept) so that `conf > 0.5` is the
    same decision in every arithmetic -- a seed cannot do that: 295 000 normal draws put about 90 inside |x| < 4e-4"""
    h = rng.normal(0, 1, (B, A, 5 + Cc, G, G)).astype(F32)
    h[:, :, 2:4] = np.clip(h[:, :, 2:4], -8, 8)
    c = h[:, :, 4]
    h[:, :, 4] = np.where(np.abs(c) < CONF_KEEPOUT, np.copysign(F32(CONF_KEEPOUT), c), c)
    return h.reshape(B, A * (5 + Cc), G, G)


def _targets(rng, n, B, A, Cc, G, anchors):
    """n rows: wh around every anchor in turn; the last tenth shares a cell with an earlier row, with another class, and half of
    those the anchor too (same (image, anchor, cell): last writer wins, classes accumulate)"""
    t = np.zeros((n, 6), np.float64)
    t[:, 0] = rng.integers(0, B, n)
    t[:, 1] = rng.integers(0, Cc, n)
    t[:, 2:4] = (rng.integers(0, G, (n, 2)) + rng.uniform(0.05, 0.95, (n, 2))) / G
    a = np.arange(n) % A
    an = np.asarray(anchors, np.float64)[a] / (8.0 * G)
    t[:, 4:6] = an * np.exp(rng.uniform(-0.3, 0.3, (n, 2)))
    nd = n // 10
    for i in range(n - nd, n):
        j = int(rng.integers(0, n - nd))
        cell = np.floor(t[j, 2:4] * G)
        t[i, 0] = t[j, 0]
        t[i, 1] = (t[j, 1] + 1) % Cc
        t[i, 2:4] = (cell + rng.uniform(0.05, 0.95, 2)) / G
        if i % 2:
            t[i, 4:6] = t[j, 4:6] * np.exp(rng.uniform(-0.02, 0.02, 2))
    return t.astype(F32)


#            name        B  A  C  G    targets seed
_RANDOM = {"stride":     (6, 3, 2, 128, 700, 11),
           "cap_ragged": (1, 3, 1, 295, 300, 12),
           "parts17":    (1, 3, 3, 38, 40, 13),
           "parts16":    (1, 3, 3, 36, 40, 14),
           "parts33":    (1, 3, 2, 53, 60, 25),
           "one_wg":     (1, 1, 1, 13, 12, 16),
           "saturated":  (2, 3, 3, 16, 24, 17),
           "empty":      (2, 3, 2, 16, 0, 18)}
CASES = list(_RANDOM)[:6] + ["edges", "saturated", "empty"]
EDGE_CELL = (0, 2, 11, 10)      # (image, anchor, gj, gi) of the 64 targets in one cell
PLANTED = (30.0, -30.0, 104.0, -104.0)


def edges_targets(dropped=True):
    """the hand-written list of `edges` (B=2, A=4, C=3, G=16), in grid units / 16"""
    G = 16.0
    r = [[0, 0, 3.3 / G, 4.6 / G, 2 / G, 2 / G],             # 2x2: anchors 0 and 1 tie bit for bit (wh_iou 1.0), anchor 0 wins
         [0, 1, 8.5 / G, 2.5 / G, 2 / G, 1 / G],             # 2x1: wh_iou exactly 0.5 against anchors 0, 1 (and 3)
         [1, 2, 5 / G, 7.4 / G, 1.1 / G, 0.9 / G],           # cx = k/G: tx = 0
         [1, 0, 0.0, 3.3 / G, 1.1 / G, 0.9 / G],             # cx = 0
         [1, 1, 1 - 2.0 ** -10, 9.7 / G, 1.1 / G, 0.9 / G],  # cx = 1 - 2^-10: gi = G - 1
         [0, 2, 6.4 / G, 9 / G, 0.9 / G, 1.2 / G],           # the same three for cy
         [0, 0, 13.3 / G, 0.0, 0.9 / G, 1.2 / G],
         [0, 1, 1.7 / G, 1 - 2.0 ** -10, 0.9 / G, 1.2 / G]]
    if dropped:
        r.append([2, 0, 3.3 / G, 4.6 / G, 1 / G, 1 / G])     # image index = B
    b, a, gj, gi = EDGE_CELL
    for i in range(64):                                       # 64 rows in one (image, anchor, cell), cycling through the classes
        r.append([b, i % 3, (gi + (i + 1) / 66.0) / G, (gj + (64 - i) / 66.0) / G, (3.6 + i / 100.0) / G, (1.9 + i / 200.0) / G])
    if dropped:
        r.append([b, 3, (gi + 0.5) / G, (gj + 0.5) / G, 4 / G, 2 / G])   # class = C, aimed at that cell, after its last row
        r.append([1, 1, 1.0, 6.5 / G, 1 / G, 1 / G])          # cx = 1.0
        r.append([1, 1, 6.5 / G, 1.0, 1 / G, 1 / G])          # cy = 1.0
    r.append([1, 0, 12.5 / G, 12.5 / G, 3.8 / G, 2.1 / G])    # two targets, one cell, best anchors 2 and 3: two object cells
    r.append([1, 2, 12.2 / G, 12.7 / G, 1.05 / G, 0.95 / G])
    return np.asarray(r, F32)


def unplanted(c):
    """`saturated` before its logits were planted"""
    h = c.head.copy().reshape(c.B, c.A, 5 + c.C, c.G, c.G)
    h0 = _head(np.random.Generator(np.random.PCG64(_RANDOM[c.name][5] + 1000)), c.B, c.A, c.C, c.G).reshape(h.shape)
    for idx in c.planted:
        h[idx] = h0[idx]
    return dataclasses.replace(c, head=h.reshape(c.head.shape), planted=())


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "edges":
        rng = np.random.Generator(np.random.PCG64(1019))
        return Case(name, 2, 4, 3, 16, EDGE_ANCHORS, _head(rng, 2, 4, 3, 16), edges_targets())
    B, A, Cc, G, n, seed = _RANDOM[name]
    anchors = ANCHORS[:A] if A > 1 else [ANCHORS[1]]
    c = Case(name, B, A, Cc, G, anchors, _head(np.random.Generator(np.random.PCG64(seed + 1000)), B, A, Cc, G),
             _targets(np.random.Generator(np.random.PCG64(seed)), n, B, A, Cc, G, anchors))
    if name == "saturated":
        # +-30 and +-104 in the conf channel of four object and four no-object cells, and in two class channels (v and -v, so both
        # target values meet both signs) of four more object cells
        asg = assign(c)
        h = c.head.copy().reshape(B, A, 5 + Cc, G, G)
        o, no = np.argwhere(asg.obj), np.argwhere(asg.noobj)
        planted = []
        for i, v in enumerate(PLANTED):
            for (b, a, gj, gi), ch, val in ((o[i], 4, v), (no[97 * (i + 1)], 4, v), (o[4 + i], 5, v), (o[4 + i], 6, -v)):
                h[b, a, ch, gj, gi] = val
                planted.append((int(b), int(a), ch, int(gj), int(gi)))
        c = dataclasses.replace(c, head=h.reshape(c.head.shape), planted=tuple(planted))
    return c
