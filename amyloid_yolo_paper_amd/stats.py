"""Detection statistics (reference ``utils/utils.py:69-190``): greedy true-positive matching on the device
(``ay_match_detections``), VOC-style AP per class on the host (a sort and two cumulative sums over the detections).
Slide level: ``match_slide`` / ``slide_statistics`` (``ay_slide_match``) match one image of any size, a whole slide's detections
against its annotations, where the per-tile kernel's 2048 targets per image do not reach."""
import numpy as np
import torch



def get_batch_statistics(outputs, targets, iou_threshold):
    """Reference ``utils/utils.py:154-190``: outputs = list of [n,7] | None (what ``non_max_suppression`` returns), targets
    [nT,6] = (sample, class, x1, y1, x2, y2 in pixels) -> [[true_positives, scores, labels]] per image with detections.
    The greedy matching of the whole batch runs in one device kernel (``ay_match_detections``, one wavefront per image)."""
    import ctypes as C

    from . import _lib
    from ._lib import check, ptr
    from .utils import _to_dev
    B = len(outputs)
    present = [i for i, o in enumerate(outputs) if o is not None]
    if not present:
        return []
    max_det = max(int(outputs[i].shape[0]) for i in present)
    max_det = max(max_det, 1)
    dev = _to_dev(torch.zeros(1)).device
    rows = torch.zeros(B, max_det, 7, device=dev, dtype=torch.float32)
    count = torch.zeros(B, device=dev, dtype=torch.int32)
    for i in present:
        n = int(outputs[i].shape[0])
        rows[i, :n] = outputs[i].detach().to(device=dev, dtype=torch.float32)
        count[i] = n
    tg = torch.as_tensor(targets, dtype=torch.float32).to(dev).contiguous().reshape(-1, 6)
    tp = torch.empty(B, max_det, device=dev, dtype=torch.float32)
    ovf = torch.zeros(1, device=dev, dtype=torch.int32)
    nT = int(tg.shape[0])
    check(_lib.lib().ay_match_detections(ptr(rows), ptr(count), B, max_det, ptr(tg) if nT else None, nT, C.c_float(float(iou_threshold)),
                                         ptr(tp), ptr(ovf), _lib.stream_ptr()), "ay_match_detections")
    tp = tp.cpu().numpy()
    if int(ovf.item()):
        raise _lib.AyError("ay_match_detections: an image has more than 2048 targets")
    batch_metrics = []
    for i in present:
        o = outputs[i].detach().cpu()
        batch_metrics.append([tp[i, : o.shape[0]].astype(np.float64), o[:, 4], o[:, -1]])
    return batch_metrics


def _class_segments(keys):
    """sorted integer keys -> (unique keys, start index of each run, one-past-the-end index of each run)"""
    cut = np.flatnonzero(np.diff(keys)) + 1
    starts = np.concatenate(([0], cut))
    return keys[starts], starts, np.concatenate((cut, [keys.size]))


def average_precision(true_pos, n_truth):
    """Area under the monotone precision envelope of ONE class (the reference's VOC-style ``compute_ap``,
    ``utils/utils.py:126-150``), from the true-positive flags of its detections in descending-confidence order.
    Returns (ap, final precision, final recall).  The curve is walked once from the right: the envelope value at a
    detection is the best precision at or after it, and the area grows by (recall step) x (envelope) wherever the recall
    moves -- i.e. at the true positives -- plus the closing step to recall 1 at precision 0, which adds nothing."""
    hits = np.cumsum(true_pos)
    false_alarms = np.cumsum(1.0 - true_pos)
    precision = hits / (hits + false_alarms)
    recall = hits / (n_truth + 1e-16)
    envelope = np.maximum.accumulate(precision[::-1])[::-1]
    step = np.diff(np.concatenate(([0.0], recall)))
    moved = step != 0
    return float(np.sum(step[moved] * envelope[moved])), float(precision[-1]), float(recall[-1])


def ap_per_class(tp, conf, pred_cls, target_cls):
    """Reference ``utils/utils.py:71-123``: precision, recall, AP, F1 per ground-truth class (and the class ids, int32), from
    the flat per-detection arrays of a whole evaluation.  One stable sort by (class, descending confidence) lays every
    class's detections out as a contiguous run; classes that occur only among the detections are ignored, a
    ground-truth class without detections scores zero."""
    tp = np.asarray(tp, np.float64)
    conf = np.asarray(conf)
    pred_cls = np.asarray(pred_cls)
    truth_ids, truth_counts = np.unique(np.asarray(target_cls), return_counts=True)
    order = np.lexsort((-conf, pred_cls))           # primary key: class, secondary: confidence descending (stable)
    tp, pred_sorted = tp[order], pred_cls[order]
    runs = {}
    if pred_sorted.size:
        ids, lo, hi = _class_segments(pred_sorted)
        runs = {c: (a, b) for c, a, b in zip(ids.tolist(), lo.tolist(), hi.tolist())}
    prec, rec, ap = (np.zeros(truth_ids.size) for _ in range(3))
    for k, (c, n_truth) in enumerate(zip(truth_ids.tolist(), truth_counts.tolist())):
        if c in runs:
            a, b = runs[c]
            ap[k], prec[k], rec[k] = average_precision(tp[a:b], n_truth)
    f1 = 2 * prec * rec / (prec + rec + 1e-16)
    return prec, rec, ap, f1, truth_ids.astype("int32")


# ---- slide level: one image of any size (THE SLIDE MATCH RULE, include/amyloid_yolo.h) ----------------------------------------
def _slide_array(a, cols, dev):
    t = a.detach() if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float32)))
    return t.to(device=dev, dtype=torch.float32).reshape(-1, cols).contiguous()


def match_slide(rows, targets, iou_thres=0.5, roi=None, cell_side=None):
    """True-positive matching of a whole slide's detections against its annotations on the device (``ay_slide_match``): the rule of
    ``get_batch_statistics`` for ONE image of any size, with no cap on the number of targets.

    ``rows`` [M,7] = (x1, y1, x2, y2, conf, cls_conf, cls_pred) and ``targets`` [T,5] = (class, x1, y1, x2, y2), both in slide
    pixels, tensors or arrays on the host or the device; ``iou_thres`` a float or a sequence of K <= 16 values in (0, 1]; ``roi`` =
    (x1, y1, x2, y2): rows and targets whose centre lies outside the closed rectangle are ignored, as if deleted.  Rows need not
    be sorted: they are ranked by ``conf * cls_conf`` (ties: lower index first).  Scores must be >= 0 and not NaN, coordinates
    finite, classes integers in 0 .. 4095 (``AyError`` for a target class outside).

    Returns a dict of device tensors: ``tp`` uint8 [K,M], ``best_iou`` float32 [M], ``best_target`` int32 [M] (-1: no target with a
    positive IoU), ``claim`` int32 [K,T] (the row that claimed the target, -1: missed), ``row_ignored`` / ``target_ignored`` bool,
    ``eligible`` / ``claimed`` int32 [K] (rows that reached threshold k with a label present; targets claimed = true positives),
    ``oversize`` (targets larger than a grid cell, which every row tests).  ``cell_side`` overrides the side of the binning grid
    (default: from the targets); the result does not depend on it.  Synchronises with the host."""
    import ctypes as C

    from . import _lib
    from ._lib import check, ptr
    from .utils import _to_dev
    dev = _to_dev(torch.zeros(1)).device
    rows, targets = _slide_array(rows, 7, dev), _slide_array(targets, 5, dev)
    M, T = int(rows.shape[0]), int(targets.shape[0])
    thr = [float(v) for v in np.atleast_1d(np.asarray(iou_thres, np.float64))]
    K = len(thr)
    thr_c = (C.c_float * max(K, 1))(*thr)
    roi_c = None if roi is None else (C.c_float * 4)(*[float(v) for v in roi])
    tp = torch.zeros(K, M, device=dev, dtype=torch.uint8)
    best_iou = torch.zeros(M, device=dev, dtype=torch.float32)
    best_target = torch.full((M,), -1, device=dev, dtype=torch.int32)
    claim = torch.full((K, T), -1, device=dev, dtype=torch.int32)
    row_ign = torch.zeros(M, device=dev, dtype=torch.uint8)
    tgt_ign = torch.zeros(T, device=dev, dtype=torch.uint8)
    stats = torch.zeros(2 * K + 2, device=dev, dtype=torch.int32)
    L = _lib.lib()
    ws = torch.empty(max(int(L.ay_slide_match_workspace_bytes(M, T, K)), 1), device=dev, dtype=torch.uint8)
    check(L.ay_slide_match(ptr(rows) if M else None, M, ptr(targets) if T else None, T, thr_c, K, roi_c,
                           C.c_float(0.0 if cell_side is None else float(cell_side)), ptr(tp) if M else None, ptr(best_iou) if M else None,
                           ptr(best_target) if M else None, ptr(claim) if T else None, ptr(row_ign) if M else None,
                           ptr(tgt_ign) if T else None, ptr(stats), ptr(ws), ws.numel(), _lib.stream_ptr()), "ay_slide_match")
    st = stats.cpu().numpy()
    if int(st[2 * K]) & _lib.CONSTANTS["AY_SLIDE_FLAG_CLASS"]:
        raise _lib.AyError("ay_slide_match: a target's class is no integer in 0 .. 4095")
    return {"tp": tp, "best_iou": best_iou, "best_target": best_target, "claim": claim, "row_ignored": row_ign.bool(),
            "target_ignored": tgt_ign.bool(), "eligible": torch.from_numpy(st[0:2 * K:2].copy()),
            "claimed": torch.from_numpy(st[1:2 * K:2].copy()), "oversize": int(st[2 * K + 1])}


def slide_statistics(rows, targets, iou_thres=0.5, roi=None, match=None):
    """Precision / recall / AP of a whole slide's detections (``match_slide`` + ``ap_per_class``).

    Arguments as for :func:`match_slide` (``match`` replaces the device call by a function of the same signature that returns at
    least ``tp``, ``claim``, ``row_ignored`` and ``target_ignored``: the tests pass the NumPy restatement).  Returns a dict:
    ``iou_thres`` (the K thresholds); ``metrics``: per threshold ``(precision, recall, AP, f1, ap_class)`` of
    ``ap_per_class(tp, conf, cls_pred, target classes)`` over the non-ignored rows and targets; ``missed``: per threshold the
    indices of the non-ignored targets that no row claimed; ``false_alarms``: per threshold the indices of the non-ignored rows
    that are no true positive; ``counts``: per threshold a dict with ``rows``, ``targets`` (non-ignored), ``tp``, ``missed`` and
    ``false_alarms``.  All indices refer to the arrays as given."""
    m = (match or match_slide)(rows, targets, iou_thres, roi)
    host = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    rows_h, targets_h = host(rows).astype(np.float32).reshape(-1, 7), host(targets).astype(np.float32).reshape(-1, 5)
    tp, claim = host(m["tp"]), host(m["claim"])
    live_r, live_t = ~host(m["row_ignored"]).astype(bool), ~host(m["target_ignored"]).astype(bool)
    thr = [float(v) for v in np.atleast_1d(np.asarray(iou_thres, np.float64))]
    out = {"iou_thres": thr, "metrics": [], "missed": [], "false_alarms": [], "counts": []}
    for k in range(len(thr)):
        out["metrics"].append(ap_per_class(tp[k][live_r], rows_h[live_r, 4], rows_h[live_r, 6], targets_h[live_t, 0]))
        missed = np.flatnonzero(live_t & (claim[k] == -1))
        alarms = np.flatnonzero(live_r & (tp[k] == 0))
        out["missed"].append(missed)
        out["false_alarms"].append(alarms)
        out["counts"].append({"rows": int(live_r.sum()), "targets": int(live_t.sum()), "tp": int(tp[k][live_r].sum()),
                              "missed": int(missed.size), "false_alarms": int(alarms.size)})
    return out
