"""THE VIEW RULE and THE VOTE RULE of include/amyloid_yolo.h restated in NumPy (float32 where the rule says fp32), for the tests of
csrc/ay_views.hip, amyloid_yolo_paper_amd/views.py and wsi.detect_region(views=...).  Plain loops, no cleverness: this file is the
yardstick, not the product."""
import numpy as np

from oracle.boxes_oracle import bbox_iou

F32 = np.float32


def bits(v):
    """view id -> (FX, FY, T)"""
    assert 0 <= int(v) <= 7
    return int(v) & 1, (int(v) >> 1) & 1, (int(v) >> 2) & 1


def source_pixel(v, x, y, S):
    """pixel (x, y) of view v shows pixel (sx, sy) of I0"""
    FX, FY, T = bits(v)
    a, b = (y, x) if T else (x, y)
    return (S - 1 - a if FX else a), (S - 1 - b if FY else b)


def view_image(I0, v):
    """I0 [..., S, S] -> its view v, pixel by pixel from the rule"""
    I0 = np.asarray(I0)
    S = I0.shape[-1]
    assert I0.shape[-2] == S
    out = np.empty_like(I0)
    for y in range(S):
        for x in range(S):
            sx, sy = source_pixel(v, x, y, S)
            out[..., y, x] = I0[..., sy, sx]
    return out


def view_image_fast(I0, v):
    """the same by flips and a transpose (shown equal to view_image in test_views_cpu)"""
    FX, FY, T = bits(v)
    out = np.asarray(I0)
    if FX:
        out = out[..., :, ::-1]
    if FY:
        out = out[..., ::-1, :]
    if T:
        out = np.swapaxes(out, -1, -2)
    return np.ascontiguousarray(out)


def unview_box(v, cx, cy, w, h, S):
    """one decoded box of view v -> the frame of I0, in fp32, one operation each"""
    FX, FY, T = bits(v)
    cx, cy, w, h, Sf = F32(cx), F32(cy), F32(w), F32(h), F32(S)
    a, b = (cy, cx) if T else (cx, cy)
    X = F32(Sf - a) if FX else a
    Y = F32(Sf - b) if FY else b
    W, H = (h, w) if T else (w, h)
    return X, Y, W, H


def unview_rows(pred, views, S):
    """pred [n_images, N, 5+C] float32, image i in view views[i % len(views)] -> a new array with the boxes in the frame of I0"""
    pred = np.asarray(pred, F32)
    out = pred.copy()
    Sf = F32(S)
    for i in range(pred.shape[0]):
        FX, FY, T = bits(views[i % len(views)])
        cx, cy, w, h = (pred[i, :, k] for k in range(4))
        a, b = (cy, cx) if T else (cx, cy)
        out[i, :, 0] = (Sf - a).astype(F32) if FX else a
        out[i, :, 1] = (Sf - b).astype(F32) if FY else b
        out[i, :, 2], out[i, :, 3] = (h, w) if T else (w, h)
    return out


def view_votes(pred, n_views, conf_thres, vote_thres, rows, count):
    """pred [B, n_views * N, 5+C] with CORNERS in columns 0..3, rows [B, max_det, 7], count [B] -> votes int32 [B, max_det]"""
    pred, rows = np.asarray(pred, F32), np.asarray(rows, F32)
    B, R, _ = pred.shape
    N = R // n_views
    assert N * n_views == R
    max_det = rows.shape[1]
    votes = np.zeros((B, max_det), np.int32)
    conf_thres, vote_thres = F32(conf_thres), F32(vote_thres)
    for b in range(B):
        cand = np.flatnonzero(pred[b, :, 4] >= conf_thres)
        cls = pred[b, cand, 5:].argmax(1)               # first maximum
        for d in range(min(max(int(count[b]), 0), max_det)):
            if len(cand) == 0:
                continue
            iou = bbox_iou(rows[b, d, :4][None], pred[b, cand, :4])
            ok = (cls == int(rows[b, d, 6])) & (iou > vote_thres)
            for j in np.unique(cand[ok] // N):
                votes[b, d] |= 1 << int(j)
    return votes


def popcount(v):
    return np.array([bin(int(x) & 0xff).count("1") for x in np.asarray(v).ravel()], np.int64).reshape(np.shape(v))


def view_select(rows, keep, count, votes, min_views):
    """-> new (rows, keep, count): per image the rows (and keep entries) with at least min_views votes, in order, in front; what
    lies behind the new count is left as the in-place compaction leaves it and is NOT part of the contract (compare [:count] only).
    An image with count > max_det keeps its count."""
    rows, count = np.array(rows, F32), np.array(count, np.int32)
    keep = None if keep is None else np.array(keep, np.int32)
    max_det = rows.shape[1]
    for b in range(rows.shape[0]):
        D = min(max(int(count[b]), 0), max_det)
        sel = np.flatnonzero(popcount(votes[b, :D]) >= min_views)
        rows[b, :len(sel)] = rows[b, sel]
        if keep is not None:
            keep[b, :len(sel)] = keep[b, sel]
        if count[b] <= max_det:
            count[b] = len(sel)
    return rows, keep, count
