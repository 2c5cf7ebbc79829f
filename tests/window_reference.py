"""THE WINDOW RULE (include/amyloid_yolo.h) restated in NumPy fp32: THE AUGMENTATION RULE with another step 4.
TEST INFRASTRUCTURE ONLY -- the product never imports this.

Only ``warp`` is restated; the record form, the dropout hash and steps 5-8 are ``tests/augment_reference.py``'s, by import.  The
kernel (``ay_augment_ingest_window_u8``) has to match bit for bit."""
import numpy as np

from augment_reference import F, drop_hash, from_row, photometry  # noqa: F401  (re-exported for the tests)


def from_window_row(row):
    """the dict form of one row of a structured ay_aug_window_params array: the embedded record plus the window fields"""
    rec = from_row(row["aug"])
    rec.update(x0=int(row["x0"]), y0=int(row["y0"]), context=int(row["context"]), fill=F(row["fill"]))
    return rec


def warp(block_u8, S, rec, taps=None):
    """steps 1-4 under the window rule: block uint8 [bh,bw,3] (bh or bw may be 0), the window rec["h"] x rec["w"] at block pixel
    (rec["x0"], rec["y0"]) -> W float32 [3,S,S] in 0..255.  ``taps`` (a list) receives (min ty, min tx, max ty, max tx) over all
    four taps of all pixels, in window coordinates."""
    blk = np.asarray(block_u8)
    bh, bw = blk.shape[:2]
    if bh == 0 or bw == 0:
        bh = bw = 0
    h, w = rec["h"], rec["w"]
    D = max(h, w)
    top = (w - h) // 2 if h <= w else 0
    left = (h - w) // 2 if h > w else 0
    scale = F(D) / F(S)
    q = np.minimum(np.floor(np.arange(S, dtype=np.int32).astype(F) * scale).astype(np.int64), D - 1)
    qx, qy = np.meshgrid(q - left, q - top)          # [S(y), S(x)]
    if rec["flip"]:
        qx = w - 1 - qx
    cx, cy = F(w - 1) / F(2), F(h - 1) / F(2)
    xc, yc = qx.astype(F) - cx, qy.astype(F) - cy
    i = rec["inv"].astype(F)
    sx = ((i[0] * xc + i[1] * yc) + i[2]) + cx
    sy = ((i[3] * xc + i[4] * yc) + i[5]) + cy
    x0f, y0f = np.floor(sx), np.floor(sy)
    fx, fy = sx - x0f, sy - y0f
    tx = np.clip(x0f, F(-1e10), F(1e10)).astype(np.int64)    # window coordinates, any distance (no int32 sum below)
    ty = np.clip(y0f, F(-1e10), F(1e10)).astype(np.int64)
    if taps is not None:
        taps.append((int(ty.min()), int(tx.min()), int(ty.max()) + 1, int(tx.max()) + 1))
    pad = np.zeros((max(bh, 1), max(bw, 1), 3), np.uint8)
    pad[:bh, :bw] = blk[:bh, :bw]
    ctx, fill = bool(rec["context"]), F(rec["fill"])

    def tap(yy, xx):
        in_window = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        by, bx = yy + rec["y0"], xx + rec["x0"]
        in_block = (by >= 0) & (by < bh) & (bx >= 0) & (bx < bw)
        v = pad[np.clip(by, 0, max(bh - 1, 0)), np.clip(bx, 0, max(bw - 1, 0))].astype(F)      # [S,S,3]
        v = np.where(in_block[..., None], v, fill)
        return v if ctx else np.where(in_window[..., None], v, F(0))

    a, b, c, d = tap(ty, tx), tap(ty, tx + 1), tap(ty + 1, tx), tap(ty + 1, tx + 1)
    fx, fy = fx[..., None], fy[..., None]
    t = a + fx * (b - a)
    u = c + fx * (d - c)
    W = t + fy * (u - t)
    assert W.dtype == F
    return np.ascontiguousarray(W.transpose(2, 0, 1))


def augment(block_u8, S, rec, taps=None):
    """the whole window rule for one image: the block uint8 [bh,bw,3] -> float32 [3,S,S]"""
    return photometry(warp(block_u8, S, rec, taps), rec)


def padding(S, rec):
    """what a record that reads nothing gives: W = 0 through steps 5-8"""
    return photometry(np.zeros((3, S, S), F), rec)
