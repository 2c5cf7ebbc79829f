"""THE AUGMENTATION RULE (include/amyloid_yolo.h) restated in NumPy fp32, for the image and for the labels.
TEST INFRASTRUCTURE ONLY -- the product never imports this.

Every array operation below is one IEEE fp32 operation per element, in the order the rule writes them, so the kernel
(``ay_augment_ingest_u8``, built with -ffp-contract=off) has to match bit for bit.  imgaug is not installed: parity with the
reference's pipeline is unpinned, this file is the yardstick."""
import numpy as np

F = np.float32


def record(h, w, inv=(1, 0, 0, 0, 1, 0), flip=0, sharpen_alpha=0.0, drop_threshold=0, drop_seed=0,
           color=(1, 0, 0, 0, 1, 0, 0, 0, 1), bright=0.0):
    """a parameter record as a plain dict (the identity unless told otherwise)"""
    return dict(h=int(h), w=int(w), inv=np.asarray(inv, F), flip=int(flip), sharpen_alpha=F(sharpen_alpha),
                drop_threshold=int(drop_threshold), drop_seed=int(drop_seed), color=np.asarray(color, F), bright=F(bright))


def from_row(row):
    """the dict form of one row of a structured ay_aug_params array"""
    return record(row["h"], row["w"], row["inv"], row["flip"], row["sharpen_alpha"], row["drop_threshold"], row["drop_seed"],
                  row["color"], row["bright"])


def warp(img_u8, S, rec):
    """steps 1-4: uint8 [h,w,3] -> W float32 [3,S,S] in 0..255"""
    img = np.asarray(img_u8)
    h, w = img.shape[:2]
    assert (h, w) == (rec["h"], rec["w"])
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
    x0 = np.clip(x0f, -2, w).astype(np.int64)        # further out than one pixel: no tap inside either way
    y0 = np.clip(y0f, -2, h).astype(np.int64)

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(F)      # [S,S,3]
        return np.where(ok[..., None], v, F(0))

    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    fx, fy = fx[..., None], fy[..., None]
    t = a + fx * (b - a)
    u = c + fx * (d - c)
    W = t + fy * (u - t)
    assert W.dtype == F
    return np.ascontiguousarray(W.transpose(2, 0, 1))


def drop_hash(S, seed):
    """step 6's hash of every pixel, uint32 [S,S]"""
    with np.errstate(over="ignore"):
        idx = np.arange(S * S, dtype=np.uint32).reshape(S, S)
        hsh = np.uint32(seed) ^ (idx * np.uint32(0x9E3779B9))
        hsh = hsh ^ (hsh >> np.uint32(16))
        hsh = hsh * np.uint32(0x7FEB352D)
        hsh = hsh ^ (hsh >> np.uint32(15))
        hsh = hsh * np.uint32(0x846CA68B)
        hsh = hsh ^ (hsh >> np.uint32(16))
    assert hsh.dtype == np.uint32
    return hsh


def photometry(W, rec):
    """steps 5-8 on W [3,S,S] -> float32 [3,S,S] in 0..1"""
    S = W.shape[-1]
    p = np.pad(W, ((0, 0), (1, 1), (1, 1)), mode="edge")          # indices clamped at the edge of the output image
    n = lambda dy, dx: p[:, 1 + dy:1 + dy + S, 1 + dx:1 + dx + S]
    ring = n(-1, -1)
    for dy, dx in ((-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)):
        ring = ring + n(dy, dx)
    v = W + rec["sharpen_alpha"] * (F(8) * W - ring)
    dropped = drop_hash(S, rec["drop_seed"]).astype(np.uint64) < np.uint64(rec["drop_threshold"])
    v = np.where(dropped[None], F(0), v)
    M = rec["color"].astype(F).reshape(3, 3)
    o = np.stack([((M[k, 0] * v[0] + M[k, 1] * v[1]) + M[k, 2] * v[2]) + rec["bright"] for k in range(3)])
    o = np.where(o > 0, o, F(0))
    o = np.where(o < 255, o, F(255))
    out = o / F(255)
    assert out.dtype == F and v.dtype == F and ring.dtype == F
    return out


def augment(img_u8, S, rec):
    """the whole rule for one image: uint8 [h,w,3] -> float32 [3,S,S]"""
    return photometry(warp(img_u8, S, rec), rec)


def labels(boxes, h, w, A, flip):
    """the label rule, corner by corner: boxes [n,5] (class cx cy w h, normalised to the tile) -> [m,5] normalised to the padded
    square, float64.  A [2,3] is the forward matrix about the centre (w/2, h/2) of the continuous image."""
    out = []
    D = max(h, w)
    left = (h - w) // 2 if h > w else 0
    top = (w - h) // 2 if h <= w else 0
    for c, bx, by, bw, bh in np.asarray(boxes, np.float64).reshape(-1, 5):
        xs, ys = [], []
        for px, py in ((bx - bw / 2, by - bh / 2), (bx + bw / 2, by - bh / 2), (bx - bw / 2, by + bh / 2), (bx + bw / 2, by + bh / 2)):
            x, y = px * w - w / 2, py * h - h / 2
            X = A[0][0] * x + A[0][1] * y + A[0][2] + w / 2
            Y = A[1][0] * x + A[1][1] * y + A[1][2] + h / 2
            xs.append(w - X if flip else X)
            ys.append(Y)
        x1, x2 = min(max(min(xs), 0), w), min(max(max(xs), 0), w)
        y1, y2 = min(max(min(ys), 0), h), min(max(max(ys), 0), h)
        if x2 - x1 <= 0 or y2 - y1 <= 0:
            continue
        out.append([c, ((x1 + x2) / 2 + left) / D, ((y1 + y2) / 2 + top) / D, (x2 - x1) / D, (y2 - y1) / D])
    return np.array(out, np.float64).reshape(-1, 5)
