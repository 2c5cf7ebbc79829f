"""THE STAIN RULE of include/amyloid_yolo.h restated in NumPy (TEST INFRASTRUCTURE ONLY): the tables in float64 rounded to fp32 once,
every device operation as one float32 NumPy operation in the order the rule writes it, the host arithmetic in float64 / Python ints.
Nothing here comes from the product.  The cut is the CPU cut of the ingest tests (a 255-padded crop, oracle.ingest_oracle.ingest for
the nearest resize) with the pixel stage swapped: ingest's value byte / 255 is turned back into the byte, which the rule then maps."""
import math

import numpy as np

import tissue_reference as tr
import views_reference as vr
from oracle.ingest_oracle import ingest

F32 = np.float32
BINS = 512
HEMATOXYLIN, DAB = (0.650, 0.704, 0.286), (0.268, 0.570, 0.776)     # Ruifrok & Johnston


def basis(stain0=HEMATOXYLIN, stain1=DAB):
    """M float64 3x3: rows 0, 1 the unit stain vectors, row 2 their normalised cross product"""
    a, b = (np.asarray(v, np.float64) / np.linalg.norm(np.asarray(v, np.float64)) for v in (stain0, stain1))
    c = np.cross(a, b)
    return np.stack([a, b, c / np.linalg.norm(c)])


def tables(gains=(1.0, 1.0), M=None):
    """-> dict of fp32 arrays od [256], D [9], A [9], T [257]"""
    M = basis() if M is None else np.asarray(M, np.float64)
    v = np.arange(256, dtype=np.float64)
    k = np.arange(257, dtype=np.float64)
    Minv = np.linalg.inv(M)
    return {"od": (-np.log10((v + 1.0) / 256.0)).astype(F32),
            "D": Minv.reshape(-1).astype(F32),
            "A": (Minv @ np.diag([gains[0], gains[1], 1.0]) @ M).reshape(-1).astype(F32),
            "T": ((256.0 * 10.0 ** (-k / 64.0) - 1.0) / 255.0).astype(F32)}


def image(raster, shrink):
    """the (halved) image the rule's pixels come from"""
    return tr.halve(raster) if shrink == 2 else np.asarray(raster)


def concentrations(px, params):
    """px uint8 [..., 3] -> fp32 [..., 2]"""
    od, D = params["od"], params["D"]
    o0, o1, o2 = (od[px[..., c]] for c in range(3))
    return np.stack([(o0 * D[s] + o1 * D[3 + s]) + o2 * D[6 + s] for s in (0, 1)], -1)


def bins(c):
    """fp32 concentrations -> bin indices: c < 0 ? 0 : min((int)(c * 64), 511)"""
    c = np.asarray(c, F32)
    safe = np.where((c >= 0) & (c < 8), c, F32(0))                       # (int) of a float beyond the int range is not taken
    return np.where(c < 0, 0, np.where(c < 8, (safe * F32(64)).astype(np.int64), BINS - 1))


def hist(raster, shrink, bg, params):
    """-> int64 [1025]: hist[s * 512 + bin], hist[1024] = tissue pixels"""
    img = image(raster, shrink)
    px = img[img.min(axis=2).astype(np.int32) < int(bg)]
    b = bins(concentrations(px, params))
    out = np.zeros(2 * BINS + 1, np.int64)
    for s in (0, 1):
        out[s * BINS:(s + 1) * BINS] = np.bincount(b[:, s], minlength=BINS)
    out[2 * BINS] = len(px)
    return out


def map_pixels(px, params):
    """px uint8 [..., 3] -> the mapped values fp32 [..., 3]"""
    od, A, T = params["od"], params["A"], params["T"]
    o0, o1, o2 = (od[px[..., c]] for c in range(3))
    out = []
    for c in range(3):
        o = (o0 * A[c] + o1 * A[3 + c]) + o2 * A[6 + c]
        o = np.where(o > 0, o, F32(0))
        o = np.where(o < 4, o, F32(4))
        u = o * F32(64)
        k = np.minimum(u.astype(np.int32), 255)
        f = u - k.astype(F32)
        x = T[k] + f * (T[k + 1] - T[k])
        x = np.where(x > 0, x, F32(0))
        out.append(np.where(x < 1, x, F32(1)))
    out = np.stack(out, -1)
    assert out.dtype == F32
    return out


def to_u8(x):
    """the uint8 form: (uint8)(x * 255.0f + 0.5f)"""
    return (np.asarray(x, F32) * F32(255) + F32(0.5)).astype(np.uint8)


def apply(raster, shrink, params):
    """the (halved) image, mapped, uint8 [H, W, 3]"""
    return to_u8(map_pixels(image(raster, shrink), params))


def exact_map(px, gains, M=None):
    """float64, with the exact exponential: 10^-od' back to a value in 0..1 (for the table's error bound)"""
    M = basis() if M is None else M
    od = -np.log10((np.asarray(px, np.float64) + 1.0) / 256.0)
    o = od @ (np.linalg.inv(M) @ np.diag([gains[0], gains[1], 1.0]) @ M)
    return np.clip((256.0 * 10.0 ** (-np.clip(o, 0.0, 4.0)) - 1.0) / 255.0, 0.0, 1.0)


def strength(h, n, p):
    """h int [2, 512], n tissue pixels -> (q0, q1)"""
    if n == 0:
        raise ValueError("no tissue")
    K = max(1, math.ceil(p * n / 100.0))
    out = []
    for s in (0, 1):
        run = 0
        for b in range(BINS):
            run += int(h[s][b])
            if run >= K:
                break
        out.append((b + 1) / 64.0)
    return tuple(out)


def gains(q, t, max_gain=4.0):
    return tuple(min(max(ts / qs, 1.0 / max_gain), max_gain) for ts, qs in zip(t, q))


def positive_fraction(h, n, stain, thres):
    """-> (share of tissue pixels in bins j .., j / 64), j = round(thres * 64)"""
    j = int(round(thres * 64.0))
    return sum(int(v) for v in h[stain][j:]) / n, j / 64.0


def cut_bytes(raster, shrink, tile, origins, S):
    """uint8 [n, 3, S, S]: the bytes the plain cut divides by 255"""
    img = image(raster, shrink)
    out = []
    for x, y in origins:
        t = np.full((tile, tile, 3), 255, np.uint8)
        c = img[max(y, 0):max(y + tile, 0), max(x, 0):max(x + tile, 0)]
        t[max(-y, 0):max(-y, 0) + c.shape[0], max(-x, 0):max(-x, 0) + c.shape[1]] = c
        v = ingest(t, S).numpy()                       # byte / 255 behind the nearest resize
        b = np.rint(v * F32(255)).astype(np.uint8)
        assert np.array_equal(b.astype(F32) / F32(255), v)
        out.append(b)
    return np.stack(out)


def cut(raster, shrink, tile, origins, views, S, params):
    """fp32 [n * V, 3, S, S], tile-major: tile i in view views[j] is image i * V + j"""
    b = cut_bytes(raster, shrink, tile, origins, S)                        # [n, 3, S, S]
    I0 = np.moveaxis(map_pixels(np.moveaxis(b, 1, -1), params), -1, 1)     # [n, 3, S, S]
    return np.stack([vr.view_image_fast(I0, v) for v in views], 1).reshape(-1, 3, S, S)
