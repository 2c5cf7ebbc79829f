"""THE BASIS RULE of include/amyloid_yolo.h restated in NumPy and Python integers (TEST INFRASTRUCTURE ONLY): the two device passes as
integer array arithmetic (the floor with np.floor_divide), the host steps in float64 and Python ints, written as plain loops where the
product uses a search.  Nothing here comes from the product.  Also the remix tables of THE STAIN RULE (unmix on one basis, mix on
another) and the synthetic two-stain slide the recovery tests are made on."""
import math

import numpy as np

import stain_reference as sref
from stain_reference import image, map_pixels, to_u8  # noqa: F401  (the pixel stage the remix tests share)

OD_SCALE, OD_MAX, EQ_MAX, DIR_BINS = 1024, 2466, 1024, 512
H_DAB = sref.basis()


def odq():
    """int64 [256]: rint(-log10((v + 1) / 256) * 1024)"""
    v = np.arange(256, dtype=np.float64)
    t = np.rint(-np.log10((v + 1.0) / 256.0) * OD_SCALE).astype(np.int64)
    assert t[255] == 0 and t[0] == OD_MAX
    return t


def beta_q(beta=0.15):
    return int(np.rint(beta * OD_SCALE))


def selected(raster, shrink, bg, bq):
    """-> (tissue pixels, integer OD of the selected pixels int64 [n, 3])"""
    img = image(raster, shrink)
    px = img[img.min(axis=2).astype(np.int32) < int(bg)]
    o = odq()[px]
    return len(px), o[o.min(axis=1) >= bq] if len(px) else np.zeros((0, 3), np.int64)


def moments(raster, shrink, bg, bq):
    """-> int64 [11]: n_tissue, n_sel, S_0..2, P_00, P_01, P_02, P_11, P_12, P_22"""
    n_t, o = selected(raster, shrink, bg, bq)
    out = [n_t, len(o)] + [int(o[:, c].sum()) for c in range(3)]
    out += [int((o[:, c] * o[:, d]).sum()) for c in range(3) for d in range(c, 3)]
    return np.array(out, np.int64)


def plane(m):
    """11 moments -> (eq1, eq2 int32 [3], eigenvalues largest first)"""
    m = [int(v) for v in m]
    n, S, P = m[1], m[2:5], m[5:]
    if n < 2:
        raise ValueError("fewer than two selected pixels")
    pairs = [(c, d) for c in range(3) for d in range(c, 3)]
    cov = np.zeros((3, 3), np.float64)
    for (c, d), p in zip(pairs, P):
        cov[c, d] = cov[d, c] = (n * p - S[c] * S[d]) / (n * (n - 1))
    w, V = np.linalg.eigh(cov)
    if not w[1] > 0:
        raise ValueError("no plane")
    e1, e2 = V[:, 2].copy(), V[:, 1].copy()
    if e1[0] + e1[1] + e1[2] < 0:
        e1 = -e1
    big = 0
    for c in (1, 2):
        if abs(e2[c]) > abs(e2[big]):
            big = c
    if e2[big] < 0:
        e2 = -e2
    return np.rint(1024.0 * e1).astype(np.int32), np.rint(1024.0 * e2).astype(np.int32), (w[2], w[1], w[0])


def direction_bins(o, eq1, eq2):
    """integer OD [n, 3] -> (k of the pixels with p1 > 0, the number of pixels with p1 <= 0)"""
    eq1, eq2 = np.asarray(eq1, np.int64), np.asarray(eq2, np.int64)
    assert np.abs(eq1).max() <= EQ_MAX and np.abs(eq2).max() <= EQ_MAX
    p1, p2 = o @ eq1, o @ eq2
    assert np.abs(256 * p2).max(initial=0) < 2 ** 31
    inside = p1 > 0
    p1, p2 = p1[inside], p2[inside]
    k = np.floor_divide(256 * p2, p1 + np.abs(p2))
    assert k.min(initial=0) >= -256 and k.max(initial=0) <= 255
    return k, int((~inside).sum())


def direction_hist(raster, shrink, bg, bq, eq1, eq2):
    """-> int64 [514]: hist[k + 256], hist[512] = outside, hist[513] = selected pixels"""
    _, o = selected(raster, shrink, bg, bq)
    k, outside = direction_bins(o, eq1, eq2)
    out = np.zeros(DIR_BINS + 2, np.int64)
    out[:DIR_BINS] = np.bincount(k + 256, minlength=DIR_BINS)
    out[DIR_BINS], out[DIR_BINS + 1] = outside, len(o)
    return out


def angle(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return math.degrees(math.acos(min(1.0, max(-1.0, float(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))))))


def half_angle(M=H_DAB):
    return 0.5 * angle(M[0], M[1])


def vectors(hist, eq1, eq2, alpha=1.0, M=H_DAB, max_angle="half"):
    """-> dict: raw [2, 3] (assigned, before the guard), vectors [2, 3], angle_to_prior, fell_back"""
    h = [int(v) for v in np.asarray(hist)[:DIR_BINS]]
    n = sum(h)
    if n == 0:
        raise ValueError("no selected pixel inside")
    q1, q2 = np.asarray(eq1, np.float64), np.asarray(eq2, np.float64)
    ends = []
    for K in (max(1, math.ceil(alpha * n / 100.0)), max(1, math.ceil((100.0 - alpha) * n / 100.0))):
        run = 0
        for b in range(DIR_BINS):
            run += h[b]
            if run >= K:
                break
        d = (b - 256 + 0.5) / 256.0
        v = (1.0 - abs(d)) * q1 + d * q2
        ends.append(v / np.linalg.norm(v))
    straight = float(ends[0] @ M[0] + ends[1] @ M[1])
    swapped = float(ends[0] @ M[1] + ends[1] @ M[0])
    if swapped > straight:
        ends = ends[::-1]
    ang = (angle(ends[0], M[0]), angle(ends[1], M[1]))
    limit = half_angle(M) if max_angle == "half" else max_angle
    fell = tuple(limit is not None and a > limit for a in ang)
    return {"raw": np.stack(ends), "vectors": np.stack([M[s] if fell[s] else ends[s] for s in (0, 1)]), "angle_to_prior": ang,
            "fell_back": fell}


def basis_of(v):
    """M float64 3x3 of two unit vectors: the two as they are, and their normalised cross product"""
    c = np.cross(v[0], v[1])
    return np.stack([v[0], v[1], c / np.linalg.norm(c)])


def estimate(raster, shrink=1, bg=220, beta=0.15, alpha=1.0, M=H_DAB, max_angle="half"):
    """the whole rule on one (probe view of a) raster -> dict with moments, hist, plane, eigenvalues and what vectors() returns; M is
    the basis of the result as stain_reference.basis builds it"""
    bq = beta_q(beta)
    m = moments(raster, shrink, bg, bq)
    eq1, eq2, w = plane(m)
    h = direction_hist(raster, shrink, bg, bq, eq1, eq2)
    out = vectors(h, eq1, eq2, alpha, M, max_angle)
    out.update(moments=m, hist=h, plane=(eq1, eq2), eigenvalues=w, M=basis_of(out["vectors"]))
    return out


def remix_tables(M_source, gains, M_target):
    """THE STAIN RULE's tables with A = inv(M_source) . diag(g0, g1, 1) . M_target, the float64 product rounded once; D the source's"""
    t = sref.tables(gains, M_source)
    Ms, Mt = np.asarray(M_source, np.float64), np.asarray(M_target, np.float64)
    t["A"] = (np.linalg.inv(Ms) @ np.diag([gains[0], gains[1], 1.0]) @ Mt).reshape(-1).astype(np.float32)
    return t


# ---- the synthetic slide -------------------------------------------------------------------------------------------------------------
def concentration_maps(H, W, dab_share, seed):
    """-> (c0, c1 float64 [h, w] over the tissue rectangle, the rectangle (y0, y1, x0, x1)): c0 ~ U(0.2, 1.6); a `dab_share` of the
    pixels carries c1 ~ U(0.3, 2.0) and 0.3 of its c0"""
    rng = np.random.default_rng(seed)
    y0, y1, x0, x1 = H // 8, H - H // 8, W // 8, W - W // 8
    shape = (y1 - y0, x1 - x0)
    c0 = rng.uniform(0.2, 1.6, shape)
    dab = rng.random(shape) < dab_share
    c1 = np.where(dab, rng.uniform(0.3, 2.0, shape), 0.0)
    return np.where(dab, 0.3 * c0, c0), c1, (y0, y1, x0, x1)


def synthetic_slide(H, W, stain0, stain1, dab_share, seed, strength=(1.0, 1.0)):
    """uint8 [H, W, 3]: a tissue rectangle on glass of 235 .. 246; inside, od = s0 c0 v0 + s1 c1 v1 on the unit vectors, bytes rint(256 *
    10^-od - 1) plus uniform noise of -2 .. 2.  Equal (H, W, dab_share, seed) give equal concentration maps whatever the vectors."""
    c0, c1, (y0, y1, x0, x1) = concentration_maps(H, W, dab_share, seed)
    rng = np.random.default_rng([seed, 1])
    slide = rng.integers(235, 247, size=(H, W, 3)).astype(np.uint8)
    M = sref.basis(stain0, stain1)
    od = strength[0] * c0[..., None] * M[0] + strength[1] * c1[..., None] * M[1]
    px = np.rint(256.0 * 10.0 ** (-od) - 1.0) + rng.integers(-2, 3, size=od.shape)
    slide[y0:y1, x0:x1] = np.clip(px, 0, 255).astype(np.uint8)
    return slide
