"""NumPy restatement of THE TISSUE RULE of include/amyloid_yolo.h (TEST INFRASTRUCTURE ONLY): a boolean image and slicing.

Nothing here comes from the product: the tile grid is restated too."""
import math

import numpy as np


def halve(r):
    """the ingest's 40x -> 20x halving: 2x2 mean, round half up"""
    h2, w2 = r.shape[0] // 2, r.shape[1] // 2
    q = r[: 2 * h2, : 2 * w2].astype(np.uint16)
    return ((q[0::2, 0::2] + q[0::2, 1::2] + q[1::2, 0::2] + q[1::2, 1::2] + 2) >> 2).astype(np.uint8)


def grid(H, W, tile, overlap=0):
    step = tile - overlap
    n = lambda extent: max(1, -(-(extent - overlap) // step))
    return n(H), n(W), step


def tissue(raster, shrink=1, bg_level=220):
    """bool [H, W]: min(R, G, B) < bg_level on the (halved) image"""
    r = halve(raster) if shrink == 2 else np.asarray(raster)
    return r.min(axis=2).astype(np.int32) < int(bg_level)


def tissue_counts(raster, tile, shrink=1, overlap=0, bg_level=220, tiles=None):
    """int32 [tiles_y, tiles_x]; slicing past the image's edge drops what lies outside: the padding never counts.
    ``tiles=(ty, tx)`` overrides the grid (a kernel call on a region states its own tile counts)."""
    t = tissue(raster, shrink, bg_level)
    ty, tx, step = grid(t.shape[0], t.shape[1], tile, overlap)
    if tiles is not None:
        ty, tx = tiles
    out = np.zeros((ty, tx), np.int32)
    for j in range(ty):
        for i in range(tx):
            out[j, i] = t[j * step:j * step + tile, i * step:i * step + tile].sum()
    return out


def wanted(counts, tile, min_tissue):
    return counts >= max(1, math.ceil(min_tissue * tile * tile))


def test_slide(region):
    """the issue's test slide: white 1000 x 1314, `region` (test_gpu_seam.region_raster()) pasted at row 96, column 192, and a
    10 x 12 speck of value 90 at rows 773-782, columns 10-21"""
    s = np.full((1000, 1314, 3), 255, np.uint8)
    s[96:96 + region.shape[0], 192:192 + region.shape[1]] = region
    s[773:783, 10:22] = 90
    return s


test_slide.__test__ = False   # a builder, not a test
