"""Merge-NMS rows bit for bit: a NumPy restatement of the merge in the ORDER of the kernels of csrc/ay_nms.hip (TEST INFRASTRUCTURE ONLY).

The oracle (`oracle/boxes_oracle.py`) fixes which candidates form a cluster and every row field but the merged corners: those are
confidence-weighted sums whose order the reference leaves open, so the kernels agree with the oracle to 1e-5 only.  All three merge
paths (alive words in registers, one per lane, in global memory) promise the same order, restated here:

  * candidates are sorted by the key (~bits(conf * max class score) << 32) | row; j is a candidate's sorted position;
  * a cluster is summed by one wavefront: lane j & 63 meets member j, words (j >> 6) in ascending order, and adds
    sw += conf, s_k += fp32(conf * corner_k) (the product is rounded before the add: the build has no contraction);
  * the 64 lanes are reduced by an xor butterfly from offset 32 down to 1; lane 0 ends with v[:h] + v[h:] halved 64 -> 1;
  * corner_k = s_k / sw in fp32.

`exact_case(C)` is the batch the exact tests share: N = 8 192 rows and images whose candidate counts sit on the word boundary and on
both sides of each path limit, in clusters of about 12 members so that a cluster's members spread over several words and lanes."""
import functools
import types

import numpy as np

from oracle import boxes_oracle as bo

F32 = np.float32
N_ROWS = 8192
CANDIDATES = (0, 1, 64, 65, 1000, 1024, 1025, 3000, 4096, 4097, 6000)
CONF_THRES, NMS_THRES = 0.5, 0.4


def sorted_positions(img, conf_thres=CONF_THRES):
    """{original row: sorted position j} of the candidates of one image [N, 5+C] (the filter kernel's key, ascending)"""
    rows = np.nonzero(img[:, 4] >= F32(conf_thres))[0]
    score = (img[rows, 4] * img[rows, 5:].max(1)).astype(F32)
    key = (np.invert(score.view(np.uint32)).astype(np.uint64) << np.uint64(32)) | rows.astype(np.uint64)
    pos = np.empty(img.shape[0], np.int64)
    pos[:] = -1
    pos[rows[np.argsort(key)]] = np.arange(rows.size)
    return pos


def merged_corners(conf, corners, j):
    """One cluster: conf [m], corners [m, 4] of its members, j [m] their sorted positions.  float32 [4]."""
    acc = np.zeros((64, 5), F32)
    for i in np.argsort(j):
        lane = int(j[i]) & 63
        w = F32(conf[i])
        acc[lane, 0] = acc[lane, 0] + w
        acc[lane, 1:] = acc[lane, 1:] + (w * corners[i].astype(F32)).astype(F32)
    h = 32
    while h:
        acc = acc[:h] + acc[h:]
        h >>= 1
    assert acc.dtype == F32 and acc.shape == (1, 5)
    return acc[0, 1:] / acc[0, 0]


def exact_rows(img, o_rows, clusters, conf_thres=CONF_THRES):
    """The oracle's rows [n, 7] of one image (corners already in `img`) with the corners merged in the kernels' order"""
    pos = sorted_positions(img, conf_thres)
    out = np.array(o_rows, F32, copy=True)
    for h, members in enumerate(clusters):
        assert (pos[members] >= 0).all()
        out[h, :4] = merged_corners(img[members, 4], img[members, :4], pos[members])
    return out


def exact_image(N, C, n, rng, per_cluster=12, size=1024.0):
    """[N, 5+C] with n candidates (conf >= 0.5) on random rows, in spatial clusters of about `per_cluster` members drawn like
    test_gpu_nms._nms_image: centres with a 4-pixel normal scatter, sides within +-10 %, 80 % of a cluster in its own class.  One
    candidate in ten shares one score (conf == conf_thres, dominant class score 0.75): their order is the original row's."""
    img = np.zeros((N, 5 + C), F32)
    img[:, 0:2] = rng.uniform(0, size, (N, 2))
    img[:, 2:4] = rng.uniform(8, 120, (N, 2))
    img[:, 4] = rng.uniform(0.0, CONF_THRES * 0.98, N)
    img[:, 5:] = rng.uniform(0.01, 0.99, (N, C))
    if n == 0:
        return img
    idx = np.sort(rng.choice(N, n, replace=False))
    n_clusters = max(1, n // per_cluster)
    centers = rng.uniform(60, size - 60, (n_clusters, 2))
    sizes = rng.uniform(20, 110, (n_clusters, 2))
    cls_of = rng.integers(0, C, n_clusters)
    which = rng.integers(0, n_clusters, n)
    img[idx, 0:2] = centers[which] + rng.normal(0, 4.0, (n, 2))
    img[idx, 2:4] = sizes[which] * rng.uniform(0.9, 1.1, (n, 2))
    img[idx, 4] = rng.permutation(np.linspace(CONF_THRES + 0.003, 0.999, n)).astype(F32)
    dom = np.where(rng.uniform(size=n) < 0.8, cls_of[which], rng.integers(0, C, n))
    img[idx, 5:] = rng.uniform(0.01, 0.45, (n, C))
    img[idx, 5 + dom] = rng.uniform(0.5, 0.99, n)
    t = np.nonzero(rng.random(n) < 0.1)[0]
    img[idx[t], 4] = F32(CONF_THRES)
    img[idx[t], 5:] = 0.25
    img[idx[t], 5 + dom[t]] = 0.75
    return img


@functools.lru_cache(maxsize=None)
def exact_case(C):
    """pred [B, N, 5+C] as cx, cy, w, h; corners: the same with corner boxes; ncand [B]; per image: rows [n, 7] | None in the kernels'
    order, o_rows the oracle's, keep [n] original rows of the heads, clusters (original rows per head).  Computed once per C and
    shared, so every array of it is read-only."""
    rng = np.random.Generator(np.random.PCG64(5))
    pred = np.stack([exact_image(N_ROWS, C, n, rng) for n in CANDIDATES])
    corners = pred.copy()
    o_rows, o_keep, o_clusters = bo.non_max_suppression(corners, CONF_THRES, NMS_THRES)   # corners in place
    rows = [None if r is None else exact_rows(corners[b], r, o_clusters[b]) for b, r in enumerate(o_rows)]
    for a in [pred, corners] + [r for r in rows if r is not None] + [r for r in o_rows if r is not None] + list(o_keep) + [c for cl in o_clusters for c in cl]:
        a.setflags(write=False)
    return types.SimpleNamespace(pred=pred, corners=corners, ncand=np.asarray(CANDIDATES), rows=rows, o_rows=o_rows, keep=o_keep,
                                 clusters=o_clusters)
