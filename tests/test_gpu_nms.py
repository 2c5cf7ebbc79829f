"""Merge-NMS at full-tile scale, with the candidate filter's flush boundaries placed on purpose (-m gpu).

`nms_filter_kernel` (csrc/ay_nms.hip) launches gx = min(64, ceil(N / 256)) workgroups per image; in iteration `it` workgroup `w` reads
rows it * gx * 256 + w * 256 + [0, 256).  A workgroup appends one 64-bit key per candidate to an LDS buffer of 1 024 keys and flushes it
into the image's key array with one global atomic when it holds more than 768 keys at an iteration boundary, and at the end.  The
inputs below are built from that geometry, so that per-workgroup counts land where a wrong flush decision or a wrong key position would
show: 768 and 769 at a decision barrier, every value of 740 .. 800 there, a buffer of exactly 1 024 keys, no candidate, one candidate in
a ragged last iteration.  `_flush_trace` replays the counter to prove that each input reaches the boundaries it is meant to reach.

References: numpy for candidate counts and keys, `oracle/boxes_oracle.py` for the corners (both bit-exact) and for merge-NMS (indices,
counts exact; rows within 1e-5 relative).  These tests do not make a flush race fire on demand; they pin the boundaries so that a wrong
flush, a lost or doubled key or a key written outside its image fails deterministically.

The merged corners are a sum whose order the reference leaves open, so the oracle pins them to 1e-5 only.  The order the three merge
paths share is restated in tests/nms_exact_reference.py; `test_nms_rows_equal_the_restatement_bit_for_bit` holds every path to it as
raw bytes."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import nms_exact_reference as R
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd import utils as ay
from amyloid_yolo_paper_amd._lib import check, ptr
from oracle import boxes_oracle as bo

pytestmark = pytest.mark.gpu
F32 = np.float32
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILTER_BUF = 1024             # NMS_FILTER_BUF: keys a workgroup holds between two flushes
FLUSH_ABOVE = FILTER_BUF - 256
THR = 0.3                     # filter tests: not a binary fraction, so a threshold kept in double somewhere would show


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def close(a, b, tol=1e-5, what=""):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.max(initial=0.0) <= tol, (what, float(err.max()), int(err.argmax()))


def next_pow2(v):
    return 1 << (int(v) - 1).bit_length()


# ----------------------------------------------------------------------------------------- launch geometry and density plans
def _geometry(N):
    gx = min(64, -(-N // 256))
    stride = gx * 256
    return gx, stride, -(-N // stride)


def _block_counts(mask):
    """[iters, gx]: candidates among the rows workgroup w reads in iteration it"""
    gx, stride, iters = _geometry(mask.size)
    m = np.zeros(iters * stride, bool)
    m[:mask.size] = mask
    return m.reshape(iters, gx, 256).sum(-1)


def _rows_of(N, counts, rng):
    """candidate mask [N] with counts[it, w] randomly chosen rows among those workgroup w reads in iteration it"""
    gx, stride, iters = _geometry(N)
    r = rng.random(iters * stride)
    r[N:] = 2.0   # rows past N rank last, so a ragged block draws from its real rows
    rank = np.argsort(np.argsort(r.reshape(iters, gx, 256), -1), -1)
    mask = (rank < np.asarray(counts)[..., None]).reshape(-1)[:N]
    assert np.array_equal(_block_counts(mask), counts)
    return mask


def _flush_trace(counts):
    """replay of the filter's LDS counter: (values read at flush decisions, sizes of all flushes)"""
    iters, gx = counts.shape
    decided, flushed = set(), []
    for w in range(gx):
        k = 0
        for it in range(iters):
            k += int(counts[it, w])
            assert k <= FILTER_BUF
            if it + 1 < iters:
                decided.add(k)
                if k > FLUSH_ABOVE:
                    flushed.append(k)
                    k = 0
        flushed.append(k)
    return decided, flushed


def _sweep_counts(N, shift):
    """Per-workgroup counts whose value at one decision barrier takes every value of 740 .. 800 across the 64 workgroups (740 .. 768
    when only three iterations precede the last), then sits at 768 .. 770 at the later barriers.  One iteration: every count 0 .. 256."""
    gx, _, iters = _geometry(N)
    size = _block_counts(np.ones(N, bool))
    w = np.arange(gx)
    c = np.zeros((iters, gx), np.int64)
    if iters == 1:
        c[0] = (w * 41 + shift) % 257
        return np.minimum(c, size)
    d = min(3, iters - 2)                       # the sweeping barrier (a decision is taken after it)
    hi = 800 if d == 3 else FLUSH_ABOVE
    v = 740 + (w + shift) % (hi - 739)
    for i in range(d + 1):
        c[i] = v // (d + 1) + (i < v % (d + 1))
    k = np.where(v > FLUSH_ABOVE, 0, v)
    for it in range(d + 1, iters):
        c[it] = np.minimum(size[it], np.where(k < 512, 256, np.minimum(256, FLUSH_ABOVE - k + (w + it) % 3)))
        k = k + c[it]
        if it + 1 < iters:
            k = np.where(k > FLUSH_ABOVE, 0, k)
    return np.minimum(c, size)


# ----------------------------------------------------------------------------------------- filter: keys, counts, corners
FILTER_KINDS = ("dense", "empty", "single_last", "sweep", "ties", "random")


def _filter_image(mask, C, rng, tied):
    N = mask.size
    img = np.empty((N, 5 + C), F32)
    img[:, 0:2] = rng.uniform(0, 1024, (N, 2))
    img[:, 2:4] = rng.uniform(8, 120, (N, 2))
    img[:, 4] = rng.uniform(0, THR * 0.98, N)
    img[:, 5:] = rng.uniform(0.01, 0.99, (N, C))
    img[mask, 4] = rng.uniform(THR + 1e-3, 1.0, int(mask.sum()))
    edge = rng.random(N)
    img[mask & (edge < 0.02), 4] = F32(THR)                                  # conf == conf_thres: a candidate
    img[~mask & (edge < 0.02), 4] = np.nextafter(F32(THR), F32(0))           # one ulp below: not one
    img[mask & (edge > 0.99), 5:] = 0.0                                      # score exactly 0
    if tied:   # every candidate has the same score: the keys differ in the row only
        img[mask, 4] = F32(THR)
        img[mask, 5:] = 0.25
        cand = np.nonzero(mask)[0]
        img[cand, 5 + rng.integers(0, C, cand.size)] = 0.75
    return img


def _filter_batch(N, C, B, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    iters = _geometry(N)[2]
    size = _block_counts(np.ones(N, bool))
    pred = np.empty((B, N, 5 + C), F32)
    decided, flushed = set(), []
    for b in range(B):
        kind = FILTER_KINDS[b % len(FILTER_KINDS)]
        mask = np.zeros(N, bool)
        if kind == "dense":
            mask[:] = True
        elif kind == "single_last":
            mask[N - 1] = True
        elif kind == "sweep":
            mask = _rows_of(N, _sweep_counts(N, b), rng)
        elif kind in ("ties", "random"):
            mask = _rows_of(N, np.minimum(size, rng.integers(0, 257, size.shape)), rng)
        pred[b] = _filter_image(mask, C, rng, kind == "ties")
        assert int((pred[b, :, 4] >= F32(THR)).sum()) == int(mask.sum())
        dec, fl = _flush_trace(_block_counts(mask))
        decided |= dec
        flushed += fl
    # the boundaries this batch is built to reach (see _sweep_counts)
    if iters >= 5:
        assert set(range(740, 801)) <= decided and FILTER_BUF in flushed
    elif iters == 4:
        assert set(range(740, FLUSH_ABOVE + 1)) <= decided and FILTER_BUF in flushed
    return pred


def _ref_keys(img, thr):
    """(~float32_bits(conf * max class score) << 32) | row over the candidate rows, sorted"""
    rows = np.nonzero(img[:, 4] >= F32(thr))[0]
    score = (img[rows, 4] * img[rows, 5:].max(1)).astype(F32)
    hi = np.invert(score.view(np.uint32)).astype(np.uint64)
    return np.sort((hi << np.uint64(32)) | rows.astype(np.uint64))


@pytest.mark.parametrize("variant", ["c3", "c3_offset", "c1", "c6", "c80"])
@pytest.mark.parametrize("N", [64512, 131072 + 37, 10000], ids=lambda n: f"N{n}")
def test_filter_keys_counts_and_corners(dev, N, variant):
    """`ay_nms_filter` alone.  N = 64 512: the headline's rows per image, four iterations; 131 109: nine, the last one ragged (37 rows,
    workgroup 0), cap 262 144; 10 000: one iteration on 40 workgroups, the last of them ragged.  C = 3 takes the 32-byte-row path on an
    aligned tensor and the generic path on a view one float into its buffer; C = 1, 6, 80 the generic path.  Checks: the candidate
    counts; each image's keys, sorted, against numpy's (no key lost, doubled or changed); nothing written into the key slots past the
    count, the rest of the workspace, the counters past the batch or the float next to the tensor; the corners of every row converted
    in place bit for bit like `xywh2xyxy`; columns 4.. untouched."""
    Cn = int(variant[1:].split("_")[0])
    offset = variant.endswith("_offset")
    B = 6 if Cn == 80 else (16 if N > 65536 else 64)
    K = 5 + Cn
    pred = _filter_batch(N, Cn, B, seed=N % 1000 + 7 * Cn + offset)
    L = _lib.lib()
    numel = B * N * K
    buf = torch.full((numel + 1,), -3.5, dtype=torch.float32, device=dev)
    view = (buf[1:] if offset else buf[:numel]).view(B, N, K)
    view.copy_(torch.from_numpy(pred))
    assert (view.data_ptr() % 16 == 0) == (not offset)     # 32-byte rows need 16-byte alignment: the offset view takes the generic path
    nbytes = L.ay_nms_workspace_bytes(B, N)
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=dev)
    cand = torch.full((B + 8,), -7, dtype=torch.int32, device=dev)
    check(L.ay_nms_filter(ptr(view), B, N, Cn, ctypes.c_float(THR), ptr(cand), ptr(ws), nbytes, _lib.stream_ptr()), "ay_nms_filter")
    torch.cuda.synchronize()

    cap = next_pow2(N)
    cnt = cand.cpu().numpy()
    assert (cnt[B:] == -7).all()
    np.testing.assert_array_equal(cnt[:B], (pred[..., 4] >= F32(THR)).sum(1))
    keys = ws[:B * cap * 8].view(torch.int64).cpu().numpy().view(np.uint64).reshape(B, cap)
    untouched = np.uint64(0xA5A5A5A5A5A5A5A5)
    for b in range(B):
        n = int(cnt[b])
        np.testing.assert_array_equal(np.sort(keys[b, :n]), _ref_keys(pred[b], THR), err_msg=f"keys of image {b}")
        assert (keys[b, n:] == untouched).all(), f"image {b}: key slots past its count were written"
    assert bool((ws[B * cap * 8:] == 0xA5).all())

    got = view.cpu().numpy()
    np.testing.assert_array_equal(got[..., :4].view(np.uint32), bo.xywh2xyxy(pred[..., :4]).view(np.uint32))
    np.testing.assert_array_equal(got[..., 4:].view(np.uint32), pred[..., 4:].view(np.uint32))
    assert float(buf[0 if offset else numel]) == -3.5


# ----------------------------------------------------------------------------------------- end to end at the same boundaries
def _heavy_counts(N, heavy):
    gx, stride, iters = _geometry(N)
    counts = np.zeros((iters, gx), np.int64)
    for w, per_it in heavy.items():
        counts[:len(per_it), w] = per_it
    return counts


def _heavy_counts_trace(N, heavy):
    """_flush_trace of the heavy workgroups (the extra candidates go to the others)"""
    return _flush_trace(_heavy_counts(N, heavy))


def _nms_image(N, C, heavy, extra, rng, conf_thres=0.5, size=1024.0):
    """[N, 5+C] in the style of golden_cases.nms_prediction (candidates in spatial clusters), with the candidates at chosen places:
    heavy = {workgroup: candidates per iteration from iteration 0}, plus `extra` rows drawn from the other workgroups.  15 % of the
    candidates share one score (conf == conf_thres, dominant class score 0.75), half of those on a grid of disjoint boxes, so the tie
    order -- the original row -- decides which of them comes first; 1 % have score exactly 0."""
    stride = _geometry(N)[1]
    mask = _rows_of(N, _heavy_counts(N, heavy), rng)
    free = np.nonzero(~np.isin((np.arange(N) % stride) // 256, list(heavy)))[0]
    mask[rng.choice(free, extra, replace=False)] = True
    img = np.zeros((N, 5 + C), F32)
    img[:, 0:2] = rng.uniform(0, size, (N, 2))
    img[:, 2:4] = rng.uniform(8, 120, (N, 2))
    img[:, 4] = rng.uniform(0.0, conf_thres * 0.98, N)
    img[:, 5:] = rng.uniform(0.01, 0.99, (N, C))
    idx = np.nonzero(mask)[0]
    n = idx.size
    if n == 0:
        return img
    n_clusters = max(1, n // 3)
    centers = rng.uniform(60, size - 60, (n_clusters, 2))
    sizes = rng.uniform(20, 110, (n_clusters, 2))
    cls_of = rng.integers(0, C, n_clusters)
    which = rng.integers(0, n_clusters, n)
    img[idx, 0:2] = centers[which] + rng.normal(0, 4.0, (n, 2))
    img[idx, 2:4] = sizes[which] * rng.uniform(0.9, 1.1, (n, 2))
    img[idx, 4] = rng.permutation(np.linspace(conf_thres + 0.003, 0.999, n)).astype(F32)
    dom = np.where(rng.uniform(size=n) < 0.8, cls_of[which], rng.integers(0, C, n))
    img[idx, 5:] = rng.uniform(0.01, 0.45, (n, C))
    img[idx, 5 + dom] = rng.uniform(0.5, 0.99, n)
    t = np.nonzero(rng.random(n) < 0.15)[0]
    img[idx[t], 4] = F32(conf_thres)
    img[idx[t], 5:] = 0.25
    img[idx[t], 5 + dom[t]] = 0.75
    g = idx[t[::2]]
    k = np.arange(g.size)
    assert g.size <= 42 * 42
    img[g, 0] = 16 + 24 * (k % 42)
    img[g, 1] = 16 + 24 * (k // 42)
    img[g, 2:4] = 12.0
    img[idx[rng.random(n) < 0.01], 5:] = 0.0
    return img


def _nms_batch(N, C, specs, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    pred = np.stack([_nms_image(N, C, heavy, extra, rng) for heavy, extra in specs])
    ncand = (pred[..., 4] >= F32(0.5)).sum(1)
    assert all(int(ncand[b]) == sum(map(sum, h.values())) + e for b, (h, e) in enumerate(specs))
    return pred, ncand


def _check_vs_oracle(dev, pred, ncand, max_det=8):
    """utils.non_max_suppression and nms_device(max_det) against the oracle: indices, counts exact, rows 1e-5 relative"""
    o_rows, o_keep, _ = bo.non_max_suppression(pred.copy(), 0.5, 0.4)
    res = ay.non_max_suppression(torch.from_numpy(pred.copy()).to(dev), 0.5, 0.4)
    np.testing.assert_array_equal(res.cand_count, ncand)
    for b in range(pred.shape[0]):
        if o_rows[b] is None:
            assert res[b] is None and ncand[b] == 0
            continue
        np.testing.assert_array_equal(res.keep_idx[b], o_keep[b], err_msg=f"image {b} ({ncand[b]} candidates)")
        close(res[b].cpu().numpy(), o_rows[b], 1e-5, f"image {b}")
    rows, keep, count, cand = ay.nms_device(torch.from_numpy(pred.copy()).to(dev), 0.5, 0.4, max_det, slot=5)
    rows, keep, count, cand = rows.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy(), cand.cpu().numpy()
    np.testing.assert_array_equal(cand, ncand)
    for b in range(pred.shape[0]):
        n_all = 0 if o_rows[b] is None else len(o_keep[b])
        assert int(count[b]) == n_all, b
        k = min(n_all, max_det)
        if k:
            np.testing.assert_array_equal(keep[b, :k], o_keep[b][:k])
            close(rows[b, :k], o_rows[b][:k], 1e-5, f"image {b}, max_det {max_det}")
    return res


# (heavy workgroups, extra candidates): every image has a workgroup that flushes in the middle of the loop
FLUSH_SPECS = [
    ({7: [200] * 4}, 200),                                   # 1 000: LDS merge; workgroup 7 flushes 800 keys after iteration 3
    ({3: [193, 192, 192, 192]}, 255),                        # 1 024: the LDS merge's limit; 769 at the barrier
    ({5: [193, 192, 192, 192]}, 256),                        # 1 025: the mid kernel's first size
    ({0: [192] * 4, 21: [195] * 4, 63: [200] * 4}, 700),     # 3 048: mid kernel; 768 (kept), 780, 800 at the barrier
    ({w: [198] * 4 for w in range(1, 5)}, 928),              # 4 096: the mid kernel's limit
    ({w: [198] * 4 for w in range(1, 5)}, 929),              # 4 097: workspace sort and scan
    ({w: [200] * 4 for w in range(7)}, 800),                 # 6 400: workspace sort and scan
]


@pytest.mark.parametrize("case", [(131072 + 37, 3, 61), (100000, 6, 62)], ids=lambda c: f"N{c[0]}_C{c[1]}")
def test_nms_flush_crossing_all_merge_paths_vs_oracle(dev, case):
    """Each merge path (LDS sort + four-wave scan up to 1 024 candidates, the mid kernel up to 4 096, the workspace sort and scan beyond)
    gets images whose candidates cross a filter flush, at the path limits, with score ties across the flush and the sorts."""
    N, C, seed = case
    pred, ncand = _nms_batch(N, C, FLUSH_SPECS, seed)
    for heavy, _ in FLUSH_SPECS:
        assert max(_heavy_counts_trace(N, heavy)[0]) > FLUSH_ABOVE   # a flush before the last iteration
    _check_vs_oracle(dev, pred, ncand)


# N = 64 512 runs four iterations: the decisions are read after iterations 0 .. 2 (at most 768: no flush before the last one)
HEADLINE_SPECS = [
    ({}, 493),                                               # a typical tile of the benchmark
    ({9: [256] * 4}, 0),                                     # 1 024 in one workgroup: 768 at the last decision, one full buffer
    ({0: [256] * 4, 33: [250] * 4}, 800),                    # 2 824: mid kernel
    ({w: [256] * 4 for w in range(10, 15)}, 0),              # 5 120: workspace sort and scan
    ({}, 0),                                                 # no candidate
    ({59: [256] * 4}, 1),                                    # 1 025 (workgroup 59: the last one with rows in iteration 3)
    ({60: [256] * 3}, 300),                                  # workgroup 60 reads no row in iteration 3: 768 at its only flush
    ({w: [247, 247, 247, 100] for w in range(3)}, 200),      # 741 at the last decision
]


def test_nms_headline_batch_vs_oracle(dev):
    """The headline shape, B = 64 images of N = 64 512 rows, C = 3, one batch in one call."""
    decided, flushed = set(), []
    for heavy, _ in HEADLINE_SPECS:
        d, f = _heavy_counts_trace(64512, heavy)
        decided |= d
        flushed += f
    assert {741, FLUSH_ABOVE} <= decided and FILTER_BUF in flushed
    pred, ncand = _nms_batch(64512, 3, HEADLINE_SPECS * 8, 63)
    _check_vs_oracle(dev, pred, ncand)


_CHILD = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
from amyloid_yolo_paper_amd import utils as ay
pred = np.load(sys.argv[2])
res = ay.non_max_suppression(torch.from_numpy(pred).to("cuda:0"), 0.5, 0.4)
out = {"cand": np.asarray(res.cand_count)}
for b, k in enumerate(res.keep_idx):
    out["keep%d" % b] = k
    out["rows%d" % b] = np.zeros((0, 7), np.float32) if res[b] is None else res[b].cpu().numpy()
np.savez(sys.argv[3], **out)
"""


def test_nms_mid_kernel_off_equals_default(dev, tmp_path):
    """AY_NMS_MID=0 (read once per process: a fresh child process) sends images with 1 025 .. 4 096 candidates to the workspace scan
    instead of the mid kernel: the same indices as the default run and the oracle, rows within 1e-5 of the oracle and, byte for byte,
    the default run's rows (the mid kernel against the workspace scan on the same images)."""
    specs = FLUSH_SPECS[2:5]
    pred, ncand = _nms_batch(131072 + 37, 3, specs, 64)
    assert ((ncand > 1024) & (ncand <= 4096)).all()
    res = _check_vs_oracle(dev, pred, ncand)
    o_rows, o_keep, _ = bo.non_max_suppression(pred.copy(), 0.5, 0.4)
    np.save(tmp_path / "pred.npy", pred)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", _CHILD, REPO, str(tmp_path / "pred.npy"),
                                                                            str(tmp_path / "out.npz")]
    p = subprocess.run(cmd, env={**os.environ, "AY_NMS_MID": "0"}, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-4000:]
    z = np.load(tmp_path / "out.npz")
    np.testing.assert_array_equal(z["cand"], ncand)
    for b in range(len(specs)):
        np.testing.assert_array_equal(z[f"keep{b}"], res.keep_idx[b])
        np.testing.assert_array_equal(z[f"keep{b}"], o_keep[b])
        close(z[f"rows{b}"], o_rows[b], 1e-5, f"image {b}")
        np.testing.assert_array_equal(z[f"rows{b}"].view(np.uint32), res[b].cpu().numpy().view(np.uint32), err_msg=f"image {b}")


# ----------------------------------------------------------------------------------------- merged rows bit for bit
@pytest.mark.parametrize("max_det", [max(R.CANDIDATES), 8], ids=lambda m: f"maxdet{m}")
@pytest.mark.parametrize("C", [3, 6], ids=lambda c: f"C{c}")
def test_nms_rows_equal_the_restatement_bit_for_bit(dev, C, max_det):
    """One batch at N = 8 192 with 0, 1, 64, 65, 1 000, 1 024, 1 025, 3 000, 4 096, 4 097 and 6 000 candidates (the word boundary and
    both sides of each path limit; C = 3 reads 32-byte rows in the filter): count, keep_idx and all seven floats of every valid row
    equal tests/nms_exact_reference.py, the merge restated in the kernels' order, as raw bytes.  max_det = 6 000 holds every head,
    max_det = 8 cuts every image that has more."""
    case = R.exact_case(C)
    np.testing.assert_array_equal((case.pred[..., 4] >= F32(0.5)).sum(1), R.CANDIDATES)
    rows, keep, count, cand = ay.nms_device(torch.from_numpy(case.pred.copy()).to(dev), R.CONF_THRES, R.NMS_THRES, max_det, slot=6)
    rows, keep, count, cand = rows.cpu().numpy(), keep.cpu().numpy(), count.cpu().numpy(), cand.cpu().numpy()
    np.testing.assert_array_equal(cand, R.CANDIDATES)
    np.testing.assert_array_equal(count, [len(k) for k in case.keep])
    for b, n in enumerate(R.CANDIDATES):
        k = min(len(case.keep[b]), max_det)
        if k:
            np.testing.assert_array_equal(keep[b, :k], case.keep[b][:k], err_msg=f"image {b} ({n} candidates)")
            np.testing.assert_array_equal(rows[b, :k].view(np.uint32), case.rows[b][:k].view(np.uint32),
                                          err_msg=f"image {b} ({n} candidates)")
