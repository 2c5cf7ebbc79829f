"""ay_merge_detections (csrc/ay_merge.hip), the union-merge of `--merge_boxes True` on the device, called through the C ABI (-m gpu).

Reference: `oracle.boxes_oracle.merge_detections_ordered` on the CPU (double precision, pure Python), through tests/merge_reference.py,
which builds the inputs and caches the oracle's rows; tests/test_merge_cpu.py shows on the CPU that each input reaches the branch it is
here for.  Every comparison is equality of float32 BITS, in rows and in order: the kernel copies input values and writes small integers
and minima, nothing is rounded (so -0.0 is not +0.0).  What a call does not own is prefilled (a NaN pattern in rows_out, -7 in
count_out, guard words behind both) and must come back untouched: the rows behind count_out[b] of every image, the guards; the inputs
must come back as they went in.

The rules pinned: membership BY VALUE among live and among removed rows (lattice, strides_present; lattice_d alone has a merged row
that equals a live row carrying the "value was removed" flag, which is still in the set); int() truncation toward zero
(truncation); the first partner at any distance from i (strides); set() on the 64-lane boundaries (dups); labels passed through and
compared as values (labels); the 2n - 1 row table (capacity); count clamped to [0, max_rows] and images max_rows rows apart (counts)."""
import numpy as np
import pytest
import torch

import merge_reference as mr
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.postprocess import merge_detections, merge_detections_batch_device, merge_detections_device

pytestmark = pytest.mark.gpu

GUARD = 16
SENT = 0x7FC0DEAD                      # a NaN no merge can produce
CASES = mr.cases()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def fresh(dev, B, M):
    return (torch.full((B * M * 7 + GUARD,), SENT, dtype=torch.int32, device=dev), torch.full((B + GUARD,), -7, dtype=torch.int32, device=dev))


def owned(out, cnt, B, M):
    """after a call: guards and the rows behind count_out[b] untouched -> (bits uint32 [B, M, 7], count_out [B])"""
    got, n = out.cpu().numpy().view(np.uint32), cnt.cpu().numpy()
    assert (got[B * M * 7:] == SENT).all() and (n[B:] == -7).all()
    got, n = got[:B * M * 7].reshape(B, M, 7), n[:B]
    for b in range(B):
        assert 0 <= n[b] <= M, (b, n[b])
        assert (got[b, n[b]:] == SENT).all(), b
    return got, n


def launch(dev, rows, count):
    """one call on rows float32 [B, M, 7], count int32 [B] (numpy)"""
    B, M, _ = rows.shape
    d_rows, d_count = torch.from_numpy(rows.copy()).to(dev), torch.from_numpy(np.asarray(count, np.int32).copy()).to(dev)
    out, cnt = fresh(dev, B, M)
    check(_lib.lib().ay_merge_detections(ptr(d_rows), ptr(d_count), B, M, ptr(out), ptr(cnt), _lib.stream_ptr()), "ay_merge_detections")
    torch.cuda.synchronize()
    assert d_rows.cpu().numpy().tobytes() == rows.tobytes() and d_count.cpu().numpy().tolist() == list(count)      # inputs as they went in
    return owned(out, cnt, B, M)


def pack(dets, M):
    """images of uneven length in one [B, M, 7] batch, the overlapping class-1 filler behind each"""
    rows = np.stack([np.concatenate([d, mr.filler(M - len(d))]) for d in dets]).astype(np.float32)
    return rows, np.asarray([len(d) for d in dets], np.int32)


def same(got, n, b, det, what):
    bits, _ = mr.expected(det)
    assert n[b] == len(bits), (what, int(n[b]), len(bits))
    diff = np.flatnonzero((got[b, :n[b]] != bits).any(1))
    assert diff.size == 0, (what, int(diff[0]), got[b, diff[0]].view(np.float32), bits[diff[0]].view(np.float32))


SMALL = [nm for nm in CASES if nm not in mr.LARGE]


# ---- 1. exact results -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("names", [SMALL, list(mr.LARGE)], ids=["small", "large"])
def test_every_family_bit_for_bit(dev, names):
    dets = [CASES[nm]() for nm in names]
    rows, count = pack(dets, max(len(d) for d in dets))
    got, n = launch(dev, rows, count)
    for b, nm in enumerate(names):
        same(got, n, b, dets[b], nm)
    if "capacity" in names:
        assert n[names.index("capacity")] == 1


@pytest.mark.parametrize("max_rows", mr.COUNT_MAX_ROWS)
def test_counts_clamp_and_images_lie_max_rows_apart(dev, max_rows):
    rows, count, valid = mr.count_batch(max_rows)
    got, n = launch(dev, rows, count)
    for b in range(len(count)):
        same(got, n, b, rows[b, :valid[b]], (max_rows, int(count[b])))
    assert n[4] == 0 and n[5] == 0 and n[3] == 1


def test_two_runs_give_the_same_bytes(dev):
    names = list(CASES)
    dets = [CASES[nm]() for nm in names]
    rows, count = pack(dets, mr.MAX_ROWS)
    a, na = launch(dev, rows, count)
    b, nb = launch(dev, rows, count)
    assert a.tobytes() == b.tobytes() and na.tobytes() == nb.tobytes()
    for k, nm in enumerate(names):
        same(a, na, k, dets[k], nm)


# ---- 2. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one_and_leave_the_outputs_alone(dev):
    L, sp = _lib.lib(), _lib.stream_ptr()
    assert L.ay_merge_detections_max_rows() == mr.MAX_ROWS == 1024
    det = CASES["lattice_a"]()
    M = len(det)
    rows, count = torch.from_numpy(det.copy()).to(dev), torch.tensor([M], dtype=torch.int32, device=dev)
    out, cnt = fresh(dev, 1, M)
    good = dict(rows=ptr(rows), count=ptr(count), batch=1, max_rows=M, rows_out=ptr(out), count_out=ptr(cnt))
    call = lambda **kw: L.ay_merge_detections(*{**good, **kw}.values(), sp)
    for bad in (dict(rows=None), dict(count=None), dict(rows_out=None), dict(count_out=None), dict(batch=0), dict(batch=-1), dict(max_rows=0),
                dict(max_rows=-1), dict(max_rows=1025), dict(rows_out=ptr(rows))):
        assert call(**bad) == -1, bad
        assert L.ay_last_error()
    torch.cuda.synchronize()
    assert (out == SENT).all() and (cnt == -7).all() and rows.cpu().numpy().tobytes() == det.tobytes() and count.item() == M
    assert call() == 0                                                 # the good call is good
    torch.cuda.synchronize()
    got, n = owned(out, cnt, 1, M)
    same(got, n, 0, det, "lattice_a")


# ---- 3. a captured HIP graph ------------------------------------------------------------------------------------------------------------
def test_hip_graph_of_one_call_replays_on_other_rows_and_counts(dev):
    """one call captured on one stream (no side branches); rows and counts overwritten in place between replays"""
    B, M = 3, 300
    a, t, p = CASES["lattice_a"](), CASES["truncation"](), CASES["strides_present"]()
    inputs = [pack([a, t, CASES["labels"]()], M), pack([t, CASES["dups_strides"]()[:150], a[:100]], M), pack([p, a[::-1], t[:7]], M)]
    rows, count = torch.from_numpy(inputs[0][0].copy()).to(dev), torch.from_numpy(inputs[0][1].copy()).to(dev)
    out, cnt = fresh(dev, B, M)

    def step():
        check(_lib.lib().ay_merge_detections(ptr(rows), ptr(count), B, M, ptr(out), ptr(cnt), _lib.stream_ptr()), "ay_merge_detections")

    step()                                                            # eager once (loads the code object)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    for k in (1, 2, 0, 1):
        out.fill_(SENT)
        cnt.fill_(-7)
        rows.copy_(torch.from_numpy(inputs[k][0].copy()))
        count.copy_(torch.from_numpy(inputs[k][1].copy()))
        g.replay()
        torch.cuda.synchronize()
        got, n = owned(out, cnt, B, M)
        eager, en = launch(dev, *inputs[k])
        assert got.tobytes() == eager.tobytes() and n.tobytes() == en.tobytes(), k
        for b in range(B):
            same(got, n, b, inputs[k][0][b, :inputs[k][1][b]], (k, b))


# ---- 4. the Python wrappers -----------------------------------------------------------------------------------------------------------------
def test_batch_wrapper_on_uneven_lists(dev):
    """M = max(n) = 37: the small image stride; None stays None; each image as a direct call of its own"""
    dets = [CASES["lattice_a"]()[:37], None, CASES["truncation"]()[:5], CASES["labels"]()[:1], CASES["dups_small"]()]
    got = merge_detections_batch_device([None if d is None else torch.from_numpy(d.copy()) for d in dets])
    assert len(got) == len(dets) and got[1] is None
    for b, d in enumerate(dets):
        if d is None:
            continue
        one, n = launch(dev, d[None], [len(d)])
        assert got[b].dtype == torch.float32 and got[b].numpy().view(np.uint32).tobytes() == one[0, :n[0]].tobytes(), b
        same(one, n, 0, d, b)
    assert merge_detections_batch_device([None, None]) == [None, None] and merge_detections_batch_device([]) == []
    with pytest.raises(_lib.AyError):
        merge_detections_batch_device([torch.from_numpy(mr.grid(1024)), torch.from_numpy(np.concatenate([mr.grid(1024), mr.filler(1)]))])


def test_device_wrapper_clamps_the_count_of_nms(dev):
    """nms_device counts every kept row, also those beyond max_det: count > M is M rows"""
    rows, count, valid = mr.count_batch(64)
    d_rows, d_count = torch.from_numpy(rows.copy()).to(dev), torch.from_numpy(count.copy()).to(dev)
    out, n = merge_detections_device(d_rows, d_count)
    torch.cuda.synchronize()
    assert out.shape == d_rows.shape and d_rows.cpu().numpy().tobytes() == rows.tobytes() and d_count.cpu().tolist() == count.tolist()
    got, n = out.cpu().numpy().view(np.uint32), n.cpu().numpy()
    for b in range(len(count)):
        same(got, n, b, rows[b, :valid[b]], int(count[b]))
        assert not got[b, n[b]:].any()                                # the wrapper hands out zeros behind count_out[b]
    with pytest.raises(_lib.AyError):
        merge_detections_device(torch.zeros(2, 1025, 7, device=dev), torch.zeros(2, dtype=torch.int32, device=dev))


# ---- 5. three implementations, one answer -------------------------------------------------------------------------------------------------
def test_host_twin_oracle_and_kernel_agree_on_pair_only_images(dev):
    """postprocess.merge_detections walks in the order of CPython's set, as the reference does: with no cluster of more than two rows
    the order cannot show, and the three are one set of rows"""
    names = list(mr.PAIR_ONLY)
    dets = [CASES[nm]() for nm in names]
    rows, count = pack(dets, mr.MAX_ROWS)
    got, n = launch(dev, rows, count)
    for b, nm in enumerate(names):
        kernel = mr.row_set(got[b, :n[b]].view(np.float32))
        host = merge_detections(torch.from_numpy(dets[b].copy()))
        assert kernel == mr.row_set(mr.expected(dets[b])[1]) == mr.row_set(host.numpy()), nm
        assert len(kernel) == n[b] < len(dets[b])
