"""GPU (-m gpu): ay_yolo_loss_fwd_bwd, ay_yolo_loss_giou_fwd_bwd and ay_build_targets against tests/yolo_loss_reference.py at the
grid sizes training runs them at: the grid-stride second sweep of yolo_loss_pass (more than 1024 x 256 cells), yolo_loss_reduce
with 1, 2, 3 and 64 rows per chunk and a short or empty last chunk, three workgroups of yolo_targets_pass1, and a hand-written
target list with an anchor tie, a wh_iou exactly on the ignore threshold, targets on cell and image edges, 64 targets in one cell,
rows the kernel drops and saturated logits.  tests/test_yolo_loss_cpu.py holds the conditions this rests on.

Counts (slots 7, 8, 9, 12, 13, 14 of the sums) are compared as integers, the nine loss and metric sums and every element of dhead
against float64 with a bar per element class: 4 E floored at 2^-22 of the class scale, E being the distance of the reference's
float32 twin from float64 (measured on the CPU, never on the kernel).  profiles/yolo_loss_margins.txt records E and the device's
measured error for every case and class; `PYTHONPATH=. python tests/test_gpu_yolo_loss.py` on the GPU prints that table."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import yolo_loss_reference as R
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from test_gpu_conv_exact import Guarded

pytestmark = pytest.mark.gpu
F32 = np.float32
RUNS = [(n, b) for n in R.CASES for b in (("mse", "giou") if n != "saturated" else ("mse",))]
run_id = lambda r: r if isinstance(r, str) else None


def _dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def _workspace(c, fill=0xA5):
    n = _lib.lib().ay_yolo_loss_workspace_bytes(c.B, c.A, c.C, c.G)
    return torch.full((n,), fill, device=_dev(), dtype=torch.uint8)


def run_loss(c, box_loss, grad_scale=1.0, ignore_thres=None, targets=None, ws=None, fill=0xA5):
    """one call on the case's head and FULL target list (dropped rows included): dhead and the 16-float sums come back from inside
    guard bands.  Without `ws` the workspace is a fresh one holding `fill` in every byte; a workspace the caller passes is used as it
    is, with whatever the call before left in it.  -> (dhead, sums) as NumPy arrays"""
    L, dev = _lib.lib(), _dev()
    tg = c.targets if targets is None else targets
    hd, td = torch.from_numpy(c.head).to(dev), torch.from_numpy(np.ascontiguousarray(tg)).to(dev)
    dhead, sums = Guarded(c.head.shape, "f32", dev), Guarded((16,), "f32", dev)
    ws = _workspace(c, fill) if ws is None else ws
    assert ws.numel() >= L.ay_yolo_loss_workspace_bytes(c.B, c.A, c.C, c.G)
    an = (C.c_float * (2 * c.A))(*[float(v) for a in c.anchors for v in a])
    fn = L.ay_yolo_loss_giou_fwd_bwd if box_loss == "giou" else L.ay_yolo_loss_fwd_bwd
    thres = c.ignore_thres if ignore_thres is None else ignore_thres
    check(fn(ptr(hd), ptr(td) if len(tg) else None, len(tg), c.B, c.A, c.C, c.G, c.img_dim, an, C.c_float(thres), C.c_float(grad_scale),
             ptr(dhead.t), ptr(sums.t), ptr(ws), ws.numel(), _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert dhead.intact() and sums.intact(), "a store outside dhead / sums_out"
    return dhead.t.cpu().numpy(), sums.t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def device(name, box_loss):
    return run_loss(R.case(name), box_loss)


def figures(name, box_loss, d, s, ignore_thres=None):
    """measured error and bar per class, printed before anything is asserted"""
    _, _, ref, Eg, Es = R.reference(name, box_loss, ignore_thres)
    eg, stray = R.grad_errors(d, ref)
    es = R.sum_errors(s, ref)
    rows = [(n, Eg[n], R.bar(Eg[n]), eg[n]) for n in R.GRAD_CLASSES] + [("sum " + n, Es[n], R.bar(Es[n]), es[n]) for n in es]
    for n, E, b, got in rows:
        print(f"{name:10s} {box_loss:4s} {n:19s} E {E:9.2e}  bar {b:9.2e}  device {got:9.2e}")
    return ref, rows, stray


def compare(name, box_loss, d, s, ignore_thres=None):
    ref, rows, stray = figures(name, box_loss, d, s, ignore_thres)
    for k in R.COUNT_SLOTS:
        assert float(s[k]) == ref.sums[k], (R.SLOT_NAMES[k], float(s[k]), ref.sums[k])
    assert s[15] == 0.0
    if box_loss == "giou":
        assert s[1] == 0.0 and s[2] == 0.0 and s[3] == 0.0
    assert np.isfinite(d).all() and np.isfinite(s).all()
    assert stray == 0, "gradient outside the object / no-object cells"
    for n, E, b, got in rows:
        assert got <= b, (name, box_loss, n, got, b)
    return ref


@pytest.mark.parametrize("name,box_loss", RUNS, ids=run_id)
def test_loss_sums_and_gradient(name, box_loss):
    """counts as integers; loss and metric sums and every gradient element within its class bar of float64 (`saturated`: of torch
    float32 autograd, the semantics bce_logit_grad claims); exact zeros everywhere else; guard bands intact"""
    d, s = device(name, box_loss)
    compare(name, box_loss, d, s)


def test_saturated_zeros_and_clamps():
    c, _, ref, _, _ = R.reference("saturated")
    d, s = device("saturated", "mse")
    d, want = d.reshape(ref.cls_id.shape), ref.dhead.reshape(ref.cls_id.shape)
    assert sum(want[idx] == 0.0 for idx in c.planted) == 12
    for idx in c.planted:
        if want[idx] == 0.0:
            assert d[idx] == 0.0, idx
        else:
            assert d[idx] != 0.0 and abs(d[idx] - want[idx]) <= 1e-5 * abs(want[idx]), idx
    plain = R.unplanted(c)
    base = R.loss_reference(plain, R.assign(plain), "mse", torch.float32)
    assert s[5] - base.sums[5] > 190 and s[4] - base.sums[4] > 120            # the -100 clamps are in the loss


@pytest.mark.parametrize("box_loss", ["mse", "giou"])
def test_empty_target_list(box_loss):
    c = R.case("empty")
    d, s = device("empty", box_loss)
    assert s[7] == 0 and s[8] == c.cells and np.isfinite(d).all()
    d = d.reshape(c.B, c.A, 5 + c.C, c.G, c.G)
    assert np.count_nonzero(d[:, :, :4]) == 0 and np.count_nonzero(d[:, :, 5:]) == 0 and np.count_nonzero(d[:, :, 4]) == c.cells
    assert all(s[k] == 0 for k in (0, 1, 2, 3, 4, 6, 9, 10, 13, 14))


@pytest.mark.parametrize("box_loss", ["mse", "giou"])
def test_edges_below_the_exact_threshold(box_loss):
    """ignore_thres = 0.4999 clears the cells whose wh_iou is exactly 0.5, which 0.5 leaves no-object (the test is `>`)"""
    d, s = run_loss(R.case("edges"), box_loss, ignore_thres=0.4999)
    ref = compare("edges", box_loss, d, s, ignore_thres=0.4999)
    assert ref.sums[8] < R.reference("edges", box_loss)[2].sums[8] == device("edges", box_loss)[1][8]


@pytest.mark.parametrize("box_loss", ["mse", "giou"])
def test_dropped_rows_change_nothing(box_loss):
    c = R.case("edges")
    d, s = run_loss(c, box_loss, targets=R.edges_targets(dropped=False))
    d0, s0 = device("edges", box_loss)
    assert np.array_equal(d, d0) and np.array_equal(s, s0)


@pytest.mark.parametrize("box_loss", ["mse", "giou"])
def test_workspace_is_rebuilt_by_every_call(box_loss):
    """one workspace, never refilled, through `stride` twice, `parts17`, `edges` at 0.4999, `edges`, `empty`: every call sees the winners,
    flags, multi-hot classes, sums and partial rows the call before left (under another layout, and for `edges` after `edges` under
    the same one, with more cells cleared) and gives the bits of a fresh workspace"""
    ws = _workspace(R.case("stride"))
    run_loss(R.case("stride"), box_loss, ws=ws)
    for name, thres in (("stride", None), ("parts17", None), ("edges", 0.4999), ("edges", None), ("empty", None)):
        d, s = run_loss(R.case(name), box_loss, ignore_thres=thres, ws=ws)
        d0, s0 = device(name, box_loss) if thres is None else run_loss(R.case(name), box_loss, ignore_thres=thres)
        assert np.array_equal(d, d0) and np.array_equal(s, s0), (name, thres)


@pytest.mark.parametrize("name,box_loss", [("stride", "mse"), ("parts17", "giou"), ("edges", "mse"), ("empty", "mse")])
def test_workspace_prefill_does_not_show(name, box_loss):
    """0xA5 in every byte reads as -2.9e-16 in the float regions of the workspace (multi-hot classes, sums, partial rows), below every
    bar; 0xFF reads as NaN there.  Both give the same bits."""
    d, s = run_loss(R.case(name), box_loss, fill=0xFF)
    d0, s0 = device(name, box_loss)
    assert np.array_equal(d, d0) and np.array_equal(s, s0)


@pytest.mark.parametrize("name,box_loss", [("stride", "mse"), ("stride", "giou"), ("cap_ragged", "mse"), ("edges", "giou")])
def test_two_runs_are_the_same_bits(name, box_loss):
    d, s = run_loss(R.case(name), box_loss)
    d0, s0 = device(name, box_loss)
    assert np.array_equal(d.view(np.uint32), d0.view(np.uint32)) and np.array_equal(s.view(np.uint32), s0.view(np.uint32))


@pytest.mark.parametrize("name,box_loss", [("stride", "mse"), ("stride", "giou"), ("edges", "mse")])
def test_grad_scale_scales_the_gradient_only(name, box_loss):
    d, s = run_loss(R.case(name), box_loss, grad_scale=0.25)
    d0, s0 = device(name, box_loss)
    assert np.array_equal(d, F32(0.25) * d0) and np.array_equal(s, s0)


BT_NAMES = ["iou_scores", "class_mask", "obj_mask", "noobj_mask", "tx", "ty", "tw", "th", "tcls", "tconf"]


@pytest.mark.parametrize("name", ["edges", "stride", "empty"])
def test_build_targets_entry_point(name):
    """ay_build_targets through the C entry point, on boxes and class scores of the test's own, against boxes_oracle.build_targets
    on the filtered list: masks, tconf, tcls and class_mask exact, tx, ty, tw, th and iou_scores within 1e-6"""
    L, dev = _lib.lib(), _dev()
    c = R.case(name)
    B, A, Cc, G = c.B, c.A, c.C, c.G
    rng = np.random.Generator(np.random.PCG64(77))
    pb = rng.uniform(0, G, (B, A, G, G, 4)).astype(F32)
    pc = rng.uniform(0, 1, (B, A, G, G, Cc)).astype(F32)
    top = np.sort(pc, -1)
    assert Cc == 1 or (top[..., -1] > top[..., -2]).all()
    sa = (np.asarray(c.anchors, F32) / F32(8)).astype(F32)
    ref = R.build_targets(pb, pc, R.filter_dropped(c.targets, B, Cc, G), sa, c.ignore_thres)
    pbd, pcd, td = (torch.from_numpy(v).to(dev) for v in (pb, pc, c.targets))
    fl = {n: Guarded((B, A, G, G, Cc) if n == "tcls" else (B, A, G, G), "f32", dev) for n in BT_NAMES if "mask" not in n or n == "class_mask"}
    obj = torch.full((B, A, G, G), 7, device=dev, dtype=torch.uint8)
    noobj = torch.full((B, A, G, G), 7, device=dev, dtype=torch.uint8)
    ws = torch.full((max(L.ay_build_targets_workspace_bytes(B, A, G), 1),), 0xA5, device=dev, dtype=torch.uint8)
    an = (C.c_float * (2 * A))(*sa.reshape(-1).tolist())
    n = len(c.targets)
    check(L.ay_build_targets(ptr(pbd), ptr(pcd), ptr(td) if n else None, n, B, A, Cc, G, an, C.c_float(c.ignore_thres),
                             ptr(fl["iou_scores"].t), ptr(fl["class_mask"].t), ptr(obj), ptr(noobj), ptr(fl["tx"].t), ptr(fl["ty"].t),
                             ptr(fl["tw"].t), ptr(fl["th"].t), ptr(fl["tcls"].t), ptr(fl["tconf"].t), ptr(ws), ws.numel(),
                             _lib.stream_ptr()))
    torch.cuda.synchronize()
    assert all(g.intact() for g in fl.values())
    got = dict({k: g.t.cpu().numpy() for k, g in fl.items()}, obj_mask=obj.cpu().numpy(), noobj_mask=noobj.cpu().numpy())
    for k, r in zip(BT_NAMES, ref):
        if k in ("obj_mask", "noobj_mask"):
            np.testing.assert_array_equal(got[k], r.astype(np.uint8), err_msg=k)
        elif k in ("tconf", "tcls", "class_mask"):
            np.testing.assert_array_equal(got[k], r, err_msg=k)
        else:
            np.testing.assert_allclose(got[k], r, rtol=1e-6, atol=1e-6, err_msg=k)


if __name__ == "__main__":      # the table of profiles/yolo_loss_margins.txt
    from test_gpu_train import adam_grid_stride_figures
    print("case       loss class               E (float32 twin vs float64)  bar = max(4 E, 2^-22)  device vs float64")
    for name, box_loss in RUNS:
        d, s = device(name, box_loss)
        figures(name, box_loss, d, s)
    for row in adam_grid_stride_figures():
        print("adam_flat  step {step:4d} grad_scale {grad_scale:4.2f} {what:7s} E {E:9.2e}  bar {bar:9.2e}  device {device:9.2e}".format(**row))
