"""GPU (-m gpu): the entry points the bf16 training step really calls (train_engine_bf16.py) -- the zeroed-workspace, apply-only
and accumulate forms of the BatchNorm passes, the split-K weight gradient on its XCD-remapped branch, the batched filter packer,
the chunked bias gradient, and gradient accumulation through the engine -- each against a float64 torch-CPU reference on the same
bf16-rounded operands, at the shapes where the kernels' loops and grids change (second loop trip, masked unroll group, several
workgroups per (image, plane), ragged last plane, ks >= 8 with a K-loop tail).

Not covered: the `cap` branch of bn_chunks (ay_train_bf16.hip) needs batch * planes * chunks > 16384 workgroups, i.e. operands above
2 GB; it is out of reach of a test that takes seconds.

Measured margins behind every bound that is not inherited from test_gpu_train_bf16.py: profiles/train_bf16_test_margins.txt.
"""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ConvDesc, check, ptr
import pack_reference
from test_gpu_train_bf16 import bf, from_blocked, to_blocked

pytestmark = pytest.mark.gpu

EPS = 1e-5


def _dev():
    return torch.device("cuda", 0)


def _ulp32(t):
    """spacing of fp32 at |t| (float64 tensor)"""
    return torch.from_numpy(np.spacing(t.abs().to(torch.float32).numpy())).double()


# ------------------------------------------------------------------------------------------------------------- BatchNorm
# (B, C, H, W, leaky, has_skip); units = 2 * H * W 16-byte units per (image, plane), a workgroup covers 256 per trip, 4 per thread
# and trip, bn_chunks = ceil(units / 8192)
BN_CASES = [
    (3, 48, 10, 10, 1, 1),    # 200 units: less than one workgroup
    (2, 32, 24, 24, 1, 0),    # 1152 units: a second trip of the unrolled loop with a masked group; skip = NULL
    (2, 32, 24, 24, 0, 1),
    (2, 32, 72, 72, 0, 1),    # 10368 units: 2 workgroups per (image, plane)
    (2, 32, 72, 72, 1, 0),
    (2, 32, 96, 96, 1, 0),    # 18432 units: 3 workgroups, image and chunk index interleave on an odd count
    (2, 32, 96, 96, 0, 1),
    (2, 24, 24, 24, 0, 0),    # ragged last plane (8 channels of 16)
    (1, 40, 9, 13, 1, 1),     # ragged last plane, h != w (the kernels see h * w only), odd pixel count
]
_bn_id = lambda c: "x".join(map(str, c[:4])) + f"-l{c[4]}s{c[5]}"  # noqa: E731


@functools.lru_cache(maxsize=None)
def _bn_case(case):
    """operands (bf16-rounded), the float64 reference forward / backward (computed once per case, never modified) and the blocked
    device copies"""
    B, Cc, H, W, leaky, has_skip = case
    dev = _dev()
    g = torch.Generator().manual_seed(1000 * Cc + 10 * H + W + leaky + 2 * has_skip)
    r = dict(case=case)
    r["z"] = z = bf(torch.randn(B, Cc, H, W, generator=g) * 2 + 0.3)
    r["skip"] = skip = bf(torch.randn(B, Cc, H, W, generator=g)) if has_skip else None
    r["gamma"], r["beta"] = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.3
    r["rm0"], r["rv0"] = torch.randn(Cc, generator=g) * 0.5, torch.rand(Cc, generator=g) + 0.5
    r["dy"] = dy = bf(torch.randn(B, Cc, H, W, generator=g))
    r["dg0"], r["db0"] = torch.randn(Cc, generator=g) * 3, torch.randn(Cc, generator=g) * 3    # gradients already accumulated
    zr = z.double().requires_grad_(True)
    gr, br = r["gamma"].double().requires_grad_(True), r["beta"].double().requires_grad_(True)
    run = {}
    for mom in (0.1, 0.9):
        rm, rv = r["rm0"].double(), r["rv0"].double()
        with torch.set_grad_enabled(mom == 0.1):
            pre = F.batch_norm(zr, rm, rv, gr, br, True, mom, EPS)     # PyTorch semantics: running_var takes the unbiased variance
        run[mom] = (rm, rv)
        if mom == 0.1:
            act = F.leaky_relu(pre, 0.1) if leaky else pre
            yr = act + skip.double() if has_skip else act
            yr.backward(dy.double())
            r["pre"], r["y"] = pre.detach(), yr.detach()
    r["running"] = run
    r["dz"], r["dgamma"], r["dbeta"] = zr.grad, gr.grad, br.grad
    z64 = z.double()
    r["mean"], r["var"] = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
    r["invstd"] = 1.0 / torch.sqrt(r["var"] + EPS)
    r["sums"] = torch.cat([z64.sum((0, 2, 3)), (z64 * z64).sum((0, 2, 3))])
    r["absmean"], r["sqmean"] = z64.abs().mean((0, 2, 3)), (z64 * z64).mean((0, 2, 3))
    r["zb"], r["dyb"] = to_blocked(z, dev), to_blocked(dy, dev)
    r["sb"] = to_blocked(skip, dev) if has_skip else None
    r["gd"], r["bd"] = r["gamma"].to(dev), r["beta"].to(dev)
    return r


def _bn_forward(r, form, momentum, zb=None):
    """one of the three forward entry points -> (y blocked, save_mean, save_invstd, running_mean, running_var)"""
    B, Cc, H, W, leaky, _ = r["case"]
    L, dev, st = _lib.lib(), _dev(), _lib.stream_ptr()
    zb = r["zb"] if zb is None else zb
    rmd, rvd = r["rm0"].clone().to(dev), r["rv0"].clone().to(dev)
    yb = torch.full_like(zb, float("nan"))
    mean, invstd = torch.full((Cc,), float("nan"), device=dev), torch.full((Cc,), float("nan"), device=dev)
    if form == "plain":        # must clear the workspace itself
        fn, ws = L.ay_bn_train_fwd_bf16, torch.full((2 * Cc,), float("nan"), device=dev, dtype=torch.float64)
    elif form == "zeroed_ws":  # the engine clears the workspaces of all layers at once
        fn, ws = L.ay_bn_train_fwd_bf16_zeroed_ws, torch.zeros(2 * Cc, device=dev, dtype=torch.float64)
    else:                      # the producer of z left the sums (the stem): the apply pass alone
        fn, ws = L.ay_bn_train_apply_bf16, r["sums"].to(dev)
    check(fn(ptr(zb), ptr(r["gd"]), ptr(r["bd"]), ptr(rmd), ptr(rvd), C.c_float(momentum), C.c_float(EPS), leaky, ptr(r["sb"]), ptr(yb),
             ptr(mean), ptr(invstd), ptr(ws), B, Cc, H, W, st), form)
    torch.cuda.synchronize()
    return yb, mean.cpu().double(), invstd.cpu().double(), rmd.cpu().double(), rvd.cpu().double()


def _stat_tolerances(r):
    """The statistics are fp32 up to the workgroup's reduction and fp64 above: a value passes through at most 32 sequential fp32 adds
    in its thread (BN_ROUNDS * BN_UNROLL), 7 levels of the cross-lane / LDS tree and, for z^2, the rounding of the product -- fewer
    than 64 roundings of at most 2^-24 relative to a partial sum that sum|z| (resp. sum z^2) bounds; the results are rounded once to
    fp32.  So |mean - mean64| <= 64 * 2^-24 * E|z| + 2^-24 |mean|, the variance E[z^2] - mean^2 inherits 64 * 2^-24 * (E[z^2] +
    2 |mean| E|z|), and invstd half of that relative to var + eps, plus its own rounding."""
    k = 64 * 2.0 ** -24
    mean_tol = k * r["absmean"] + 2.0 ** -24 * r["mean"].abs()
    var_tol = k * (r["sqmean"] + 2 * r["mean"].abs() * r["absmean"])
    invstd_rel_tol = 0.5 * var_tol / (r["var"] + EPS) + 2.0 ** -23
    return mean_tol, invstd_rel_tol


@pytest.mark.parametrize("form", ["plain", "zeroed_ws", "apply"])
@pytest.mark.parametrize("case", BN_CASES, ids=_bn_id)
def test_bn_forward_forms(case, form):
    """ay_bn_train_fwd_bf16 (workspace pre-filled with NaN), ay_bn_train_fwd_bf16_zeroed_ws and ay_bn_train_apply_bf16 (sums computed
    here in fp64) against F.batch_norm(train) -> LeakyReLU(0.1) | identity -> (+ skip) in float64, rounded once to bf16: y within one
    bf16 ulp + 1e-3 (the bound of test_bn_train_bf16_fwd_bwd_and_plumbing), save_mean / save_invstd against fp64 (_stat_tolerances),
    the running statistics from random starting values at momentum 0.1 and 0.9 (1e-5 / 1e-4 as there), pad lanes exact zeros."""
    B, Cc, H, W, leaky, has_skip = case
    r = _bn_case(case)
    want = r["y"].to(torch.bfloat16).float()
    mean_tol, invstd_rel_tol = _stat_tolerances(r)
    for momentum in (0.1, 0.9):
        yb, mean, invstd, rm, rv = _bn_forward(r, form, momentum)
        got = from_blocked(yb, Cc)
        assert bool(torch.isfinite(got).all()), (form, momentum)
        err = (got - want).abs()
        assert bool((err <= want.abs() * 2.0 ** -7 + 1e-3).all()), (form, float(err.max()))
        if Cc % 16:
            assert bool((yb[:, -1, :, :, Cc % 16:].float().cpu() == 0).all()), "pad lanes of y must be exact zeros"
        rel = (invstd / r["invstd"] - 1).abs()
        print(f"bn stats {_bn_id(case)} {form} momentum {momentum}: worst error / bound: save_mean "
              f"{float(((mean - r['mean']).abs() / mean_tol).max()):.3f}, save_invstd {float((rel / invstd_rel_tol).max()):.3f}")
        assert bool(((mean - r["mean"]).abs() <= mean_tol).all()), (form, float(((mean - r["mean"]).abs() / mean_tol).max()))
        assert bool((rel <= invstd_rel_tol).all()), (form, float((rel / invstd_rel_tol).max()))
        rm_ref, rv_ref = r["running"][momentum]
        assert float((rm - rm_ref).abs().max()) < 1e-5 and float((rv - rv_ref).abs().max()) < 1e-4, \
            (form, momentum, float((rm - rm_ref).abs().max()), float((rv - rv_ref).abs().max()))


@pytest.mark.parametrize("form", ["plain", "acc0", "acc1", "acc1_zeroed_ws"])
@pytest.mark.parametrize("case", BN_CASES, ids=_bn_id)
def test_bn_backward_forms(case, form):
    """ay_bn_train_bwd_bf16, ay_bn_train_bwd_bf16_acc (accumulate 0 and 1; these clear the NaN-filled workspace themselves) and
    ay_bn_train_bwd_bf16_acc_zeroed_ws (the engine's form) against float64 autograd through the reference forward: dz within one bf16
    ulp + 2e-3 and dgamma / dbeta within 1e-3 of the reference maximum (the bounds of test_bn_train_bf16_fwd_bwd_and_plumbing);
    accumulate = 1 must give r + grad for a random r already in dgamma / dbeta, within the same bound plus one fp32 ulp of r;
    accumulate = 0 must overwrite NaN; pad lanes of dz exact zeros.

    The reference's LeakyReLU derivative jumps at pre = 0 and the kernel recomputes pre = (z - mean) * invstd * gamma + beta in fp32
    from fp32-rounded mean / invstd: five roundings of at most 2^-24 each on terms of size |xhat gamma| + |beta| <= 6 * 1.5 + 1.5 here,
    i.e. an error below 5 * 2^-24 * 10.5 = 3.2e-6.  Where |pre| < 4e-6 in the reference the kernel may therefore land on either side
    of the jump: such an element must match one of the two candidates (dpre = dy or 0.1 dy) within the same dz bound, and its largest
    possible contribution (0.9 |dy|, 0.9 |dy xhat|) is added to that channel's dbeta / dgamma allowance.  Every other element is held
    to the reference's own side."""
    B, Cc, H, W, leaky, has_skip = case
    r = _bn_case(case)
    L, dev, st = _lib.lib(), _dev(), _lib.stream_ptr()
    mean, invstd = r["mean"].float().to(dev), r["invstd"].float().to(dev)
    dzb = torch.full_like(r["zb"], float("nan"))
    accumulate = int(form.startswith("acc1"))
    if accumulate:
        dg, db = r["dg0"].clone().to(dev), r["db0"].clone().to(dev)
    else:
        dg, db = torch.full((Cc,), float("nan"), device=dev), torch.full((Cc,), float("nan"), device=dev)
    if form.endswith("zeroed_ws"):
        ws = torch.zeros(2 * Cc, device=dev, dtype=torch.float64)
    else:
        ws = torch.full((2 * Cc,), float("nan"), device=dev, dtype=torch.float64)
    head = (ptr(r["dyb"]), ptr(r["zb"]), ptr(r["gd"]), ptr(r["bd"]), ptr(mean), ptr(invstd), leaky, ptr(dzb), ptr(dg), ptr(db), ptr(ws))
    if form == "plain":
        check(L.ay_bn_train_bwd_bf16(*head, B, Cc, H, W, st), form)
    elif form.endswith("zeroed_ws"):
        check(L.ay_bn_train_bwd_bf16_acc_zeroed_ws(*head, accumulate, B, Cc, H, W, st), form)
    else:
        check(L.ay_bn_train_bwd_bf16_acc(*head, accumulate, B, Cc, H, W, st), form)
    torch.cuda.synchronize()
    near = (r["pre"].abs() < 4e-6) if leaky else torch.zeros_like(r["pre"], dtype=torch.bool)
    xhat = (r["z"].double() - r["mean"].view(1, -1, 1, 1)) * r["invstd"].view(1, -1, 1, 1)
    slack_b = (0.9 * r["dy"].double().abs() * near).sum((0, 2, 3))
    slack_g = (0.9 * (r["dy"].double() * xhat).abs() * near).sum((0, 2, 3))
    gz = from_blocked(dzb, Cc).double()
    assert bool(torch.isfinite(gz).all())
    err = (gz - r["dz"]).abs()
    ok = err <= r["dz"].abs() * 2.0 ** -7 + 2e-3
    # the other side of the jump: dpre changes by -+0.9 dy, dz by gamma * invstd times that (its share in the sums is 1 / n of it)
    side = torch.where(r["pre"] > 0, -0.9, 0.9) * r["dy"].double() * (r["gamma"].double() * r["invstd"]).view(1, -1, 1, 1)
    other = r["dz"] + side
    ok |= near & ((gz - other).abs() <= other.abs() * 2.0 ** -7 + 2e-3)
    assert bool(ok.all()), (form, float(err.max()))
    if Cc % 16:
        assert bool((dzb[:, -1, :, :, Cc % 16:].float().cpu() == 0).all()), "pad lanes of dz must be exact zeros"
    for name, got, ref, r0, slack in (("dgamma", dg, r["dgamma"], r["dg0"], slack_g), ("dbeta", db, r["dbeta"], r["db0"], slack_b)):
        got = got.cpu().double()
        assert bool(torch.isfinite(got).all()), (form, name)
        tol = 1e-3 * float(ref.abs().max()) + slack
        if accumulate:
            ref, tol = ref + r0.double(), tol + _ulp32(r0.double())
        e = (got - ref).abs()
        assert bool((e <= tol).all()), (form, name, float(e.max()), float(ref.abs().max()))


@pytest.mark.parametrize("m", [0, 4, 32])
def test_bn_statistics_under_cancellation(m):
    """E[z^2] - mean^2 on channels whose mean is m standard deviations from zero: z = 0.25 m + 0.25 randn (bf16-rounded) on the
    3-workgroup shape.  Contract: save_invstd within 2^-11 relative of float64 (a quarter of a bf16 half-ulp: y cannot move by more
    than its own rounding), save_mean within 2^-11 std.  The kernel sums z and z^2 in fp32 inside a workgroup (runs of ~20 per thread,
    a tree over 128 lanes) and in fp64 above; emulated on the CPU that order gives 1.8e-5 / 5e-7 / 7e-8 relative for m = 32 / 4 / 0.
    Measured (1.3e-5 at m = 32): profiles/train_bf16_test_margins.txt."""
    case = (2, 32, 96, 96, 1, 0)
    B, Cc, H, W, leaky, _ = case
    r = dict(_bn_case(case))
    g = torch.Generator().manual_seed(77 + m)
    z = bf(m * 0.25 + 0.25 * torch.randn(B, Cc, H, W, generator=g))
    z64 = z.double()
    mean64, var64 = z64.mean((0, 2, 3)), z64.var((0, 2, 3), unbiased=False)
    invstd64 = 1.0 / torch.sqrt(var64 + EPS)
    zb = to_blocked(z, _dev())
    for form in ("zeroed_ws", "plain"):
        yb, mean, invstd, _, _ = _bn_forward(r, form, 0.1, zb=zb)
        e_is = float((invstd / invstd64 - 1).abs().max())
        e_mu = float(((mean - mean64).abs() * invstd64).max())
        print(f"bn cancellation m={m} {form}: invstd rel err {e_is:.3e}, mean err / std {e_mu:.3e} (bound {2.0 ** -11:.3e})")
        assert e_is <= 2.0 ** -11 and e_mu <= 2.0 ** -11, (form, e_is, e_mu)
        pre = (z64 - mean64.view(1, -1, 1, 1)) * invstd64.view(1, -1, 1, 1) * r["gamma"].double().view(1, -1, 1, 1) + r["beta"].double().view(1, -1, 1, 1)
        want = F.leaky_relu(pre, 0.1).to(torch.bfloat16).float()
        err = (from_blocked(yb, Cc) - want).abs()
        assert bool((err <= want.abs() * 2.0 ** -7 + 1e-3).all()), (form, float(err.max()))


# ------------------------------------------------------------------------------------------------------- weight gradient
# (cin, cout, k, stride, H, B): one per kernel instantiation, each with a split-K count that is a multiple of 8 (the XCD remapping of
# workgroups to slices) and a group count that the split does not divide (slices of unequal length, a half-empty last group)
WGRAD_KS8_CASES = [(64, 256, 3, 1, 65, 3), (32, 64, 3, 1, 67, 3), (128, 256, 3, 2, 66, 3), (32, 64, 3, 2, 66, 3), (256, 128, 1, 1, 67, 3),
                   (128, 64, 1, 1, 105, 2), (64, 32, 1, 1, 105, 2)]


@pytest.mark.parametrize("case", WGRAD_KS8_CASES, ids=lambda c: "x".join(map(str, c)))
def test_wgrad_split_k_slices_of_8(case):
    """ay_conv_wgrad_bf16 / _acc(accumulate=1) / _ws (full workspace, accumulate 0 and 1; one byte short: the atomics path) at ks >= 8,
    against the filter gradient of F.conv2d on the same bf16 operands in float64.

    Bound: 8 x the error of torch's own fp32 filter gradient against the float64 one -- the reference's noise, with room for another
    summation order (2e-3 of max|dW| would be the size of one lost pixel at ~12 000 pixels per tap).  That bound must itself stay
    below a quarter of what ONE zeroed output pixel of dz changes in dW (asserted per case): a dropped segment cannot hide in it.
    On top, for results held in fp32 next to a pre-fill r: one fp32 ulp of the result."""
    cin, cout, k, s, H, B = case
    L, dev, st = _lib.lib(), _dev(), _lib.stream_ptr()
    pad = (k - 1) // 2
    Ho = (H + 2 * pad - k) // s + 1
    g = torch.Generator().manual_seed(7 * cin + cout + H)
    x = bf(torch.randn(B, cin, H, H, generator=g))
    dz = bf(torch.randn(B, cout, Ho, Ho, generator=g))
    r0 = torch.randn(cout, cin, k, k, generator=g)
    threads = torch.get_num_threads()
    try:    # one thread: the fp32 reference's summation order, and with it `noise`, does not depend on how the host splits the work
        torch.set_num_threads(1)
        ref32 = torch.nn.grad.conv2d_weight(x, (cout, cin, k, k), dz, s, pad).double()     # autograd's filter gradient of F.conv2d
    finally:
        torch.set_num_threads(threads)
    ref64 = torch.nn.grad.conv2d_weight(x.double(), (cout, cin, k, k), dz.double(), s, pad)
    noise = float((ref32 - ref64).abs().max())
    bound = 8 * noise
    # one output pixel of dz zeroed: dW changes by the outer product of that pixel's dz and its input window, whose largest entry is
    # max|dz| * max|window|; the weakest of ALL output pixels counts (windows over the zero padding included)
    xwin = F.max_pool2d(F.pad(x.abs().amax(1, keepdim=True), (pad,) * 4), k, s)
    assert xwin.shape[-2:] == (Ho, Ho)
    one_pixel = float((dz.abs().amax(1, keepdim=True) * xwin).min())
    assert bound < 0.25 * one_pixel, (bound, one_pixel)

    cpad = (cout + 31) // 32 * 32
    xb, dzb = to_blocked(x, dev), to_blocked(dz, dev, cpad)
    d = ConvDesc(B, cin, cout, H, H, Ho, Ho, k, s, 0, 0, cpad)
    n_el = cout * cin * k * k
    nws = L.ay_conv_wgrad_workspace_bytes(C.byref(d))
    assert nws % (4 * n_el) == 0
    ks = nws // (4 * n_el)
    assert ks >= 8 and ks % 8 == 0, f"ks = {ks}: the case left the slice-remapping branch of wgrad_bf16_kernel (adjust H)"
    ratios = {}

    def judge(name, got, extra=0.0):
        assert bool(torch.isfinite(got).all()), name
        e = float((got.double() - ref64).abs().max())
        ratios[name] = e / noise
        assert e <= bound + extra, (name, e, bound, extra)

    nan = lambda: torch.full((cout, cin, k, k), float("nan"), device=dev)  # noqa: E731
    dw = nan()
    check(L.ay_conv_wgrad_bf16(C.byref(d), ptr(xb), ptr(dzb), ptr(dw), st), "wgrad")
    judge("atomics", dw.cpu())
    dwa = r0.clone().to(dev)
    check(L.ay_conv_wgrad_bf16_acc(C.byref(d), ptr(xb), ptr(dzb), ptr(dwa), 1, st), "wgrad_acc")
    ulp_res = 2.0 ** -23 * float((ref64 + r0.double()).abs().max())
    judge("atomics onto r", dwa.cpu().double() - r0.double(), ulp_res)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    runs = []
    for _ in range(2):
        dw2 = nan()
        check(L.ay_conv_wgrad_bf16_ws(C.byref(d), ptr(xb), ptr(dzb), ptr(dw2), 0, ptr(ws), ws.numel(), st), "wgrad_ws")
        runs.append(dw2.cpu())
    assert torch.equal(runs[0], runs[1]), "slab reduction is not reproducible"
    judge("slabs", runs[0])
    dw3 = torch.zeros(cout, cin, k, k, device=dev)
    check(L.ay_conv_wgrad_bf16_ws(C.byref(d), ptr(xb), ptr(dzb), ptr(dw3), 1, ptr(ws), ws.numel(), st), "wgrad_ws acc")
    assert torch.equal(dw3.cpu(), runs[0]), "accumulate onto zeros must give the bits of accumulate = 0"
    dw4 = r0.clone().to(dev)
    check(L.ay_conv_wgrad_bf16_ws(C.byref(d), ptr(xb), ptr(dzb), ptr(dw4), 1, ptr(ws), ws.numel(), st), "wgrad_ws acc")
    assert torch.equal(dw4.cpu(), runs[0] + r0), "accumulate = 1 is one fp32 add of the fixed-order slab sum onto dW"
    dw5 = nan()
    check(L.ay_conv_wgrad_bf16_ws(C.byref(d), ptr(xb), ptr(dzb), ptr(dw5), 0, ptr(ws), ws.numel() - 1, st), "wgrad_ws short")
    judge("workspace one byte short", dw5.cpu())
    print(f"wgrad {'x'.join(map(str, case))}: ks {ks}, fp32 reference noise {noise:.3e}, one pixel {one_pixel:.3e}, error / noise: "
          + ", ".join(f"{n} {v:.2f}" for n, v in ratios.items()))


# --------------------------------------------------------------------------------------------------- batched filter packer
def test_pack_batch_against_single_packers():
    """ay_pack_batch_bf16 (one launch over a job table, what a training step uses) against ay_pack_conv_weights_bf16,
    ay_pack_dgrad_weights_bf16 and ay_pack_dgrad_s2_weights_bf16: byte equality over what those write, bytes past a job's total
    untouched; and the single packers (ay_pack_conv_weights_f16 too) byte for byte against the documented layouts built in NumPy
    (tests/pack_reference.py).  Jobs with padded output and input channels, totals below one block and off a multiple of it; work
    items in a scrambled order (they are independent)."""
    L, dev, st = _lib.lib(), _dev(), _lib.stream_ptr()
    blk = L.ay_pack_batch_block()
    g = torch.Generator().manual_seed(5)
    # (kind, cout, cout_pad, cin, cin_pad, k)
    specs = [(0, 24, 32, 64, 0, 1), (0, 256, 256, 128, 0, 3), (0, 128, 256, 128, 0, 3), (0, 12, 16, 16, 0, 3),
             (1, 24, 32, 48, 64, 1), (1, 24, 32, 48, 64, 3), (1, 10, 16, 20, 32, 1), (1, 10, 16, 20, 32, 3),
             (2, 80, 96, 48, 64, 3)]
    TAIL = 4096
    jobs, keep, want = [], [], []
    for kind, cout, cout_pad, cin, cin_pad, k in specs:
        w = torch.randn(cout, cin, k, k, generator=g).to(dev)
        if kind == 0:
            nbytes = L.ay_packed_weight_bytes(cout_pad, cin, k)
        elif kind == 1:
            assert cout_pad == (cout + 15) // 16 * 16
            nbytes = L.ay_packed_dgrad_weight_bytes(cout, cin_pad, k)
        else:
            nbytes = L.ay_packed_dgrad_s2_weight_bytes(cout_pad, cin_pad)
        single = torch.full((nbytes + TAIL,), 0xFF, device=dev, dtype=torch.uint8)
        if kind == 0:
            check(L.ay_pack_conv_weights_bf16(ptr(w), ptr(single), cout, cout_pad, cin, k, st))
        elif kind == 1:
            check(L.ay_pack_dgrad_weights_bf16(ptr(w), ptr(single), cout, cin, cin_pad, k, st))
        else:
            check(L.ay_pack_dgrad_s2_weights_bf16(ptr(w), ptr(single), cout, cout_pad, cin, cin_pad, st))
        dst = torch.full((nbytes + TAIL,), 0xFF, device=dev, dtype=torch.uint8)
        jobs.append((w.data_ptr(), dst.data_ptr(), kind, cout, cout_pad, cin, cin_pad, k, nbytes // 2))
        keep.append((w, dst))
        want.append(single)
    totals = [j[8] for j in jobs]
    assert any(t < blk for t in totals) and any(t % blk for t in totals if t > blk) and any(t % blk == 0 for t in totals)
    job_dt = np.dtype([("src", "<u8"), ("dst", "<u8"), ("kind", "<i4"), ("cout", "<i4"), ("cout_pad", "<i4"), ("cin", "<i4"),
                       ("cin_pad", "<i4"), ("ksize", "<i4"), ("total", "<u8")])      # ay_pack_job (include/amyloid_yolo.h)
    work_dt = np.dtype([("job", "<u4"), ("first", "<u4")])                           # ay_pack_work
    assert job_dt.itemsize == 48 and work_dt.itemsize == 8
    items = [(j, b) for j, t in enumerate(totals) for b in range((t + blk - 1) // blk)]
    items = [items[i] for i in np.random.default_rng(3).permutation(len(items))]
    jd = torch.from_numpy(np.array(jobs, dtype=job_dt).view(np.uint8).copy()).to(dev)
    wd = torch.from_numpy(np.array(items, dtype=work_dt).view(np.uint8).copy()).to(dev)
    check(L.ay_pack_batch_bf16(ptr(jd), ptr(wd), len(items), st), "ay_pack_batch_bf16")
    torch.cuda.synchronize()
    for spec, (w, dst), single, t in zip(specs, keep, want, totals):
        a, b_ = dst.cpu(), single.cpu()
        assert bool((b_[2 * t:] == 0xFF).all()), spec                       # the single packer wrote exactly `total` elements
        assert bool((b_[: 2 * t].view(torch.int16) != -1).all())            # ... every one of them (0xFFFF is no packed value)
        assert torch.equal(a[: 2 * t], b_[: 2 * t]), (spec, int((a[: 2 * t] != b_[: 2 * t]).sum()))
        assert bool((a[2 * t:] == 0xFF).all()), (spec, "bytes past the job's total were written")
        kind, cout, cout_pad, cin, cin_pad, k = spec
        wn = w.cpu().numpy()
        ref = (pack_reference.forward_image(wn, cout_pad) if kind == 0 else pack_reference.dgrad_image(wn, cin_pad) if kind == 1
               else pack_reference.dgrad_s2_images(wn, cout_pad, cin_pad))
        assert np.array_equal(b_[: 2 * t].numpy().view(np.uint16), pack_reference.bits(ref)), (spec, "single packer against the documented layout")
    cout, cout_pad, cin, k = 12, 16, 16, 3           # the IEEE-half forward image
    w = torch.randn(cout, cin, k, k, generator=g)
    nbytes = L.ay_packed_weight_bytes(cout_pad, cin, k)
    half = torch.full((nbytes + TAIL,), 0xFF, device=dev, dtype=torch.uint8)
    check(L.ay_pack_conv_weights_f16(ptr(w.to(dev)), ptr(half), cout, cout_pad, cin, k, st))
    half = half.cpu()
    assert bool((half[nbytes:] == 0xFF).all())
    assert np.array_equal(half[:nbytes].numpy().view(np.uint16), pack_reference.bits(pack_reference.forward_image(w.numpy(), cout_pad), "f16"))


# ------------------------------------------------------------------------------------------------------------ bias gradient
@pytest.mark.parametrize("shape", [(3, 24, 13, 13), (3, 5, 75, 75)], ids=str)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_bias_grad_acc(shape, accumulate):
    """ay_bias_grad_f32_acc (the head layers' bias gradient on the bf16 path: partial sums per chunk of 16384 pixels combined by fp32
    atomics) against dz.sum((0, 2, 3)) in float64, plus what dbias held (accumulate = 1) or over NaN (accumulate = 0).  hw off a
    multiple of 64; the second shape has two chunks whose boundary falls inside an image.  Bound: every value passes through at most
    ceil(pixels per chunk / 256) sequential fp32 adds in its thread, a block reduction (8 levels) and the chunks' atomics, each
    rounding at most 2^-24 of a partial sum bounded by sum|dz|; plus one fp32 ulp of the pre-fill."""
    B, Cc, H, W = shape
    L, dev, st = _lib.lib(), _dev(), _lib.stream_ptr()
    g = torch.Generator().manual_seed(H + Cc)
    dz = torch.randn(B, Cc, H, W, generator=g)
    r0 = torch.randn(Cc, generator=g) * 10
    n = B * H * W
    chunks = (n + 16383) // 16384
    assert (H * W) % 64 != 0
    ref = dz.double().sum((0, 2, 3))
    tol = (math.ceil(n / chunks / 256) + 8 + chunks) * 2.0 ** -24 * dz.double().abs().sum((0, 2, 3))
    db = r0.clone().to(dev) if accumulate else torch.full((Cc,), float("nan"), device=dev)
    dzd = dz.to(dev)
    check(L.ay_bias_grad_f32_acc(ptr(dzd), ptr(db), accumulate, B, Cc, H * W, st), "ay_bias_grad_f32_acc")
    got = db.cpu().double()
    if accumulate:
        ref, tol = ref + r0.double(), tol + _ulp32(ref + r0.double())
    assert bool(torch.isfinite(got).all())
    assert bool(((got - ref).abs() <= tol).all()), float(((got - ref).abs() / tol).max())


# ------------------------------------------------------------------------------------- gradient accumulation through the engine
@pytest.fixture(scope="module")
def engine(tmp_cfg_dir):
    """Darknet(precision="bf16") with the synthetic weights of the step test, and a copy of its buffers (BN running statistics);
    released with its device memory when the module is done"""
    from amyloid_yolo_paper_amd import cfg_gen, parse_config, synth
    from amyloid_yolo_paper_amd.models import Darknet
    C_ = 3
    cfg = cfg_gen.write_cfg(C_, tmp_cfg_dir)
    defs = parse_config.parse_model_config(cfg)
    wpath = os.path.join(tmp_cfg_dir, f"synth_c{C_}.weights")
    if not os.path.exists(wpath):
        synth.write_darknet_weights(wpath, defs, synth.synth_params(defs, seed=7), seen=0)
    m = Darknet(cfg, precision="bf16").to("cuda")
    m.load_darknet_weights(wpath)
    m.train()
    yield m, {k: v.detach().clone() for k, v in m.named_buffers()}
    del m
    torch.cuda.empty_cache()


def _batch(B, S, start, seed):
    from amyloid_yolo_paper_amd import synth
    x = torch.from_numpy(synth.synth_tiles(B, S, start))
    tg = torch.from_numpy(synth.synth_targets(B, 3, seed=seed, max_per_tile=6, min_per_tile=3, wh_range=(0.05, 0.4), grid=S // 8))
    return x, tg


def _grads_after(m, buffers, batches):
    """p.grad after forward / backward over `batches` from zeroed gradients, with NO zero_grad() in between; the BN running statistics
    start from the loaded ones every time"""
    with torch.no_grad():
        for k, v in m.named_buffers():
            v.copy_(buffers[k])
    for p in m.parameters():
        p.grad = None      # the backward creates zeros where a gradient is missing
    for x, tg in batches:
        loss, _ = m(x, tg)
        assert bool(torch.isfinite(loss))
        loss.backward()
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters()}


def _worst_rel_l2(got, want):
    worst, where = 0.0, None
    for n, w in want.items():
        assert bool(torch.isfinite(got[n]).all()), n
        rel = float((got[n].double() - w.double()).norm() / (w.double().norm() + 1e-300))
        if rel > worst:
            worst, where = rel, n
    return worst, where


@pytest.mark.parametrize("S_b", [96, 128], ids=["same_shape", "two_contexts"])
def test_gradient_accumulation_through_engine(engine, S_b):
    """Two backward passes without zero_grad() leave g_a + g_b in every p.grad (train.py:116-119, gradient_accumulations > 1): the
    kernels ADD into p.grad (accumulate = 1 everywhere), from one (B, S) context or -- multiscale training -- from two.  g_a and g_b
    come from separate steps on zeroed gradients.  Bound: relative L2 per tensor of max(4 x the run-to-run difference of g_a between
    two identical zeroed steps, 1e-6) (train_engine_bf16.py records the first step as reproducible to 2e-6; the sum of two fp32
    gradients and the kernels' in-place add round alike)."""
    m, buffers = engine
    m.__dict__.pop("_train_ctx", None)     # each case builds its own (B, S) contexts (train_engine_bf16._context keeps them here)
    a, b = _batch(2, 96, 10, 21), _batch(2, S_b, 20, 22)
    g_a = _grads_after(m, buffers, [a])
    assert len(m.__dict__.get("_train_ctx", ())) == 1, "the engine no longer keeps its contexts in model._train_ctx: fix the reset above"
    g_a2 = _grads_after(m, buffers, [a])
    g_b = _grads_after(m, buffers, [b])
    g_ab = _grads_after(m, buffers, [a, b])
    assert len(m.__dict__["_train_ctx"]) == (1 if S_b == 96 else 2)
    assert all(float(g.abs().max()) > 0 for g in g_a.values()) and all(float(g.abs().max()) > 0 for g in g_b.values())
    repeat, where_r = _worst_rel_l2(g_a2, g_a)
    err, where_e = _worst_rel_l2(g_ab, {n: g_a[n] + g_b[n] for n in g_a})
    bound = max(4 * repeat, 1e-6)
    print(f"gradient accumulation S_b={S_b}: run-to-run rel L2 of g_a {repeat:.3e} ({where_r}), |acc - (g_a + g_b)| rel L2 {err:.3e} "
          f"({where_e}), bound {bound:.3e}")
    assert err <= bound, (err, bound, where_e)
