"""The ring convolution kernels across ITEM BOUNDARIES: every workgroup works through several items, so the loader state that
runs ahead of the MFMA side (next item's descriptors and lane offsets, the scale/shift region, the mailbox sequence) and the
waits that order DMA pieces against the epilogue's stores are exercised -- test_conv_bf16_kernel gives each workgroup one item.

Each case goes through the C ABI and is held to test_conv_bf16_kernel's bar: torch-CPU fp32 convolution of the operands rounded
to the storage type (+affine, leaky, residual), rounded once; 1 ulp of the result (2^-7 relative for bf16, 2^-10 for half) + 1e-3
(half: 2e-4) absolute.  The batch repeats a few distinct images, so the reference is computed once per distinct image.  On top:
  * guard bands: input and residual lie inside larger buffers whose surroundings hold NaNs, the output inside a buffer of a
    sentinel pattern that must come back untouched (a descriptor range or lane offset that is off by a row reads a neighbour,
    or a NaN, instead of zero);
  * repeat: two calls into two outputs give the same bits (a wait that lets a piece land late shows as a difference);
  * image independence: image b of the batch has the bits of the same image run alone -- and of every other copy of it.

The persistent kernels beside the plain ring (stride-2 data gradient, fused residual block, fused stem, training stem) go through
the same harness with the bounds of their own tests; their batches are sized from the device's CU count so that every workgroup
the launch can start gets at least 8 items (_batch_for)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ConvDesc, check, ptr

gpu = pytest.mark.gpu
U = 4               # distinct images of a batch
GUARD = 8192        # elements on either side of a tensor
SENTINEL = 0x5A5A   # output fill: 1.5e16 as bfloat16, 203.25 as half -- no convolution of these operands comes near either


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def _tdt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float16


def _guarded(shape, tdt, dev, fill):
    """(whole buffer, view of `shape` in its middle); the buffer holds `fill` (NaN, or the sentinel bit pattern)"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, device=dev, dtype=tdt)
    if fill is None:
        buf.fill_(float("nan"))
    else:
        buf.view(torch.int16).fill_(fill)
    return buf, buf[GUARD:GUARD + n].view(shape)


def _guards_intact(buf, n):
    raw = buf.view(torch.int16)
    return bool((raw[:GUARD] == SENTINEL).all()) and bool((raw[GUARD + n:] == SENTINEL).all())


def _blocked_in(L, dtype, x_unique, B, dev, st):
    """the batch (image b = distinct image b % U) in the blocked layout, inside NaN guard bands"""
    tdt = _tdt(dtype)
    _, c, h, w = x_unique.shape
    xd = x_unique.to(dev).repeat((B + U - 1) // U, 1, 1, 1)[:B].contiguous()
    buf, xb = _guarded((B, c // 16, h, w, 16), tdt, dev, None)
    check(getattr(L, f"ay_nchw_f32_to_blocked_{dtype}")(ptr(xd), ptr(xb), B, c, h, w, st))
    torch.cuda.synchronize()
    return buf, xb


def _verify(L, dtype, run, out_shape, cout, ref_unique, B, dev, st, accept=None):
    """run(out, b0, nb): the call under test on images b0 .. b0 + nb - 1 into `out` ([nb] + out_shape[1:]); accept(got, ref): the
    bound of an entry point whose own test sets another one than the convolutions' (ref: rounded to the storage type)"""
    tdt = _tdt(dtype)
    n = int(np.prod(out_shape))
    buf1, o1 = _guarded(out_shape, tdt, dev, SENTINEL)
    buf2, o2 = _guarded(out_shape, tdt, dev, SENTINEL)
    run(o1, 0, B)
    run(o2, 0, B)
    torch.cuda.synchronize()
    assert _guards_intact(buf1, n) and _guards_intact(buf2, n), "output guard band overwritten"
    r1, r2 = o1.view(torch.int16), o2.view(torch.int16)
    assert torch.equal(r1, r2), "two calls differ"
    # against the reference: the U distinct images ...
    Ho, Wo = out_shape[2], out_shape[3]
    got = torch.empty(U, cout, Ho, Wo, device=dev)
    check(getattr(L, f"ay_blocked_{dtype}_to_nchw_f32")(ptr(o1), ptr(got), U, cout, Ho, Wo, st))
    got = got.cpu()
    assert bool(torch.isfinite(got).all())
    ref = ref_unique.to(tdt).to(torch.float32)
    if accept is not None:
        accept(got, ref)
    else:
        err = (got - ref).abs()
        bound = ref.abs() * 2.0 ** -7 + 1e-3 if dtype == "bf16" else ref.abs() * 2.0 ** -10 + 2e-4
        assert bool((err <= bound).all()), float((err - bound).max())
    # ... and every further image has the bits of its first copy
    for b in range(U, B):
        assert torch.equal(r1[b], r1[b % U]), f"image {b} differs from image {b % U}"
    # one image run alone (the last: its items are the last of their workgroups)
    buf3, o3 = _guarded((1,) + tuple(out_shape[1:]), tdt, dev, SENTINEL)
    run(o3, B - 1, 1)
    torch.cuda.synchronize()
    assert _guards_intact(buf3, n // B)
    assert torch.equal(o3.view(torch.int16)[0], r1[B - 1]), "image run alone differs"


def _conv_case(dev, dtype, cin, cout, k, stride, H, B, has_res=False, entry="ay_conv_fwd"):
    L = _lib.lib()
    st = _lib.stream_ptr()
    tdt = _tdt(dtype)
    rnd = lambda t: t.to(tdt).to(torch.float32)
    g = torch.Generator().manual_seed(cin * 7 + cout + k + H + stride)
    x = rnd(torch.randn(U, cin, H, H, generator=g))
    w = torch.randn(cout, cin, k, k, generator=g) * (1.0 / np.sqrt(cin * k * k))
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    pad = (k - 1) // 2
    Ho = (H + 2 * pad - k) // stride + 1
    res = rnd(torch.randn(U, cout, Ho, Ho, generator=g)) if has_res else None
    ref = F.leaky_relu(F.conv2d(x, rnd(w), None, stride, pad) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), 0.1)
    if has_res:
        ref = ref + res
    assert cout % 32 == 0
    xbuf, xb = _blocked_in(L, dtype, x, B, dev, st)
    rbuf, rb = _blocked_in(L, dtype, res, B, dev, st) if has_res else (None, None)
    wd = w.to(dev)
    packed = torch.empty(L.ay_packed_weight_bytes(cout, cin, k), device=dev, dtype=torch.uint8)
    check(getattr(L, f"ay_pack_conv_weights_{dtype}")(ptr(wd), ptr(packed), cout, cout, cin, k, st))
    sc, sh = scale.to(dev), shift.to(dev)
    fn = getattr(L, f"{entry}_{dtype}")

    def run(out, b0, nb):
        d = ConvDesc(nb, cin, cout, H, H, Ho, Ho, k, stride, 1, 0, cout)
        check(fn(C.byref(d), ptr(xb[b0:b0 + nb]), ptr(packed), ptr(sc), ptr(sh), ptr(rb[b0:b0 + nb]) if has_res else None, ptr(out), st), entry)

    _verify(L, dtype, run, (B, cout // 16, Ho, Ho, 16), cout, ref, B, dev, st)


RING_CASES = [
    # cin, cout, k, stride, H, batch
    (32, 128, 3, 2, 128, 48),    # stride 2, two slots: 64^2 out, 16 tiles per image, 768 items of two stages
    (16, 128, 3, 2, 66, 40),     # stride 2, two slots, a single stage per item, ragged 33^2 out (tiled as a canvas of 10 images per row)
    (64, 256, 1, 1, 64, 50),     # 1x1, 256-channel tile, two slots: one stage per item, 800 items
    (128, 256, 1, 1, 64, 50),    # the same with two stages
    (512, 512, 1, 1, 32, 100),   # 256-channel tile, two channel groups
    (128, 128, 1, 1, 64, 50),    # 1x1 with three slots
    (128, 256, 3, 2, 26, 493),   # stride 2 on the canvas (test_conv_bf16_kernel's row, batch raised to 770 items; last canvas row part empty)
]


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", RING_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_ring_kernel_across_items(dev, case, dtype):
    cin, cout, k, stride, H, B = case
    _conv_case(dev, dtype, cin, cout, k, stride, H, B)


M16_CASES = [
    # cin, cout, H, batch, residual
    (32, 128, 64, 100, False),   # one stage pair per item: the loader wraps to the next item inside every item
    (32, 128, 64, 100, True),
    (64, 128, 64, 100, False),   # 8 tiles per image, 800 items
    (64, 128, 64, 100, True),
    (64, 128, 40, 48, True),     # ragged: tile rows 16 + 16 + 8, columns 32 + 8 (6 tiles per image, 288 items)
]


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", M16_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_m16_kernel_across_items(dev, case, dtype):
    cin, cout, H, B, has_res = case
    _conv_case(dev, dtype, cin, cout, 3, 1, H, B, has_res, entry="ay_conv3x3_m16_fwd")


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_cat_kernel_across_items(dev, dtype):
    """route [upsampled x2 | direct] folded into the 1x1: two sources, two descriptors, one offset array each"""
    c1, c2, cout, H, B = 64, 64, 128, 32, 100   # 4 tiles per image, 400 items of two stages
    L = _lib.lib()
    st = _lib.stream_ptr()
    tdt = _tdt(dtype)
    rnd = lambda t: t.to(tdt).to(torch.float32)
    g = torch.Generator().manual_seed(c1 + c2 + H)
    a_half = rnd(torch.randn(U, c1, H // 2, H // 2, generator=g))
    b_full = rnd(torch.randn(U, c2, H, H, generator=g))
    w = torch.randn(cout, c1 + c2, 1, 1, generator=g) * (1.0 / np.sqrt(c1 + c2))
    scale, shift = torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1
    ref = F.conv2d(torch.cat([F.interpolate(a_half, scale_factor=2, mode="nearest"), b_full], 1), rnd(w))
    ref = F.leaky_relu(ref * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1), 0.1)
    abuf, ab = _blocked_in(L, dtype, a_half, B, dev, st)
    bbuf, bb = _blocked_in(L, dtype, b_full, B, dev, st)
    wd, sc, sh = w.to(dev), scale.to(dev), shift.to(dev)
    packed = torch.empty(L.ay_packed_weight_bytes(cout, c1 + c2, 1), device=dev, dtype=torch.uint8)
    check(getattr(L, f"ay_pack_conv_weights_{dtype}")(ptr(wd), ptr(packed), cout, cout, c1 + c2, 1, st))
    fn = getattr(L, f"ay_conv1x1_cat_fwd_{dtype}")

    def run(out, b0, nb):
        d = ConvDesc(nb, c1 + c2, cout, H, H, H, H, 1, 1, 1, 0, cout)
        check(fn(C.byref(d), ptr(ab[b0:b0 + nb]), c1, ptr(bb[b0:b0 + nb]), ptr(packed), ptr(sc), ptr(sh), ptr(out), st), "cat")

    _verify(L, dtype, run, (B, cout // 16, H, H, 16), cout, ref, B, dev, st)


def _batch_for(items_per_image, wgs_per_cu=1):
    """(batch, items, workgroups): the smallest multiple of U images that gives every workgroup a persistent launch can start --
    8 XCDs x min(items per XCD, wgs_per_cu x CUs per XCD), CUs rounded down to a multiple of 8 -- at least 8 items"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cus -= cus % 8
    B = -(-8 * wgs_per_cu * cus // items_per_image)
    B += -B % U
    n_items = B * items_per_image
    wgs = 8 * min(-(-n_items // 8), wgs_per_cu * cus // 8)
    assert n_items >= 8 * wgs, (n_items, wgs)
    return B, n_items, wgs


def _guarded_f32(t_unique, B, dev):
    """the batch (image b = distinct image b % U) as fp32 NCHW inside NaN guard bands"""
    buf, v = _guarded((B,) + tuple(t_unique.shape[1:]), torch.float32, dev, None)
    v.copy_(t_unique.to(dev).repeat((B + U - 1) // U, 1, 1, 1)[:B])
    return buf, v


@gpu
@pytest.mark.parametrize("has_prev", [False, True], ids=["plain", "prev"])
@pytest.mark.parametrize("cin_pad", [32, 64, 128])
def test_dgrad_s2_across_items(dev, cin_pad, has_prev):
    """ay_conv_dgrad_s2_bf16 at hout = 16 with every tile form: pair tile 16x32 of 32 real channels (cin_pad 32), pair tile 8x32
    of 64 (cin_pad 64), class tile 8x32 of 128 (cin_pad 128); the parity class rides in the item's group index.  64 channels of
    dz = two stages per item = fetch-ahead distance 3: the first three items of a workgroup are static, the others -- most of
    them, asserted -- come from the counter.  Reference and bound of test_dgrad_s2_parity_classes: autograd through
    F.conv2d(stride=2) on the rounded filters, |ref| 2^-7 + 2e-3.  With a previous gradient dx is read and written in place, as
    the training step does."""
    L = _lib.lib()
    st = _lib.stream_ptr()
    cin, cout, Ho = cin_pad, 64, 16
    H = 2 * Ho
    th, real, classes = {32: (16, 32, 2), 64: (8, 64, 2), 128: (8, 128, 4)}[cin_pad]
    n_cgroups = classes * cin_pad // real
    B, n_items, wgs = _batch_for(-(-Ho // th) * -(-Ho // 32) * n_cgroups)
    assert n_items - 3 * wgs > n_items // 2, "most items are dealt by the counter"
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    g = torch.Generator().manual_seed(cin_pad * 5 + cout + H)
    w = torch.randn(cout, cin, 3, 3, generator=g) / np.sqrt(cout * 9 / 4)
    x = torch.zeros(U, cin, H, H, requires_grad=True)
    y = F.conv2d(x, bf(w), None, 2, 1)
    dz = bf(torch.randn(y.shape, generator=g))
    y.backward(dz)
    prev = bf(torch.randn(U, cin, H, H, generator=g))
    ref = x.grad + prev if has_prev else x.grad
    zbuf, zb = _blocked_in(L, "bf16", dz, B, dev, st)
    pbuf, pb = _blocked_in(L, "bf16", prev, B, dev, st) if has_prev else (None, None)
    packed = torch.empty(L.ay_packed_dgrad_s2_weight_bytes(cout, cin_pad), device=dev, dtype=torch.uint8)
    check(L.ay_pack_dgrad_s2_weights_bf16(ptr(w.to(dev)), ptr(packed), cout, cout, cin, cin_pad, st))
    ones, zeros = torch.ones(cin_pad, device=dev), torch.zeros(cin_pad, device=dev)

    def run(out, b0, nb):
        if has_prev:
            out.copy_(pb[b0:b0 + nb])
        d = ConvDesc(nb, cin, cout, H, H, Ho, Ho, 3, 2, 0, 0, cout)
        check(L.ay_conv_dgrad_s2_bf16(C.byref(d), ptr(zb[b0:b0 + nb]), ptr(packed), ptr(ones), ptr(zeros), ptr(out) if has_prev else None,
                                      ptr(out), cin_pad, st), "dgrad s2")

    def accept(got, ref):
        err = (got - ref).abs()
        print("dgrad s2 max error", float(err.max()))
        assert bool((err <= ref.abs() * 2.0 ** -7 + 2e-3).all()), float(err.max())

    _verify(L, "bf16", run, (B, cin_pad // 16, H, H, 16), cin, ref, B, dev, st, accept)


@gpu
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", [(64, 16, 16), (128, 8, 32)], ids=lambda c: "x".join(str(v) for v in c))
def test_resblock_across_items(dev, case, dtype):
    """ay_resblock_fwd_{bf16,f16}, one item per image (C = 64: the 16x32 tile, C = 128: the 8x32 tile), static dealing: the loader
    runs across phase and item boundaries.  Reference and bound of test_resblock_fused_kernel for the torch-CPU composition: the
    share of elements above |ref| 2^-6 + 2e-3 is at most 1e-3.
    The cap against this seed, checked on the CPU: the same composition in float64 (intermediate and result rounded to bf16 at
    the same points) differs from the rounded fp32 reference in 61 of 65 536 elements (C = 64) and 42 of 131 072 (C = 128), by
    one ulp each (0.0156 at |ref| = 2.28 where the bound is 0.0376; 0.0078 at 1.98, bound 0.0329): a share of 0 above the bound,
    so the cap of 1e-3 is all the kernel's own.  In half precision: 80 and 276 elements, 0.00195 at most, share 0 as well."""
    Cc, H, W = case
    CM = Cc // 2
    L = _lib.lib()
    st = _lib.stream_ptr()
    tdt = _tdt(dtype)
    rnd = lambda t: t.to(tdt).to(torch.float32)
    B, n_items, wgs = _batch_for(1)
    g = torch.Generator().manual_seed(Cc * 3 + H)
    x = rnd(torch.randn(U, Cc, H, W, generator=g))
    w1 = torch.randn(CM, Cc, 1, 1, generator=g) * (1.0 / np.sqrt(Cc))
    w2 = torch.randn(Cc, CM, 3, 3, generator=g) * (1.0 / np.sqrt(CM * 9))
    s1, t1 = torch.rand(CM, generator=g) + 0.5, torch.randn(CM, generator=g) * 0.1
    s2, t2 = torch.rand(Cc, generator=g) + 0.5, torch.randn(Cc, generator=g) * 0.1
    mid = rnd(F.leaky_relu(F.conv2d(x, rnd(w1)) * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1), 0.1))
    ref = F.leaky_relu(F.conv2d(mid, rnd(w2), None, 1, 1) * s2.view(1, -1, 1, 1) + t2.view(1, -1, 1, 1), 0.1) + x
    xbuf, xb = _blocked_in(L, dtype, x, B, dev, st)
    w1d, w2d = w1.to(dev), w2.to(dev)
    p1 = torch.empty(L.ay_packed_weight_bytes(CM, Cc, 1), device=dev, dtype=torch.uint8)
    p2 = torch.empty(L.ay_packed_weight_bytes(Cc, CM, 3), device=dev, dtype=torch.uint8)
    check(getattr(L, f"ay_pack_conv_weights_{dtype}")(ptr(w1d), ptr(p1), CM, CM, Cc, 1, st))
    check(getattr(L, f"ay_pack_conv_weights_{dtype}")(ptr(w2d), ptr(p2), Cc, Cc, CM, 3, st))
    s1d, t1d, s2d, t2d = s1.to(dev), t1.to(dev), s2.to(dev), t2.to(dev)
    fn = getattr(L, f"ay_resblock_fwd_{dtype}")

    def run(out, b0, nb):
        check(fn(ptr(xb[b0:b0 + nb]), ptr(p1), ptr(s1d), ptr(t1d), 1, ptr(p2), ptr(s2d), ptr(t2d), 1, ptr(out), nb, Cc, H, W, st), "resblock")

    def accept(got, ref):
        err = (got - ref).abs()
        share = float((err > ref.abs() * 2.0 ** -6 + 2e-3).float().mean())
        print("resblock share above the bound", share, "max error", float(err.max()))
        assert share <= 1e-3, (share, float(err.max()))

    _verify(L, dtype, run, (B, Cc // 16, H, W, 16), Cc, ref, B, dev, st, accept)


@gpu
@pytest.mark.parametrize("size", [(8, 64), (16, 66)], ids=["pipelined-8x64", "serial-16x66"])
def test_stem_fused_across_items(dev, size):
    """ay_stem_s2_fused_fwd, static dealing, image tiles fetched two items ahead: 8x64 images are one 4x32 item each of the
    pipelined kernel; 16x66 (a width that is no multiple of 4) takes the serial-phase kernel, two 8x32 items per image, the
    second one column wide.  Reference and bound of test_stem_fused_kernel."""
    H, W = size
    L = _lib.lib()
    st = _lib.stream_ptr()
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    Ho, Wo = H // 2, W // 2
    th = 4 if W % 4 == 0 else 8
    B, n_items, wgs = _batch_for(-(-Ho // th) * -(-Wo // 32))
    g = torch.Generator().manual_seed(11 + H + W)
    x = torch.rand(U, 3, H, W, generator=g)
    w0 = torch.randn(32, 3, 3, 3, generator=g) * 0.3
    s0, t0 = torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.2
    w1 = torch.randn(64, 32, 3, 3, generator=g) * (1.0 / np.sqrt(288))
    s1, t1 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.1
    mid = bf(F.leaky_relu(F.conv2d(bf(x), bf(w0), None, 1, 1) * s0.view(1, -1, 1, 1) + t0.view(1, -1, 1, 1), 0.1))
    ref = F.leaky_relu(F.conv2d(mid, bf(w1), None, 2, 1) * s1.view(1, -1, 1, 1) + t1.view(1, -1, 1, 1), 0.1)
    w0p = torch.zeros(32, 32)
    w0p[:, :27] = w0.reshape(32, 27)
    xbuf, xd = _guarded_f32(x, B, dev)
    w0d, w1d = w0p.to(torch.bfloat16).to(dev), w1.to(dev)
    s0d, t0d, s1d, t1d = s0.to(dev), t0.to(dev), s1.to(dev), t1.to(dev)
    packed = torch.empty(L.ay_packed_weight_bytes(64, 32, 3), device=dev, dtype=torch.uint8)
    check(L.ay_pack_conv_weights_bf16(ptr(w1d), ptr(packed), 64, 64, 32, 3, st))

    def run(out, b0, nb):
        check(L.ay_stem_s2_fused_fwd(ptr(xd[b0:b0 + nb]), ptr(w0d), ptr(s0d), ptr(t0d), 1, ptr(packed), ptr(s1d), ptr(t1d), 1, ptr(out),
                                     nb, H, W, st), "fused stem")

    def accept(got, ref):
        err = (got - ref).abs()
        bound = ref.abs() * 2.0 ** -7 + 4e-3   # an intermediate that rounds the other way moves the sum by ~1e-3
        share = float((err > bound).float().mean())
        print("fused stem share above the bound", share, "max error", float(err.max()))
        assert share <= 1e-3 and float(err.max()) <= 0.05, (share, float(err.max()))

    _verify(L, "bf16", run, (B, 4, Ho, Wo, 16), 64, ref, B, dev, st, accept)


def _stem_train_operands(dev, B, H, W):
    """image, filters (both roundings of test_stem_train_kernels), incoming gradient; forward reference and the filter gradient
    of every distinct image"""
    bf = lambda t: t.to(torch.bfloat16).to(torch.float32)
    g = torch.Generator().manual_seed(H * 7 + W)
    x = torch.rand(U, 3, H, W, generator=g)
    w = torch.randn(32, 3, 3, 3, generator=g) * 0.3
    dz = bf(torch.randn(U, 32, H, W, generator=g))
    ref_z, ref_dw = None, []
    for u in range(U):
        wb = bf(w).requires_grad_(True)
        y = F.conv2d(bf(x[u:u + 1]), wb, None, 1, 1)
        y.backward(dz[u:u + 1])
        ref_z = y.detach() if ref_z is None else torch.cat([ref_z, y.detach()])
        ref_dw.append(wb.grad.double())
    w0 = torch.zeros(32, 32)
    w0[:, :27] = w.reshape(32, 27)
    xbuf, xd = _guarded_f32(x, B, dev)
    return x, xbuf, xd, w0.to(torch.bfloat16).to(dev), dz, ref_z, ref_dw


@gpu
@pytest.mark.parametrize("stats", [False, True], ids=["fwd", "fwd_stats"])
def test_stem_train_fwd_across_items(dev, stats):
    """ay_stem_train_fwd_bf16 / ay_stem_train_fwd_stats_bf16 on 8x64 images, one item each, two workgroups per CU (so 16 items per
    CU), static dealing with the image tile fetched ahead.  Reference and bound of test_stem_train_kernels: F.conv2d on the
    rounded image and filters; every error within |ref| 2^-7 + 1e-6 and fewer than 0.02 of the elements with any error; the
    statistics are the sums of the rounded outputs to 1e-5.
    The cap against this seed, checked on the CPU: the float64 convolution of the same rounded operands, rounded to bf16, differs
    from the rounded fp32 reference in 0 of 65 536 elements, so the cap of 0.02 is all the kernel's own summation order."""
    H, W = 8, 64
    L = _lib.lib()
    st = _lib.stream_ptr()
    B, n_items, wgs = _batch_for(1, wgs_per_cu=2)
    x, xbuf, xd, w0d, dz, ref_z, ref_dw = _stem_train_operands(dev, B, H, W)
    sums = torch.full((64,), float("nan"), device=dev, dtype=torch.float64)
    sws = torch.empty(L.ay_stem_train_stats_workspace_bytes(), device=dev, dtype=torch.uint8)

    def run(out, b0, nb):
        if stats:
            check(L.ay_stem_train_fwd_stats_bf16(ptr(xd[b0:b0 + nb]), ptr(w0d), ptr(out), ptr(sums), ptr(sws), sws.numel(), nb, H, W, st),
                  "stem fwd + stats")
        else:
            check(L.ay_stem_train_fwd_bf16(ptr(xd[b0:b0 + nb]), ptr(w0d), ptr(out), nb, H, W, st), "stem fwd")

    seen = {}

    def accept(got, ref):
        seen["z"] = got
        err = (got - ref).abs()
        share = float((err > 0).float().mean())
        print("stem train share of elements with an error", share, "max error", float(err.max()))
        assert bool((err <= ref.abs() * 2.0 ** -7 + 1e-6).all()) and share < 0.02, (float(err.max()), share)

    _verify(L, "bf16", run, (B, 2, H, W, 16), 32, ref_z, B, dev, st, accept)
    if stats:
        # the whole batch once more (the harness ended on a single image); every image has the bits of its first copy (asserted
        # above), so the sums of the rounded outputs are B / U times those of the distinct images -- exact in float64
        zb = torch.empty(B, 2, H, W, 16, device=dev, dtype=torch.bfloat16)
        run(zb, 0, B)
        g64 = seen["z"].double()
        ref_sums = torch.cat([g64.sum((0, 2, 3)), (g64 * g64).sum((0, 2, 3))]) * (B // U)
        assert float((sums.cpu() - ref_sums).abs().max()) <= 1e-5 * float(ref_sums.abs().max()), (sums.cpu(), ref_sums)


@gpu
def test_stem_train_wgrad_across_items(dev):
    """ay_stem_train_wgrad_bf16 on 8x64 images, one item each, static dealing over two stage buffers; every wave sums over all items
    of its workgroup.  The result is one filter gradient for the batch, so the harness applies in the form a sum allows: NaN guard
    bands around image and dz, a sentinel band around dw, two calls with the same bits, the last image run alone against its own
    reference.  Reference and bound of test_stem_train_kernels: autograd of F.conv2d on the rounded operands,
    2e-5 max|ref| sqrt(B H W / 1000) + 1e-4, accumulation onto an existing dw within 1e-5 max|ref| more."""
    H, W = 8, 64
    L = _lib.lib()
    st = _lib.stream_ptr()
    B, n_items, wgs = _batch_for(1)
    x, xbuf, xd, w0d, dz, ref_z, ref_dw = _stem_train_operands(dev, B, H, W)
    zbuf, zb = _blocked_in(L, "bf16", dz, B, dev, st)
    ws = torch.empty(L.ay_stem_train_wgrad_workspace_bytes(), device=dev, dtype=torch.uint8)

    def run(b0, nb, accumulate=0, init=None):
        buf, dw = _guarded((32, 3, 3, 3), torch.float32, dev, SENTINEL)
        if init is not None:
            dw.fill_(init)
        check(L.ay_stem_train_wgrad_bf16(ptr(xd[b0:b0 + nb]), ptr(zb[b0:b0 + nb]), ptr(dw), accumulate, ptr(ws), ws.numel(), nb, H, W, st),
              "stem wgrad")
        torch.cuda.synchronize()
        raw = buf.view(torch.int32)   # 864 floats between two bands of GUARD floats
        assert bool((raw[:GUARD] == SENTINEL * 0x10001).all()) and bool((raw[GUARD + 864:] == SENTINEL * 0x10001).all()), "output guard band overwritten"
        return dw.cpu()

    def within(got, ref, nb, extra=0.0):
        tol = 2e-5 * float(ref.abs().max()) * np.sqrt(nb * H * W / 1000.0) + 1e-4 + extra * float(ref.abs().max())
        err = float((got.double() - ref).abs().max())
        print("stem wgrad error", err, "tolerance", tol)
        assert np.isfinite(err) and err <= tol, (err, tol)

    ref = sum(ref_dw) * (B // U)
    d1, d2 = run(0, B), run(0, B)
    assert torch.equal(d1, d2), "the filter gradient must not depend on the run"
    within(d1, ref, B)
    within(run(0, B, accumulate=1, init=1.0) - 1.0, ref, B, extra=1e-5)
    within(run(B - 1, 1), ref_dw[(B - 1) % U], 1)


def test_conv_rejects_inputs_beyond_the_descriptor_range():
    """The ring kernels read one image's input through a buffer descriptor (32-bit lane offsets, 0x80000000 = "nothing to fetch"):
    an image whose INPUT exceeds 2 GiB -- while its output stays below -- is refused with the argument error before anything is
    launched.  Host-side check, no GPU."""
    L = _lib.lib()
    dummy = C.c_void_p(0x1000)
    d = ConvDesc(1, 64, 32, 8192, 8192, 4096, 4096, 3, 2, 1, 0, 32)          # in 8 GiB, out 1 GiB
    assert L.ay_conv_fwd_bf16(C.byref(d), dummy, dummy, dummy, dummy, None, dummy, None) == -1
    assert b"input" in L.ay_last_error() and b"2 GiB" in L.ay_last_error()
    assert L.ay_conv_fwd_f16(C.byref(d), dummy, dummy, dummy, dummy, None, dummy, None) == -1
    d = ConvDesc(1, 512, 128, 2048, 2048, 2048, 2048, 3, 1, 1, 0, 128)       # in 4 GiB, out 1 GiB
    assert L.ay_conv3x3_m16_fwd_bf16(C.byref(d), dummy, dummy, dummy, dummy, None, dummy, None) == -1
    assert b"input" in L.ay_last_error() and b"2 GiB" in L.ay_last_error()
    d = ConvDesc(1, 512, 128, 2048, 2048, 2048, 2048, 1, 1, 1, 0, 128)
    assert L.ay_conv1x1_cat_fwd_bf16(C.byref(d), dummy, 256, dummy, dummy, dummy, dummy, dummy, None) == -1
    assert b"2 GiB" in L.ay_last_error()
