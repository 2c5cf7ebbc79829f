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
  * image independence: image b of the batch has the bits of the same image run alone -- and of every other copy of it."""
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


def _verify(L, dtype, run, out_shape, cout, ref_unique, B, dev, st):
    """run(out, b0, nb): the call under test on images b0 .. b0 + nb - 1 into `out` ([nb] + out_shape[1:])"""
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
