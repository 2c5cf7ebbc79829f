"""GPU (-m gpu): the convolution kernels against the EXACT reference of tests/conv_exact_reference.py -- integer operands, so every
comparison is equality with the bits a float64 convolution and the documented fp32 epilogue give (no tolerance, no share of
elements left out).  tests/test_conv_exact_cpu.py holds the conditions this rests on, asserted on the reference alone.

What each group pins beyond today's tolerance tests:
  * round-to-nearest-even of the one rounding per stored activation (every case has >= 100 exact ties), the order affine ->
    LeakyReLU -> residual -> rounding, exact zeros in padded channels, every pixel of every tile (a missing border term changes an
    integer sum by at least one grid unit);
  * the 16-bit intermediate of the fused stem and the fused residual block (its rounding changes 2-19 % of the bfloat16 values);
  * rectangular images (hin != win) through every entry point that takes them: the `rect` tests; outputs lie inside guard bands.

Kernel instantiations reached: profiles/conv_exact_kernels.txt holds the kernel names of a traced run of this module (square and
rectangular cases as two runs).  It shows the 16x16x32 kernel with and without residual, both fused residual blocks and both
fused-stem kernels in both types, the stem and training-stem kernels, the five fp32 MFMA forms, every register-staged
conv_bf16_kernel that conv_fwd_16 can select, the 256-wide 1x1 ring kernel with and without canvas, the route-folding 1x1
(launch_ring1x1<128, ..., true>), all seven weight-gradient instantiations, and launch_dgrad_s2 for cin_pad 128 and 64 with and
without a gradient in dx and for cin_pad 32 in its 16-row and 8-row forms, each with and without one.

A residual on a 1x1 layer: no layer of the network adds a shortcut there in the FORWARD pass, but every bf16 training step does in
the BACKWARD pass.  train_backward_bf16 computes a stride-1 data gradient as ay_conv_fwd_bf16 on re-packed filters with
residual == out == the gradient already in dx, and in a residual block [1x1 C -> C/2, 3x3 C/2 -> C + shortcut] the shortcut has put
dy there before the 1x1 layer's data gradient arrives.  So the 1x1 forward kernels run with a residual, in place, once per residual
block and step (profiles/train_step_kernels.txt: a traced training step, with the module that compares each kernel exactly):
  * C = 128 ... 1024: conv_bf16_ring_kernel<1, 1, 128, 2, 4, 8, 32, 4, 3, true, false, CANVAS> with and without canvas (a residual
    keeps cout_pad % 256 == 0 away from the 256-wide tile);
  * C = 64 (32 input channels, no multiple of 64): the register-staged conv_bf16_kernel<1, 1, 32, 1, 4, 8, 32, 1, false, true>.
DGRAD_S1_ACC_1X1_CASES pins them: six shapes (both kernels; the ring kernel on a canvas and image by image, at 128, 256 and 512
channels), dz in [-64, 64] so that the sums meet bfloat16's rounding, each run in place and with the residual in a buffer of its own
(which comes back unchanged), both equal to the reference and to each other bit for bit.  SQUARE_CONV_CASES adds the plain BN=128 1x1
ring kernel tiled image by image, which appeared only in its route-folding form before.
Of the ring kernels (nine tile shapes x residual x canvas x type) the trace still lacks these, which nothing selects:
  * a residual on a stride-2 layer (BN 128 / 64), and on a 1x1 layer in the forms the data gradient does not take (BN 64 / 32 ring
    tiles, the half type): no layer of the network adds a shortcut there in either pass and no case does; these forms remain unused
    and untested, and are not first run here.
The slab reduction of ay_conv_wgrad_bf16_ws takes one lane group per slab, at most 16 / 8 / 4 by the filter count (below 256 K /
below 1 M / from 1 M weights), and the slab count is at most a 24th of the K steps (B * hout * ceil(wout / 32) / segments per step).
The trace shows wgrad_reduce_kernel<1>, <2> (2 and 3 slabs) and <16> (the 128 x 96 case: 384 K steps, 16 slabs).  <8> and <4> need
192 and 96 K steps at 256 K and 1 M weights and more -- images of 100 x 64 at 128 -> 256 channels, whose float64 reference takes longer
than a test here may; test_gpu_train_bf16_paths.py runs the slab path with 8 and more slabs against its tolerance."""
import ctypes as C

import pytest
import torch

import conv_exact_reference as R
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ConvDesc, check, ptr
from test_gpu_parity import CONV_CASES, F32_CASES
from test_gpu_train_bf16 import WGRAD_CASES

pytestmark = pytest.mark.gpu
GUARD = 8192          # 16-bit elements on either side of an output
SENTINEL = 0x5A5A
ids = lambda c: "x".join(str(int(v)) for v in c)
DTYPES = ["bf16", "f16"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def _tdt(dtype):
    return {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[dtype]


def _ceil(v, m):
    return (v + m - 1) // m * m


def blocked(dtype, t, dev, cpad=None):
    """NCHW float32 (CPU) -> blocked 16-bit device tensor [B][cpad/16][H][W][16]; channels beyond C are zero"""
    L = _lib.lib()
    B, Cc, H, W = t.shape
    cpad = _ceil(Cc, 16) if cpad is None else cpad
    if cpad != Cc:
        t = torch.cat([t, torch.zeros(B, cpad - Cc, H, W)], 1)
    td = t.contiguous().to(dev)
    out = torch.empty(B, cpad // 16, H, W, 16, device=dev, dtype=_tdt(dtype))
    check(getattr(L, f"ay_nchw_f32_to_blocked_{dtype}")(ptr(td), ptr(out), B, cpad, H, W, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return out


class Guarded:
    """an output tensor pre-filled with NaN in the middle of a buffer of sentinels: a store outside the tensor shows"""

    def __init__(self, shape, dtype, dev):
        n16 = int(torch.Size(shape).numel()) * (2 if dtype == "f32" else 1)
        self.buf = torch.full((n16 + 2 * GUARD,), SENTINEL, device=dev, dtype=torch.int16)
        self.n16 = n16
        self.t = self.buf[GUARD:GUARD + n16].view(_tdt(dtype)).view(shape)
        self.t.fill_(float("nan"))

    def intact(self):
        return bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n16:] == SENTINEL).all())


def unblocked(dtype, ob, channels):
    """blocked device tensor (16-bit, or float32 for dtype "f32") -> NCHW float32 on the CPU, exactly"""
    L = _lib.lib()
    B, _, H, W, _ = ob.shape
    out = torch.empty(B, channels, H, W, device=ob.device)
    fn = L.ay_blocked_f32_to_nchw_f32 if dtype == "f32" else getattr(L, f"ay_blocked_{dtype}_to_nchw_f32")
    check(fn(ptr(ob), ptr(out), B, channels, H, W, _lib.stream_ptr()))
    return out.cpu()


def packed_filters(dtype, w, cpad, dev):
    L = _lib.lib()
    cout, cin, k, _ = w.shape
    wd = w.contiguous().to(dev)
    packed = torch.empty(L.ay_packed_weight_bytes(cpad, cin, k), device=dev, dtype=torch.uint8)
    check(getattr(L, f"ay_pack_conv_weights_{dtype}")(ptr(wd), ptr(packed), cout, cpad, cin, k, _lib.stream_ptr()))
    torch.cuda.synchronize()
    return packed


def padded_vec(v, cpad, dev):
    out = torch.zeros(cpad, device=dev)
    out[:v.numel()] = v.to(dev)
    return out


def with_zero_channels(want, cpad):
    B, Cc, H, W = want.shape
    return want if cpad == Cc else torch.cat([want, torch.zeros(B, cpad - Cc, H, W)], 1)


# ------------------------------------------------------------------------------------------- 1. ay_conv_fwd_{bf16,f16}
def run_conv(dev, case, dtype, entry="ay_conv_fwd", cpad_mult=32):
    cin, cout, k, stride, H, W, leaky, has_res, out_f32, B = case
    L = _lib.lib()
    st = _lib.stream_ptr()
    r = R.conv_reference(case, dtype)
    Ho, Wo = r["out"].shape[2:]
    cpad = _ceil(cout, cpad_mult)
    xb = blocked(dtype, r["x"], dev)
    packed = packed_filters(dtype, r["w"], cpad, dev)
    sc, sh = padded_vec(r["scale"], cpad, dev), padded_vec(r["shift"], cpad, dev)
    rb = blocked(dtype, r["res"], dev, cpad) if has_res else None
    odt = "f32" if out_f32 else dtype
    out = Guarded((B, cpad // 16, Ho, Wo, 16), odt, dev)
    d = ConvDesc(B, cin, cout, H, W, Ho, Wo, k, stride, int(leaky), int(out_f32), cpad)
    check(getattr(L, f"{entry}_{dtype}")(C.byref(d), ptr(xb), ptr(packed), ptr(sc), ptr(sh), ptr(rb), ptr(out.t), st), entry)
    got = unblocked(odt, out.t, cpad)
    assert out.intact(), "stores outside the output tensor"
    R.assert_same_numbers(got, with_zero_channels(r["out"], cpad), f"{entry}_{dtype} {ids(case)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [R.conv_case(c) for c in CONV_CASES] + R.SQUARE_CONV_CASES, ids=ids)
def test_conv_fwd_exact(dev, case, dtype):
    """every branch of conv_fwd_16 (CONV_CASES of test_gpu_parity, SQUARE_CONV_CASES): the reference's bits, padded channels exact zeros"""
    run_conv(dev, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.RECT_CONV_CASES, ids=ids)
def test_conv_fwd_exact_rect(dev, case, dtype):
    """hin != win through every branch: wide, tall, stride 2 with odd and even sides mixed, canvases of cells that are not square"""
    run_conv(dev, case, dtype)


# ------------------------------------------------------------------------------------------- 2. direct entry points
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.M16_CASES, ids=ids)
def test_conv3x3_m16_exact(dev, case, dtype):
    run_conv(dev, case, dtype, entry="ay_conv3x3_m16_fwd", cpad_mult=128)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", R.M16_RECT_CASES, ids=ids)
def test_conv3x3_m16_exact_rect(dev, case, dtype):
    run_conv(dev, case, dtype, entry="ay_conv3x3_m16_fwd", cpad_mult=128)


def run_cat(dev, case, dtype):
    c1, c2, cout, H, W = case
    L = _lib.lib()
    r = R.cat_reference(case, dtype)
    ab, bb = blocked(dtype, r["a"], dev), blocked(dtype, r["b"], dev)
    packed = packed_filters(dtype, r["w"], cout, dev)
    sc, sh = r["scale"].to(dev), r["shift"].to(dev)
    out = Guarded((2, cout // 16, H, W, 16), dtype, dev)
    d = ConvDesc(2, c1 + c2, cout, H, W, H, W, 1, 1, 1, 0, cout)
    check(getattr(L, f"ay_conv1x1_cat_fwd_{dtype}")(C.byref(d), ptr(ab), c1, ptr(bb), ptr(packed), ptr(sc), ptr(sh), ptr(out.t), _lib.stream_ptr()))
    got = unblocked(dtype, out.t, cout)
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"conv1x1_cat {dtype} {ids(case)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.CAT_CASES if c[3] == c[4]], ids=ids)
def test_conv1x1_cat_exact(dev, case, dtype):
    run_cat(dev, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.CAT_CASES if c[3] != c[4]], ids=ids)
def test_conv1x1_cat_exact_rect(dev, case, dtype):
    run_cat(dev, case, dtype)


def run_resblock(dev, case, dtype):
    Cc, H, W, B, leaky1, leaky2 = case
    L = _lib.lib()
    r = R.resblock_reference(case, dtype)
    xb = blocked(dtype, r["x"], dev)
    p1, p2 = packed_filters(dtype, r["w1"], Cc // 2, dev), packed_filters(dtype, r["w2"], Cc, dev)
    s1, t1, s2, t2 = (r[k].to(dev) for k in ("scale1", "shift1", "scale2", "shift2"))
    out = Guarded((B, Cc // 16, H, W, 16), dtype, dev)
    check(getattr(L, f"ay_resblock_fwd_{dtype}")(ptr(xb), ptr(p1), ptr(s1), ptr(t1), int(leaky1), ptr(p2), ptr(s2), ptr(t2), int(leaky2), ptr(out.t),
                                                 B, Cc, H, W, _lib.stream_ptr()), "resblock")
    got = unblocked(dtype, out.t, Cc)
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"resblock {dtype} {ids(case)}")
    # the two ay_conv_fwd calls it replaces reach the same bits: the intermediate's rounding is the stored one
    mid = Guarded((B, Cc // 32, H, W, 16), dtype, dev)
    d1 = ConvDesc(B, Cc, Cc // 2, H, W, H, W, 1, 1, int(leaky1), 0, Cc // 2)
    check(getattr(L, f"ay_conv_fwd_{dtype}")(C.byref(d1), ptr(xb), ptr(p1), ptr(s1), ptr(t1), None, ptr(mid.t), _lib.stream_ptr()), "conv1")
    R.assert_same_numbers(unblocked(dtype, mid.t, Cc // 2), r["mid"], f"resblock intermediate {dtype} {ids(case)}")
    out2 = Guarded((B, Cc // 16, H, W, 16), dtype, dev)
    d2 = ConvDesc(B, Cc // 2, Cc, H, W, H, W, 3, 1, int(leaky2), 0, Cc)
    check(getattr(L, f"ay_conv_fwd_{dtype}")(C.byref(d2), ptr(mid.t), ptr(p2), ptr(s2), ptr(t2), ptr(xb), ptr(out2.t), _lib.stream_ptr()), "conv2")
    R.assert_same_numbers(unblocked(dtype, out2.t, Cc), r["out"], f"two-call block {dtype} {ids(case)}")
    assert mid.intact() and out2.intact()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.RESBLOCK_CASES if c[1] == c[2]], ids=ids)
def test_resblock_exact(dev, case, dtype):
    """C 64 and 128, each activation on and off: every output equals the reference, the 16-bit intermediate included (no share of
    elements left out, unlike test_resblock_fused_kernel)"""
    run_resblock(dev, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.RESBLOCK_CASES if c[1] != c[2]], ids=ids)
def test_resblock_exact_rect(dev, case, dtype):
    run_resblock(dev, case, dtype)


def run_stem_fused(dev, case, dtype):
    H, W, B = case
    L = _lib.lib()
    r = R.stem_fused_reference(case, dtype)
    w0p = torch.zeros(32, 32)
    w0p[:, :27] = r["w0"].reshape(32, 27)
    xd, w0d = r["x"].to(dev), w0p.to(_tdt(dtype)).to(dev)
    packed = packed_filters(dtype, r["w1"], 64, dev)
    s0, t0, s1, t1 = (r[k].to(dev) for k in ("scale1", "shift1", "scale2", "shift2"))
    out = Guarded((B, 4, H // 2, W // 2, 16), dtype, dev)
    fn = L.ay_stem_s2_fused_fwd if dtype == "bf16" else L.ay_stem_s2_fused_fwd_f16
    check(fn(ptr(xd), ptr(w0d), ptr(s0), ptr(t0), 1, ptr(packed), ptr(s1), ptr(t1), 1, ptr(out.t), B, H, W, _lib.stream_ptr()), "stem fused")
    got = unblocked(dtype, out.t, 64)
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"stem fused {dtype} {ids(case)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.STEM_FUSED_CASES if c[0] == c[1]], ids=ids)
def test_stem_fused_exact(dev, case, dtype):
    """W % 4 == 0 takes the pipelined kernel, any other width the 4-byte-DMA kernel: every output equals the reference"""
    run_stem_fused(dev, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.STEM_FUSED_CASES if c[0] != c[1]], ids=ids)
def test_stem_fused_exact_rect(dev, case, dtype):
    run_stem_fused(dev, case, dtype)


def run_stem_conv(dev, case, dtype):
    H, W, B = case
    L = _lib.lib()
    r = R.stem_conv_reference(case, dtype)
    xd, wd, sc, sh = (r[k].to(dev) for k in ("x", "w", "scale", "shift"))
    out = Guarded((B, 2, H, W, 16), dtype, dev)
    fn = L.ay_stem_conv_fwd if dtype == "bf16" else L.ay_stem_conv_fwd_f16
    check(fn(ptr(xd), ptr(wd), ptr(sc), ptr(sh), ptr(out.t), B, H, W, 1, _lib.stream_ptr()))
    got = unblocked(dtype, out.t, 32)
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"stem conv {dtype} {ids(case)}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.STEM_CONV_CASES if c[0] == c[1]], ids=ids)
def test_stem_conv_exact(dev, case, dtype):
    run_stem_conv(dev, case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [c for c in R.STEM_CONV_CASES if c[0] != c[1]], ids=ids)
def test_stem_conv_exact_rect(dev, case, dtype):
    run_stem_conv(dev, case, dtype)


# ------------------------------------------------------------------------------------------- 3. fp32 path
def run_f32(dev, case, entry):
    cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B = case
    L = _lib.lib()
    r = R.f32_reference(case)
    Ho, Wo = r["out"].shape[2:]
    d = ConvDesc(B, cin1 + cin2, cout, H, W, Ho, Wo, k, stride, int(leaky), 0, cout)
    x1d, wd, scd, shd = (r[k_].to(dev) for k_ in ("x1", "w", "scale", "shift"))
    x2d = None if r["x2"] is None else r["x2"].to(dev)
    rd = None if r["res"] is None else r["res"].to(dev)
    out = Guarded((B, cout, Ho, Wo), "f32", dev)
    check(getattr(L, entry)(C.byref(d), ptr(x1d), cin1, up1, ptr(x2d), ptr(wd), ptr(scd), ptr(shd), ptr(rd), ptr(out.t), _lib.stream_ptr()), entry)
    got = out.t.cpu()
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"{entry} {ids(case)}")


@pytest.mark.parametrize("entry", ["ay_conv_fwd_f32", "ay_conv_fwd_f32_valu"])
@pytest.mark.parametrize("case", [R.f32_case(c) for c in F32_CASES], ids=ids)
def test_conv_f32_exact(dev, case, entry):
    """exact-fp32 MFMA (32x32x2) and the VALU fmaf chain of the fp32 training engine: fp32 outputs, bit for bit"""
    run_f32(dev, case, entry)


@pytest.mark.parametrize("entry", ["ay_conv_fwd_f32", "ay_conv_fwd_f32_valu"])
@pytest.mark.parametrize("case", R.RECT_F32_CASES, ids=ids)
def test_conv_f32_exact_rect(dev, case, entry):
    run_f32(dev, case, entry)


@pytest.mark.parametrize("entry", ["ay_conv_fwd_f32", "ay_conv_fwd_f32_valu"])
def test_conv_f32_refuses_odd_upsampled_side(dev, entry):
    """up1 = 1 reads src1 at (y >> 1, x >> 1) of a plane of (hin >> 1) x (win >> 1): an odd side would address a row or column
    past it.  Refused on the host: AY_ERR_ARG, a message, the output untouched"""
    L = _lib.lib()
    t = torch.zeros(1 << 12, device=dev)
    for hin, win in ((13, 12), (12, 13)):
        d = ConvDesc(1, 8, 8, hin, win, hin, win, 1, 1, 1, 0, 8)
        out = Guarded((1, 8, hin, win), "f32", dev)
        rc = getattr(L, entry)(C.byref(d), ptr(t), 8, 1, None, ptr(t), ptr(t), ptr(t), None, ptr(out.t), _lib.stream_ptr())
        torch.cuda.synchronize()
        assert rc == -1                      # AY_ERR_ARG
        assert len(L.ay_last_error()) > 0 and b"up1" in L.ay_last_error()
        assert bool(torch.isnan(out.t).all()) and out.intact()


@pytest.mark.parametrize("entry", ["ay_conv_fwd_f32", "ay_conv_fwd_f32_valu"])
def test_conv_f32_refuses_zero_stride(dev, entry):
    """the shared output-size check divides by the stride: stride 0 is refused on the host before it, the output untouched"""
    L = _lib.lib()
    t = torch.zeros(1 << 12, device=dev)
    d = ConvDesc(1, 8, 8, 12, 12, 12, 12, 1, 0, 1, 0, 8)
    out = Guarded((1, 8, 12, 12), "f32", dev)
    rc = getattr(L, entry)(C.byref(d), ptr(t), 8, 0, None, ptr(t), ptr(t), ptr(t), None, ptr(out.t), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1                      # AY_ERR_ARG
    assert b"output size" in L.ay_last_error()
    assert bool(torch.isnan(out.t).all()) and out.intact()


def run_f32_grads(dev, case):
    cin, cout, k, s, H, W, B = case
    L = _lib.lib()
    st = _lib.stream_ptr()
    r = R.grad_reference(case)
    Ho, Wo = r["dz"].shape[2:]
    d = ConvDesc(B, cin, cout, H, W, Ho, Wo, k, s, 0, 0, cout)
    xd, wd, dzd = r["x"].to(dev), r["w"].to(dev), r["dz"].to(dev)
    dx = Guarded((B, cin, H, W), "f32", dev)
    check(L.ay_conv_dgrad_f32(C.byref(d), ptr(dzd), ptr(wd), ptr(dx.t), 0, st))
    R.assert_same_numbers(dx.t.cpu(), r["dx"], f"dgrad_f32 {ids(case)}")
    prev = R.residuals(R.gen(cin, cout, H, W, 43), r["dx"].shape)
    dx.t.copy_(prev.to(dev))
    check(L.ay_conv_dgrad_f32(C.byref(d), ptr(dzd), ptr(wd), ptr(dx.t), 1, st))      # accumulate onto integer contents
    R.assert_same_numbers(dx.t.cpu(), prev + r["dx"], f"dgrad_f32 accumulate {ids(case)}")
    dw = Guarded((cout, cin, k, k), "f32", dev)
    check(L.ay_conv_wgrad_f32(C.byref(d), ptr(xd), ptr(dzd), ptr(dw.t), st))
    R.assert_same_numbers(dw.t.cpu(), r["dw"], f"wgrad_f32 {ids(case)}")
    assert dx.intact() and dw.intact()


@pytest.mark.parametrize("case", [c for c in R.F32_GRAD_CASES if c[4] == c[5]], ids=ids)
def test_f32_gradients_exact(dev, case):
    run_f32_grads(dev, case)


@pytest.mark.parametrize("case", [c for c in R.F32_GRAD_CASES if c[4] != c[5]], ids=ids)
def test_f32_gradients_exact_rect(dev, case):
    run_f32_grads(dev, case)


# ------------------------------------------------------------------------------------------- 4. bf16 training kernels
def run_wgrad(dev, case):
    cin, cout, k, s, H, W, B = case
    L = _lib.lib()
    st = _lib.stream_ptr()
    r = R.grad_reference(case)
    Ho, Wo = r["dz"].shape[2:]
    cpad = _ceil(cout, 32)
    xb, dzb = blocked("bf16", r["x"], dev), blocked("bf16", r["dz"], dev, cpad)
    d = ConvDesc(B, cin, cout, H, W, Ho, Wo, k, s, 0, 0, cpad)
    shape = (cout, cin, k, k)
    prev = R.residuals(R.gen(cin, cout, k, 47), shape)
    forms = {}
    dw = Guarded(shape, "f32", dev)
    check(L.ay_conv_wgrad_bf16(C.byref(d), ptr(xb), ptr(dzb), ptr(dw.t), st), "wgrad")
    forms["atomics"] = dw.t.cpu()
    dwa = Guarded(shape, "f32", dev)
    dwa.t.copy_(prev.to(dev))
    check(L.ay_conv_wgrad_bf16_acc(C.byref(d), ptr(xb), ptr(dzb), ptr(dwa.t), 1, st), "wgrad_acc")
    forms["atomics onto contents"] = dwa.t.cpu() - prev      # integers: the subtraction is exact
    ws = torch.empty(max(L.ay_conv_wgrad_workspace_bytes(C.byref(d)), 16), device=dev, dtype=torch.uint8)
    dws = Guarded(shape, "f32", dev)
    check(L.ay_conv_wgrad_bf16_ws(C.byref(d), ptr(xb), ptr(dzb), ptr(dws.t), 0, ptr(ws), ws.numel(), st), "wgrad_ws")
    forms["slabs"] = dws.t.cpu()
    dws.t.copy_(prev.to(dev))
    check(L.ay_conv_wgrad_bf16_ws(C.byref(d), ptr(xb), ptr(dzb), ptr(dws.t), 1, ptr(ws), ws.numel(), st), "wgrad_ws acc")
    forms["slabs onto contents"] = dws.t.cpu() - prev
    assert dw.intact() and dwa.intact() and dws.intact()
    for name, got in forms.items():      # exact sums: atomics and slabs cannot differ, from each other or from the reference
        R.assert_same_numbers(got, r["dw"], f"wgrad {name} {ids(case)}")


@pytest.mark.parametrize("case", [R.wgrad_case(c) for c in WGRAD_CASES], ids=ids)
def test_wgrad_bf16_exact(dev, case):
    """the seven instantiations (narrow / plain 3x3 s1, 3x3 s2 and 1x1, the wide 1x1), three forms each: fp32 integers, bit for bit"""
    run_wgrad(dev, case)


@pytest.mark.parametrize("case", R.RECT_WGRAD_CASES, ids=ids)
def test_wgrad_bf16_exact_rect(dev, case):
    run_wgrad(dev, case)


def run_dgrad_s2(dev, case):
    cin, cout, H, W, has_prev = case
    L = _lib.lib()
    st = _lib.stream_ptr()
    r = R.dgrad_reference(case, 2)
    B = 2
    cpad, cin_pad = _ceil(cout, 32), _ceil(cin, 32)
    dzb = blocked("bf16", r["dz"], dev, cpad)
    wd = r["w"].to(dev)
    packed = torch.empty(L.ay_packed_dgrad_s2_weight_bytes(cpad, cin_pad), device=dev, dtype=torch.uint8)
    check(L.ay_pack_dgrad_s2_weights_bf16(ptr(wd), ptr(packed), cout, cpad, cin, cin_pad, st))
    ones, zeros = torch.ones(cin_pad, device=dev), torch.zeros(cin_pad, device=dev)
    dx = Guarded((B, cin_pad // 16, H, W, 16), "bf16", dev)
    if has_prev:
        dx.t.copy_(blocked("bf16", r["prev"], dev, cin_pad))
    d = ConvDesc(B, cin, cout, H, W, H // 2, W // 2, 3, 2, 0, 0, cpad)
    check(L.ay_conv_dgrad_s2_bf16(C.byref(d), ptr(dzb), ptr(packed), ptr(ones), ptr(zeros), ptr(dx.t) if has_prev else None, ptr(dx.t), cin_pad, st), "dgrad s2")
    got = unblocked("bf16", dx.t, cin_pad)
    assert dx.intact()
    R.assert_same_numbers(got, with_zero_channels(r["out"], cin_pad), f"dgrad_s2 {ids(case)}")


@pytest.mark.parametrize("case", [c for c in R.DGRAD_S2_CASES if c[2] == c[3]], ids=ids)
def test_dgrad_s2_exact(dev, case):
    """cin_pad 32 / 64 / 128, with and without a gradient already in dx (added before the one rounding)"""
    run_dgrad_s2(dev, case)


@pytest.mark.parametrize("case", [c for c in R.DGRAD_S2_CASES if c[2] != c[3]], ids=ids)
def test_dgrad_s2_exact_rect(dev, case):
    run_dgrad_s2(dev, case)


def run_dgrad_s1(dev, case):
    cin, cout, k, H, W, has_prev = case
    L = _lib.lib()
    st = _lib.stream_ptr()
    r = R.dgrad_reference(case, 1)
    B = 2
    cpad, cin_pad = _ceil(cout, 32), _ceil(cin, 32)
    dzb = blocked("bf16", r["dz"], dev, cpad)
    wd = r["w"].to(dev)
    packed = torch.empty(L.ay_packed_dgrad_weight_bytes(cpad, cin_pad, k), device=dev, dtype=torch.uint8)
    check(L.ay_pack_dgrad_weights_bf16(ptr(wd), ptr(packed), cout, cin, cin_pad, k, st))
    ones, zeros = torch.ones(cin_pad, device=dev), torch.zeros(cin_pad, device=dev)
    shape = (B, cin_pad // 16, H, W, 16)
    d = ConvDesc(B, cpad, cin, H, W, H, W, k, 1, 0, 0, cin_pad)
    want = with_zero_channels(r["out"], cin_pad)
    # in place, as train_backward_bf16 issues it: the gradient already in dx is the residual operand AND the output
    dx = Guarded(shape, "bf16", dev)
    if has_prev:
        dx.t.copy_(blocked("bf16", r["prev"], dev, cin_pad))
    check(L.ay_conv_fwd_bf16(C.byref(d), ptr(dzb), ptr(packed), ptr(ones), ptr(zeros), ptr(dx.t) if has_prev else None, ptr(dx.t), st), "dgrad")
    got = unblocked("bf16", dx.t, cin_pad)
    assert dx.intact()
    R.assert_same_numbers(got, want, f"dgrad_s1 {ids(case)}")
    if not has_prev:
        return
    # the same with the residual in a buffer of its own, which comes back unchanged: the in-place form read nothing stale
    prev = Guarded(shape, "bf16", dev)
    prev.t.copy_(blocked("bf16", r["prev"], dev, cin_pad))
    kept = prev.t.clone()
    dx2 = Guarded(shape, "bf16", dev)
    check(L.ay_conv_fwd_bf16(C.byref(d), ptr(dzb), ptr(packed), ptr(ones), ptr(zeros), ptr(prev.t), ptr(dx2.t), st), "dgrad, separate residual")
    got2 = unblocked("bf16", dx2.t, cin_pad)
    assert dx2.intact() and prev.intact()
    assert torch.equal(prev.t.view(torch.int16), kept.view(torch.int16)), "the residual operand changed"
    R.assert_same_numbers(got2, want, f"dgrad_s1, separate residual {ids(case)}")
    assert torch.equal(dx2.t.view(torch.int16), dx.t.view(torch.int16)), "in-place and separate-buffer forms differ in their bits"


@pytest.mark.parametrize("case", [c for c in R.DGRAD_S1_CASES if c[3] == c[4]], ids=ids)
def test_dgrad_s1_exact(dev, case):
    """the stride-1 data gradient: ay_pack_dgrad_weights_bf16 + ay_conv_fwd_bf16, accumulation through the residual operand -- in place
    (residual == out, the engine's form) and from a buffer of its own, bit-identical; the 1x1 cases are the accumulating data gradient
    of a residual block's first convolution"""
    run_dgrad_s1(dev, case)


@pytest.mark.parametrize("case", [c for c in R.DGRAD_S1_CASES if c[3] != c[4]], ids=ids)
def test_dgrad_s1_exact_rect(dev, case):
    run_dgrad_s1(dev, case)


def run_stem_train(dev, case):
    B, H, W = case
    L = _lib.lib()
    st = _lib.stream_ptr()
    r = R.stem_train_reference(case)
    w0 = torch.zeros(32, 32)
    w0[:, :27] = r["w"].reshape(32, 27)
    xd, w0d = r["x"].to(dev), w0.to(torch.bfloat16).to(dev)
    zb = Guarded((B, 2, H, W, 16), "bf16", dev)
    check(L.ay_stem_train_fwd_bf16(ptr(xd), ptr(w0d), ptr(zb.t), B, H, W, st), "stem fwd")
    R.assert_same_numbers(unblocked("bf16", zb.t, 32), r["z"], f"stem_train_fwd {ids(case)}")
    dzb = blocked("bf16", r["dz"], dev)
    ws = torch.empty(L.ay_stem_train_wgrad_workspace_bytes(), device=dev, dtype=torch.uint8)
    dw = Guarded((32, 3, 3, 3), "f32", dev)
    check(L.ay_stem_train_wgrad_bf16(ptr(xd), ptr(dzb), ptr(dw.t), 0, ptr(ws), ws.numel(), B, H, W, st), "stem wgrad")
    R.assert_same_numbers(dw.t.cpu(), r["dw"], f"stem_train_wgrad {ids(case)}")
    prev = R.residuals(R.gen(B, H, W, 53), (32, 3, 3, 3))
    dw.t.copy_(prev.to(dev))
    check(L.ay_stem_train_wgrad_bf16(ptr(xd), ptr(dzb), ptr(dw.t), 1, ptr(ws), ws.numel(), B, H, W, st), "stem wgrad acc")
    want = prev.double() + r["dw"].double()      # on the grid 1/64, far below 2^24 grid units: exact in fp32
    R.assert_same_numbers(dw.t.cpu(), R.to_f32_exact(want, "dW + contents"), f"stem_train_wgrad accumulate {ids(case)}")
    assert zb.intact() and dw.intact()


@pytest.mark.parametrize("case", [c for c in R.STEM_TRAIN_CASES if c[1] == c[2]], ids=ids)
def test_stem_train_exact(dev, case):
    run_stem_train(dev, case)


@pytest.mark.parametrize("case", [c for c in R.STEM_TRAIN_CASES if c[1] != c[2]], ids=ids)
def test_stem_train_exact_rect(dev, case):
    run_stem_train(dev, case)
