"""Exact references for the convolution kernels on SMALL-INTEGER operands (TEST INFRASTRUCTURE ONLY -- never imported by the
product), and the case lists the exact tests share (tests/test_conv_exact_cpu.py, tests/test_gpu_conv_exact.py).

The technique (the one rocBLAS uses for its GEMM tests): with integer activations in [-4, 4], filters in [-2, 2] and output
gradients in [-4, 4] ([-64, 64] for the accumulating 1x1 data gradients, see dgrad_reference) every product and every partial sum of a convolution is an integer far below 2^24, hence exactly
representable in fp32 -- ANY summation order (MFMA 32x32x16, 16x16x32, 32x32x2 f32, split-K slabs, fp32 atomics, an fmaf chain)
leaves the same fp32 accumulator, and a float64 convolution gives that accumulator exactly.  The epilogue the kernels promise
(csrc/ay_common.h, csrc/ay_conv_common.h: IEEE operations in a fixed order, ONE rounding per stored activation, to nearest even)
is then restated here in float32 torch operations, one per step:

    v = acc * scale + shift        exact by construction (scale[c] = 2^-e, shift[c] = k / 16; asserted against float64)
    l = max(v, float32(0.1) * v)   LeakyReLU, one fp32 rounding
    o = l + residual               one fp32 rounding
    out = round_to_nearest_even(o) to bfloat16 | half; nothing for fp32 outputs

so the kernel's output BITS are known and the comparison is equality (as numbers: -0 == +0; a NaN anywhere fails).

Two-layer kernels (fused stem, fused residual block): the first stage uses scale[c] = 10 * 2^-e and shift[c] = 10 * 2^-e * k.
Its pre-activations are multiples of 10 * 2^-e, for which float32(0.1) * v rounds to exactly v / 10 (asserted), so the 16-bit
intermediate stays on a power-of-two grid after the LeakyReLU as well and the second stage's sums are exact again -- while a
good share of the intermediates does change under its rounding (measured per case: `mid_inexact`).

Conditions on the REFERENCE (never on a kernel's result; tests/test_conv_exact_cpu.py asserts them for every case):
  * headroom: max over outputs of sum |a_i| |b_i| <= 2^20 * grid (grid = 1 for integer operands, the measured power-of-two
    grid of the operands otherwise): at least 4 spare bits below fp32's 24, a design margin for the unmeasured way a CDNA4 MFMA
    aligns its addends;
  * rounding exercised, 16-bit outputs: LeakyReLU cases have >= 25 % of the outputs not representable before the rounding, every
    case has >= 100 exact ties (the values where round-to-nearest-even differs from both truncation and round-half-up).  The
    exponent range of `scale` is widened per case, on the reference alone, until this holds (`final_affine`).
"""
import functools
import math

import torch
import torch.nn.functional as F

STORE = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
SIG_BITS = {"bf16": 8, "f16": 11}     # significand bits of the storage types (fp32: 24)
HEADROOM_BITS = 20                    # sums stay below 2^20 grid units: 4 spare bits
MIN_TIES = 100
MIN_INEXACT_LEAKY = 0.25
TENTH = torch.tensor(0.1, dtype=torch.float32)


# ------------------------------------------------------------------------------------------------ operand generators
def gen(*key):
    """a seeded generator; the key is the case itself, so a case has the same operands in every test"""
    seed = 0
    for v in key:
        seed = (seed * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def ints(g, shape, r):
    """integers in [-r, r] as float32 (exact in bfloat16 and half for r <= 256)"""
    return torch.randint(-r, r + 1, tuple(shape), generator=g).to(torch.float32)


def activations(g, shape):
    return ints(g, shape, 4)


def filters(g, shape):
    return ints(g, shape, 2)


def residuals(g, shape):
    return ints(g, shape, 8)


def stem_image(g, shape, denom=16):
    """multiples of 1/denom in [0, 1] (denom <= 128: a grid bfloat16 holds exactly)"""
    return torch.randint(0, denom + 1, tuple(shape), generator=g).to(torch.float32) / float(denom)


def final_affine(g, c, e_lo=3, e_hi=7):
    """scale[c] = 2^-e, e in e_lo..e_hi; shift[c] = k / 16, |k| <= 32"""
    e = torch.randint(e_lo, e_hi + 1, (c,), generator=g)
    k = torch.randint(-32, 33, (c,), generator=g)
    return torch.pow(2.0, -e.to(torch.float32)), k.to(torch.float32) / 16.0


def stage1_affine(g, c):
    """first stage of a two-layer kernel: scale[c] = 10 * 2^-e (e in 1..3), shift[c] = scale[c] * k, |k| <= 6"""
    e = torch.randint(1, 4, (c,), generator=g)
    k = torch.randint(-6, 7, (c,), generator=g)
    scale = 10.0 * torch.pow(2.0, -e.to(torch.float32))
    return scale, scale * k.to(torch.float32)


# ------------------------------------------------------------------------------------------------ the reference
def conv_acc(x, w, stride=1, pad=None):
    """the exact accumulator: F.conv2d in float64"""
    pad = (w.shape[-1] - 1) // 2 if pad is None else pad
    return F.conv2d(x.double(), w.double(), None, stride, pad)


def grid_of(*tensors):
    """largest power of two that divides every value of the tensors (1.0 for integers; values are dyadic rationals)"""
    g = 1.0
    for _ in range(40):
        if all(bool((t.double() / g == torch.round(t.double() / g)).all()) for t in tensors):
            return g
        g /= 2.0
    raise AssertionError("operands are not on a power-of-two grid")


def headroom_bits(x, w, stride=1, pad=None, grid=1.0):
    """log2 of (max over outputs of sum |a_i| |b_i|) / grid: the bits an exact accumulator needs"""
    pad = (w.shape[-1] - 1) // 2 if pad is None else pad
    m = float(F.conv2d(x.abs().double(), w.abs().double(), None, stride, pad).max())
    return math.log2(max(m / grid, 1.0))


def to_f32_exact(t64, what="accumulator"):
    t = t64.to(torch.float32)
    assert torch.equal(t.double(), t64), f"{what} is not exact in fp32"
    return t


def leaky_f32(v, leaky):
    return torch.maximum(v, v * TENTH) if leaky else v


def round_store(o, store):
    """the single rounding of a stored value (torch casts round to nearest even), back as float32"""
    if store == "f32":
        return o
    out = o.to(STORE[store]).to(torch.float32)
    assert bool(torch.isfinite(out).all()), "reference leaves the storage type's range"
    return out


def epilogue(acc64, scale, shift, leaky, res, store):
    """-> (o, out): the fp32 value before the rounding and the stored value, both float32, in the documented operation order"""
    acc = to_f32_exact(acc64)
    sc, sh = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    v = acc * sc + sh
    assert torch.equal(v.double(), acc64 * sc.double() + sh.double()), "acc * scale + shift is not exact in fp32"
    o = leaky_f32(v, leaky)
    if res is not None:
        o = o + res
    return o, round_store(o, store)


def first_stage(acc64, scale, shift, leaky, store):
    """intermediate of a two-layer kernel: -> (mid, share of the intermediates that changed under the rounding)"""
    acc = to_f32_exact(acc64)
    sc, sh = scale.view(1, -1, 1, 1), shift.view(1, -1, 1, 1)
    v = acc * sc + sh
    assert torch.equal(v.double(), acc64 * sc.double() + sh.double()), "first stage: acc * scale + shift is not exact in fp32"
    t = v * TENTH
    assert torch.equal(t.double() * 10.0, v.double()), "float32(0.1) * v is not exactly v / 10 on this grid"
    l = leaky_f32(v, leaky)
    mid = round_store(l, store)
    return mid, float((mid != l).float().mean())


def rounding_stats(o, store):
    """(share of values the storage type cannot hold, number of exact ties) of the fp32 values `o` before their rounding"""
    if store == "f32":
        return 0.0, 0
    drop = 24 - SIG_BITS[store]
    low = o.contiguous().view(torch.int32) & ((1 << drop) - 1)
    normal = o.abs() >= (2.0 ** -126 if store == "bf16" else 2.0 ** -14)   # a subnormal result has fewer bits: not counted
    inexact = (low != 0) & normal
    ties = (low == (1 << (drop - 1))) & normal
    return float(inexact.float().mean()), int(ties.sum())


def rounding_ok(o, store, leaky):
    inexact, ties = rounding_stats(o, store)
    return store == "f32" or (ties >= MIN_TIES and (not leaky or inexact >= MIN_INEXACT_LEAKY))


def assert_same_numbers(got, want, what=""):
    """equality as numbers (-0 == +0), no NaN anywhere"""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (what, tuple(got.shape), tuple(want.shape))
    assert not bool(torch.isnan(got).any()), (what, "NaN in the result", int(torch.isnan(got).sum()))
    bad = got != want
    if bool(bad.any()):
        idx = [int(v) for v in bad.nonzero()[0]]
        g_, w_ = got[tuple(idx)].item(), want[tuple(idx)].item()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} values differ; first at {idx}: got {g_!r}, want {w_!r}")


# ------------------------------------------------------------------------------------------------ single-layer cases
def conv_case(c):
    """CONV_CASES entry of test_gpu_parity (cin, cout, k, stride, H, leaky, residual, out_f32[, B]) -> the rectangular form
    (cin, cout, k, stride, H, W, leaky, residual, out_f32, B)"""
    cin, cout, k, stride, H, leaky, has_res, out_f32 = c[:8]
    return (cin, cout, k, stride, H, H, bool(leaky), bool(has_res), bool(out_f32), c[8] if len(c) > 8 else 2)


RECT_CONV_CASES = [
    # cin, cout, k, stride, H, W, leaky, residual, out_f32, B        one per branch of conv_fwd_16, hin != win
    (32, 64, 3, 1, 13, 40, True, True, False, 2),       # 8x32 tile, BN=64, wide
    (128, 256, 3, 1, 13, 40, True, True, False, 2),     # 8x32 tile, BN=128 (fewer than 16 rows), wide
    (64, 128, 3, 1, 40, 13, True, False, False, 2),     # 16x32 ring tile: two tall images side by side on the canvas
    (128, 256, 3, 1, 40, 13, True, True, False, 1),     # 16x16x32 kernel (one image: no canvas), tall, residual
    (128, 128, 3, 1, 20, 45, False, True, False, 1),    # 16x16x32 kernel, wide, linear: rows 16+4, columns 32+13
    (16, 32, 3, 1, 13, 40, True, False, False, 2),      # 32-channel tile
    (64, 32, 3, 1, 40, 13, False, True, False, 3),
    (128, 256, 3, 2, 26, 14, True, False, False, 2),    # stride 2, BN=128: 26x14 -> 13x7
    (32, 64, 3, 2, 14, 26, True, False, False, 3),      # stride 2, BN=64: 14x26 -> 7x13
    (64, 128, 3, 2, 13, 20, True, False, False, 2),     # stride 2, odd and even side mixed: 13x20 -> 7x10
    (16, 32, 3, 2, 26, 14, True, False, False, 2),      # stride 2, the register-staged 32-channel kernel
    (64, 32, 1, 1, 13, 40, True, False, False, 2),      # 1x1, NK=4, BN=32
    (256, 128, 1, 1, 40, 13, True, False, False, 2),    # 1x1, BN=128
    (512, 256, 1, 1, 13, 40, True, False, False, 2),    # 1x1, BN=256
    (48, 96, 1, 1, 40, 13, True, False, False, 2),      # 1x1, NK=1 (cin % 64 != 0)
    (256, 24, 1, 1, 13, 40, False, False, True, 2),     # fp32 head, cout 24 -> 32
    (128, 255, 1, 1, 20, 9, False, False, True, 2),     # fp32 head, 64-channel tile, 255 -> 256
    (128, 256, 3, 1, 13, 9, True, True, False, 7),      # canvas, cells 14 x 10, odd batch, residual
    (256, 128, 1, 1, 9, 13, True, False, False, 5),     # canvas 1x1, cells 10 x 14
    (128, 256, 3, 2, 26, 14, True, False, False, 5),    # canvas stride 2: input cells 28 x 16, output cells 14 x 8
    # the ring kernel's variants that the cases above leave out: tiled image by image (one image) and canvases without a residual
    (16, 128, 3, 1, 20, 45, True, False, False, 1),     # 16x32 ring tile (cin % 32 != 0: not the 16x16x32 kernel), one image
    (48, 128, 3, 1, 20, 45, True, True, False, 1),      # the same with a residual
    (64, 128, 3, 1, 13, 40, True, False, False, 1),     # 8x32 tile, BN=128, one image, no residual
    (32, 64, 3, 1, 13, 40, True, False, False, 1),      # BN=64, one image, no residual
    (32, 64, 3, 1, 13, 9, True, False, False, 5),       # BN=64, canvas, no residual
    (16, 32, 3, 1, 13, 40, True, False, False, 1),      # 32-channel tile, one image, no residual
]

# ay_conv3x3_m16_fwd_* called directly (its smallest shapes in test_gpu_parity, and one wide and one tall rectangle)
M16_CASES = [(32, 128, 3, 1, 33, 33, True, False, False, 2), (128, 256, 3, 1, 16, 16, True, True, False, 2)]
M16_RECT_CASES = [(64, 128, 3, 1, 18, 37, True, True, False, 2), (32, 128, 3, 1, 37, 18, False, False, False, 1)]

# square cases beyond CONV_CASES of test_gpu_parity (same form as RECT_CONV_CASES)
SQUARE_CONV_CASES = [
    (256, 128, 1, 1, 32, 32, True, False, False, 1),    # 1x1 ring kernel, BN=128, tiled image by image (one image), not route-folding
]


def _out_hw(k, stride, H, W):
    pad = (k - 1) // 2
    return (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1


@functools.lru_cache(maxsize=None)
def conv_operands(case):
    """integer operands of a single-layer case and the exact accumulator: shared by the storage types and the tests"""
    cin, cout, k, stride, H, W, leaky, has_res, out_f32, B = case
    g = gen(cin, cout, k, stride, H, W, B, has_res)
    x = activations(g, (B, cin, H, W))
    w = filters(g, (cout, cin, k, k))
    Ho, Wo = _out_hw(k, stride, H, W)
    res = residuals(g, (B, cout, Ho, Wo)) if has_res else None
    return x, w, res, conv_acc(x, w, stride), headroom_bits(x, w, stride)


@functools.lru_cache(maxsize=None)
def conv_reference(case, store):
    """-> dict(x, w, scale, shift, res, out, o, e_hi, bits, inexact, ties).  out_f32 cases store fp32 whatever `store` says (`store`
    is then only the operands' type).  The scales' exponent range starts at 3..7 and is widened upwards, one step at a time, until the
    reference exercises the rounding of the storage type (module docstring)."""
    cin, cout, k, stride, H, W, leaky, has_res, out_f32, B = case
    x, w, res, acc, bits = conv_operands(case)
    st = "f32" if out_f32 else store
    for e_hi in range(7, 16):
        scale, shift = final_affine(gen(cout, e_hi, 11), cout, 3, e_hi)
        o, out = epilogue(acc, scale, shift, leaky, res, st)
        if rounding_ok(o, st, leaky):
            break
    inexact, ties = rounding_stats(o, st)
    return dict(x=x, w=w, scale=scale, shift=shift, res=res, out=out, o=o, e_hi=e_hi, bits=bits, inexact=inexact, ties=ties, store=st)


# ------------------------------------------------------------------------------------------------ fp32 path
RECT_F32_CASES = [
    # cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B
    (24, 0, 0, 40, 3, 1, 13, 40, True, True, 2),        # wide, two channel groups (the second ragged), shortcut
    (32, 16, 1, 24, 1, 1, 26, 12, True, False, 2),      # tall, route [upsampled x2 | direct]
    (16, 0, 0, 32, 3, 2, 13, 20, True, False, 2),       # stride 2, odd and even side mixed
    # 3x3 over the route [upsampled x2 | direct]: halo and padding through >> up1, the route boundary on a stage boundary of
    # every stage size (4, 8, 16), both sources inside one stage loop
    (16, 16, 1, 24, 3, 1, 12, 20, True, True, 2),       # stride 1, shortcut, ragged channel group
    (16, 32, 1, 24, 3, 2, 12, 20, True, False, 1),      # stride 2: the upsampled source's halo meets the padding on the even / odd column split
]


def f32_case(c):
    """F32_CASES entry of test_gpu_parity -> the rectangular form"""
    cin1, cin2, up1, cout, k, stride, H, leaky, has_res, B = c
    return (cin1, cin2, up1, cout, k, stride, H, H, bool(leaky), bool(has_res), B)


@functools.lru_cache(maxsize=None)
def f32_reference(case):
    cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B = case
    g = gen(cin1, cin2, up1, cout, k, stride, H, W, B, 3)
    x1 = activations(g, (B, cin1, H >> up1, W >> up1))
    x2 = activations(g, (B, cin2, H, W)) if cin2 else None
    w = filters(g, (cout, cin1 + cin2, k, k))
    Ho, Wo = _out_hw(k, stride, H, W)
    res = residuals(g, (B, cout, Ho, Wo)) if has_res else None
    scale, shift = final_affine(g, cout)
    xin = x1.repeat_interleave(2, 2).repeat_interleave(2, 3) if up1 else x1
    if cin2:
        xin = torch.cat([xin, x2], 1)
    acc = conv_acc(xin, w, stride)
    o, out = epilogue(acc, scale, shift, leaky, res, "f32")
    return dict(x1=x1, x2=x2, xin=xin, w=w, scale=scale, shift=shift, res=res, out=out, bits=headroom_bits(xin, w, stride))


# ------------------------------------------------------------------------------------------------ two-layer kernels
RESBLOCK_CASES = [
    # C, H, W, B, leaky1, leaky2
    (64, 13, 13, 2, True, True),
    (64, 40, 40, 1, False, True),
    (64, 13, 40, 2, True, False),        # wide
    (128, 13, 13, 2, True, True),
    (128, 32, 32, 1, True, False),
    (128, 40, 13, 2, False, True),       # tall
]

STEM_FUSED_CASES = [
    # H, W, B
    (24, 72, 2),     # W % 4 == 0: the pipelined kernel; 36 output columns = two tiles, wide
    (72, 24, 1),     # the same kernel, tall
    (40, 40, 2),     # square
    (20, 70, 2),     # W % 4 != 0: the 4-byte-DMA kernel, wide
    (38, 38, 1),     # square, W % 4 == 2
]


def _second_stage(mid, w2, stride, leaky2, res, store):
    acc2 = conv_acc(mid, w2, stride)
    grid = grid_of(mid)
    bits = headroom_bits(mid, w2, stride, grid=grid)
    cout = w2.shape[0]
    for e_hi in range(7, 16):
        scale, shift = final_affine(gen(cout, e_hi, 13), cout, 3, e_hi)
        o, out = epilogue(acc2, scale, shift, leaky2, res, store)
        if rounding_ok(o, store, leaky2):
            break
    inexact, ties = rounding_stats(o, store)
    return dict(scale2=scale, shift2=shift, out=out, o=o, e_hi=e_hi, bits=bits, grid=grid, inexact=inexact, ties=ties)


@functools.lru_cache(maxsize=None)
def resblock_reference(case, store):
    """out = leaky2(bn2(conv3x3(mid))) + x, mid = round(leaky1(bn1(conv1x1(x)))): x in [-4, 4], w1 and w2 in [-2, 2]"""
    Cc, H, W, B, leaky1, leaky2 = case
    g = gen(Cc, H, W, B, 5)
    x = activations(g, (B, Cc, H, W))
    w1 = filters(g, (Cc // 2, Cc, 1, 1))
    w2 = filters(g, (Cc, Cc // 2, 3, 3))
    s1, t1 = stage1_affine(g, Cc // 2)
    mid, mid_inexact = first_stage(conv_acc(x, w1), s1, t1, leaky1, store)
    r = _second_stage(mid, w2, 1, leaky2, x, store)
    r.update(x=x, w1=w1, w2=w2, scale1=s1, shift1=t1, mid=mid, mid_inexact=mid_inexact, bits1=headroom_bits(x, w1))
    return r


@functools.lru_cache(maxsize=None)
def stem_fused_reference(case, store):
    """layer 0 (3x3 s1, 3 -> 32) + layer 1 (3x3 s2, 32 -> 64), each affine + LeakyReLU; image on the grid 1/16, filters in [-2, 2]"""
    H, W, B = case
    g = gen(H, W, B, 9)
    x = stem_image(g, (B, 3, H, W))
    w0 = filters(g, (32, 3, 3, 3))
    w1 = filters(g, (64, 32, 3, 3))
    s0, t0 = stage1_affine(g, 32)
    mid, mid_inexact = first_stage(conv_acc(x, w0), s0, t0, True, store)
    r = _second_stage(mid, w1, 2, True, None, store)
    r.update(x=x, w0=w0, w1=w1, scale1=s0, shift1=t0, mid=mid, mid_inexact=mid_inexact, bits1=headroom_bits(x, w0, grid=grid_of(x)))
    return r


CAT_CASES = [(64, 64, 128, 8, 8), (128, 64, 128, 26, 26), (64, 64, 128, 8, 20), (64, 128, 256, 26, 10)]   # c1, c2, cout, H, W


@functools.lru_cache(maxsize=None)
def cat_reference(case, store):
    """1x1 convolution (affine, LeakyReLU) over the route [nearest-x2-upsampled a | b], B = 2"""
    c1, c2, cout, H, W = case
    g = gen(c1, c2, cout, H, W, 37)
    a = activations(g, (2, c1, H // 2, W // 2))
    b = activations(g, (2, c2, H, W))
    w = filters(g, (cout, c1 + c2, 1, 1))
    xin = torch.cat([a.repeat_interleave(2, 2).repeat_interleave(2, 3), b], 1)
    acc = conv_acc(xin, w)
    for e_hi in range(7, 16):
        scale, shift = final_affine(gen(cout, e_hi, 41), cout, 3, e_hi)
        o, out = epilogue(acc, scale, shift, True, None, store)
        if rounding_ok(o, store, True):
            break
    inexact, ties = rounding_stats(o, store)
    return dict(a=a, b=b, xin=xin, w=w, scale=scale, shift=shift, out=out, o=o, e_hi=e_hi, bits=headroom_bits(xin, w), inexact=inexact, ties=ties)


STEM_CONV_CASES = [(20, 20, 2), (13, 70, 2), (66, 9, 1)]   # H, W, B: a block is 4 rows x 64 columns


@functools.lru_cache(maxsize=None)
def stem_conv_reference(case, store):
    """ay_stem_conv_fwd: 3x3 s1 3 -> 32 in fp32 from the fp32 image and fp32 filters, affine + LeakyReLU, one rounding"""
    H, W, B = case
    g = gen(H, W, B, 17)
    x = stem_image(g, (B, 3, H, W))
    w = filters(g, (32, 3, 3, 3))
    acc = conv_acc(x, w)
    for e_hi in range(7, 16):
        scale, shift = final_affine(gen(32, e_hi, 19), 32, 3, e_hi)
        o, out = epilogue(acc, scale, shift, True, None, store)
        if rounding_ok(o, store, True):
            break
    inexact, ties = rounding_stats(o, store)
    return dict(x=x, w=w, scale=scale, shift=shift, out=out, o=o, e_hi=e_hi, bits=headroom_bits(x, w, grid=grid_of(x)), inexact=inexact, ties=ties)


# ------------------------------------------------------------------------------------------------ training kernels
# cin, cout, k, stride, H, W, B; the last: 384 K steps, hence 16 split-K slabs and the 16-lane form of the slab reduction
RECT_WGRAD_CASES = [(32, 64, 3, 1, 13, 40, 2), (128, 256, 3, 2, 26, 14, 2), (256, 128, 1, 1, 40, 13, 2), (32, 64, 3, 1, 128, 96, 2)]


# the fp32 training kernels (any channel count): cin, cout, k, stride, H, W, B; the last two are rectangles
F32_GRAD_CASES = [(5, 7, 3, 1, 9, 9, 2), (6, 4, 3, 2, 11, 11, 2), (8, 3, 1, 1, 6, 6, 2), (4, 6, 3, 2, 8, 8, 2), (5, 7, 3, 1, 9, 14, 2), (6, 4, 3, 2, 11, 8, 2)]


def wgrad_case(c):
    cin, cout, k, s, H, B = c
    return (cin, cout, k, s, H, H, B)


@functools.lru_cache(maxsize=None)
def grad_reference(case, dz_range=4):
    """float64 autograd of F.conv2d on integer x, w, dz: -> dict(x, w, dz, dw, dx, bits_dw, bits_dx); dw and dx are exact integers"""
    cin, cout, k, s, H, W, B = case
    g = gen(cin, cout, k, s, H, W, B, 23)
    x = activations(g, (B, cin, H, W))
    w = filters(g, (cout, cin, k, k))
    Ho, Wo = _out_hw(k, s, H, W)
    dz = ints(g, (B, cout, Ho, Wo), dz_range)
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    F.conv2d(x64, w64, None, s, (k - 1) // 2).backward(dz.double())
    xa, wa = x.abs().double().requires_grad_(True), w.abs().double().requires_grad_(True)
    F.conv2d(xa, wa, None, s, (k - 1) // 2).backward(dz.abs().double())
    return dict(x=x, w=w, dz=dz, dw=to_f32_exact(w64.grad, "dW"), dx=to_f32_exact(x64.grad, "dx"),
                bits_dw=math.log2(max(float(wa.grad.max()), 1.0)), bits_dx=math.log2(max(float(xa.grad.max()), 1.0)))


DGRAD_S2_CASES = [
    # cin, cout, H, W, has_prev        cin_pad 32 / 64 / 128 select the kernel; cout is large so that sums pass 256 and get rounded
    (32, 256, 24, 24, True), (32, 256, 40, 24, False), (24, 256, 16, 40, True),        # cin_pad 32: 16x32 items from 16 rows of dz
    (32, 256, 36, 20, True), (24, 256, 24, 40, False),                                 # ... and each item size with the other has_prev
    (64, 256, 24, 24, False), (48, 256, 14, 40, True),
    (128, 256, 24, 24, True), (128, 512, 40, 14, False),
]
# The 1x1 data gradient of a residual block [1x1 C -> C/2, 3x3 C/2 -> C + shortcut] ACCUMULATES: the shortcut's backward has put dy into
# dx before it, so every bf16 training step runs the 1x1 forward kernels with a residual, in place (train_engine_bf16.py,
# `residual = out = dval[j]`).  cin, cout = C, C/2 as in the network: the forward kernel then sees C/2 -> C channels.
DGRAD_S1_ACC_1X1_CASES = [
    (64, 32, 1, 13, 40, True),        # 32 input channels (not a multiple of 64): the register-staged NK=1 kernel with a residual
    (128, 64, 1, 40, 13, True),       # BN=128 ring kernel, residual, canvas (6 tiles against 10)
    (128, 64, 1, 32, 32, True),       # the same, tiled image by image (no canvas saves a tenth of 8 tiles)
    (256, 128, 1, 13, 13, True),      # canvas; cout_pad % 256 == 0, turned away from the 256-wide tile by the residual
    (256, 128, 1, 32, 20, True),      # the same, image by image
    (512, 256, 1, 13, 13, True),      # canvas, four channel groups of 128, K loop of 4 stages
]
DGRAD_S1_CASES = [(32, 256, 3, 13, 13, True), (64, 256, 3, 13, 40, True), (128, 512, 1, 40, 13, False)] + DGRAD_S1_ACC_1X1_CASES   # cin, cout, k, H, W, has_prev
ACC_1X1_DZ_RANGE = 64


def dgrad_reference(case, stride):
    """data gradient (+ a gradient already accumulated, integers in [-8, 8]) rounded once to bfloat16.

    The accumulating 1x1 cases draw dz from [-64, 64]: with dz in [-4, 4] and the network's cout = cin / 2 their sums stay below 256,
    bfloat16 holds every one of them and no rounding would be tested.  Filters stay in [-2, 2]; sum |w| |dz| <= 256 * 2 * 64 = 2^15."""
    if stride == 2:
        cin, cout, H, W, has_prev = case
        k = 3
    else:
        cin, cout, k, H, W, has_prev = case
    wide = stride == 1 and k == 1 and has_prev
    key = (cin, cout, k, stride, H, W, 2)
    r = grad_reference(key, ACC_1X1_DZ_RANGE) if wide else grad_reference(key)
    prev = residuals(gen(cin, cout, H, W, 29), r["dx"].shape) if has_prev else None
    o = r["dx"] + prev if has_prev else r["dx"]
    if has_prev:
        assert torch.equal(o.double(), r["dx"].double() + prev.double()), "dx + prev is not exact in fp32"
    inexact, ties = rounding_stats(o, "bf16")
    return dict(w=r["w"], dz=r["dz"], dx=r["dx"], prev=prev, out=round_store(o, "bf16"), o=o, bits=r["bits_dx"], inexact=inexact, ties=ties)


STEM_TRAIN_CASES = [(2, 40, 72), (1, 24, 24), (2, 13, 132)]   # B, H, W (W % 4 == 0)


@functools.lru_cache(maxsize=None)
def stem_train_reference(case):
    """z = bf16(conv3x3(x, w)) and dW = autograd of the convolution; w in [-2, 2], dz in [-4, 4].  This forward has no scale to widen,
    so the image lies on the grid 1/64 (7 bits: exact in bfloat16): the sums then need up to 11 bits and their rounding is exercised"""
    B, H, W = case
    g = gen(B, H, W, 31)
    x = stem_image(g, (B, 3, H, W), 64)
    w = filters(g, (32, 3, 3, 3))
    dz = activations(g, (B, 32, H, W))
    x64, w64 = x.double(), w.double().requires_grad_(True)
    z64 = F.conv2d(x64, w64, None, 1, 1)
    z64.backward(dz.double())
    wa = w.abs().double().requires_grad_(True)
    F.conv2d(x64, wa, None, 1, 1).backward(dz.abs().double())
    o = to_f32_exact(z64.detach(), "z")
    inexact, ties = rounding_stats(o, "bf16")
    return dict(x=x, w=w, dz=dz, z=round_store(o, "bf16"), o=o, dw=to_f32_exact(w64.grad, "dW"), inexact=inexact, ties=ties,
                bits=headroom_bits(x, w, grid=1.0 / 64), bits_dw=math.log2(float(wa.grad.max()) * 64))
