"""Reference of the split-bf16 convolution ay_conv_fwd_split (TEST INFRASTRUCTURE ONLY -- never imported by the product):
THE SPLIT RULE of include/amyloid_yolo.h in torch, the convolution of the included plane products in float64, and the epilogue
restated in float32 steps, one IEEE operation each, as conv_exact_reference.py does.  Shared by tests/test_split_cpu.py (the
conditions, asserted on the reference alone) and tests/test_gpu_split.py (the kernel against it, bit for bit).

Plane-wiring cases.  Operand magnitudes come from LEVELS = {1, 1 + 2^-9, 1 + 2^-9 + 2^-17} with a random sign: they split to the
planes (1, 2^-9, 2^-17), a plane being zero where its term is absent, so every plane of every operand is 0 or a signed power of
two and every included product is a multiple of 2^-18 (the smallest, p1 q1).  Filters have at most 3 non-zero entries per output
channel, hence sum |x| |w| <= 3 * LEVELS[2]^2 < 4 = 2^20 * 2^-18: conv_exact_reference's HEADROOM_BITS rule on the grid 2^-18.
Any summation order of the included products leaves the same fp32 accumulator, and float64 gives its bits.  The affine step uses
scale[c] in {1, 2} and shift[c] = k / 16, |k| <= 32 (wiring_affine): |acc * scale + shift| < 16 on the grid 2^-18 is 22 bits, exact
in fp32, so conv_exact_reference.epilogue applies as it stands (it asserts that exactness); conv_exact_reference's own scales
2^-3 .. 2^-7 would push the low planes' contributions below the rounding of "+ shift" and hide them.

The magnitudes are drawn with probabilities LEVEL_P = (0.15, 0.25, 0.6), set on this reference alone so that each plane product
reaches at least half of the outputs of every case with a margin: an output sees three entries of a filter, and a plane term that
is present in k of them survives unless it cancels (k = 2, opposite signs).  For p2 (present with probability P) that leaves
3 P (1-P)^2 + 1.5 P^2 (1-P) + P^3 = 0.59 under a uniform draw (P = 1/3), before the borders take taps away, and 0.72 with P = 0.6.
"Integer" operands are +-1 (three entries per filter leave no room for more).
"""
import functools

import torch

import conv_exact_reference as R

INCLUDED = {2: [(0, 0), (0, 1), (1, 0)], 3: [(0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1)]}   # (activation plane, filter plane)
LEVELS = (1.0, 1.0 + 2.0 ** -9, 1.0 + 2.0 ** -9 + 2.0 ** -17)
LEVEL_P = (0.15, 0.25, 0.6)
PLANE_VALUES = (1.0, 2.0 ** -9, 2.0 ** -17)
WIRING_GRID = 2.0 ** -18
TAPS_PER_FILTER = 3
PATTERNS = ("x", "w", "xw")      # which operand is multi-level: activations | filters | both


def bf16_rne(t):
    return t.to(torch.bfloat16).to(torch.float32)


def split(x, n=3):
    """THE SPLIT RULE: float32 tensor -> n float32 tensors holding the bf16 planes (fp32 subtractions)"""
    assert x.dtype == torch.float32
    planes, r = [], x
    for _ in range(n):
        p = bf16_rne(r)
        planes.append(p)
        r = r - p
    return planes


def plane_products(xin, w, stride):
    """{(a, b): float64 convolution of activation plane a with filter plane b} for the six products of nsplit = 3"""
    px, pw = split(xin), split(w)
    return {ab: R.conv_acc(px[ab[0]], pw[ab[1]], stride) for ab in INCLUDED[3]}


def split_acc(products, nsplit, without=None):
    """the accumulator ay_conv_fwd_split holds: the sum of the included plane products (`without`: one of them left out)"""
    return sum(products[ab] for ab in INCLUDED[nsplit] if ab != without)


def epilogue_f32(acc64, scale, shift, leaky, res):
    """the fp32 kernel's epilogue in float32 steps (acc * scale + shift asserted exact, LeakyReLU, + residual): fp32 output"""
    return R.epilogue(acc64, scale, shift, leaky, res, "f32")[1]


def wiring_affine(g, c):
    """scale[c] in {1, 2}, shift[c] = k / 16 with |k| <= 32"""
    e = torch.randint(0, 2, (c,), generator=g)
    k = torch.randint(-32, 33, (c,), generator=g)
    return torch.pow(2.0, e.to(torch.float32)), k.to(torch.float32) / 16.0


# ---------------------------------------------------------------------------------------------- plane-wiring cases
WIRING_CASES = [
    # cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B     (the form of conv_exact_reference.RECT_F32_CASES)
    (32, 0, 0, 64, 3, 1, 33, 33, True, True, 2),        # 3x3 s1, one pixel into the second tile column / fifth tile row, residual
    (32, 0, 0, 40, 3, 2, 13, 13, True, False, 1),       # 3x3 s2, odd input (13 -> 7), ragged channel group
    (128, 256, 1, 64, 1, 1, 26, 26, True, False, 1),    # 1x1 over the route [upsampled x2 | direct]
    (3, 0, 0, 32, 3, 1, 70, 70, True, False, 2),        # stem: 3 channels in a stage of 16, ragged tiles
]


def _signs(g, shape):
    return torch.randint(0, 2, tuple(shape), generator=g).to(torch.float32) * 2.0 - 1.0


def _levels(g, shape, multi):
    s = _signs(g, shape)
    if not multi:
        return s
    n = int(torch.Size(shape).numel())
    idx = torch.multinomial(torch.tensor(LEVEL_P), n, replacement=True, generator=g).view(tuple(shape))
    return s * torch.tensor(LEVELS, dtype=torch.float32)[idx]


def _sparse_filters(g, cout, cin, k, multi):
    """at most TAPS_PER_FILTER non-zero entries per output channel, at seeded positions over all (ci, tap)"""
    n = cin * k * k
    pos = torch.randint(0, n, (cout, TAPS_PER_FILTER), generator=g)
    mask = torch.zeros(cout, n)
    mask.scatter_(1, pos, 1.0)
    return (_levels(g, (cout, n), multi) * mask).view(cout, cin, k, k)


@functools.lru_cache(maxsize=None)
def wiring_operands(case, pattern):
    cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B = case
    g = R.gen(cin1, cin2, up1, cout, k, stride, H, W, B, PATTERNS.index(pattern), 43)
    xm, wm = "x" in pattern, "w" in pattern
    x1 = _levels(g, (B, cin1, H >> up1, W >> up1), xm)
    x2 = _levels(g, (B, cin2, H, W), xm) if cin2 else None
    w = _sparse_filters(g, cout, cin1 + cin2, k, wm)
    Ho, Wo = R._out_hw(k, stride, H, W)
    res = R.residuals(g, (B, cout, Ho, Wo)) if has_res else None
    scale, shift = wiring_affine(g, cout)
    xin = x1.repeat_interleave(2, 2).repeat_interleave(2, 3) if up1 else x1
    if cin2:
        xin = torch.cat([xin, x2], 1)
    return dict(x1=x1, x2=x2, xin=xin, w=w, scale=scale, shift=shift, res=res, products=plane_products(xin, w, stride))


@functools.lru_cache(maxsize=None)
def wiring_reference(case, pattern, nsplit):
    """-> the operands of wiring_operands plus `out`, the bits ay_conv_fwd_split(nsplit) must produce"""
    r = dict(wiring_operands(case, pattern))
    r["out"] = epilogue_f32(split_acc(r["products"], nsplit), r["scale"], r["shift"], case[8], r["res"])
    return r


def wiring_without(case, pattern, nsplit, ab):
    """the output with the included plane product `ab` left out"""
    r = wiring_operands(case, pattern)
    return epilogue_f32(split_acc(r["products"], nsplit, without=ab), r["scale"], r["shift"], case[8], r["res"])


def populated(pattern, ab):
    """does the pattern give the plane product `ab` non-zero planes on both sides?  (an operand of +-1 has p1 = p2 = 0)"""
    a, b = ab
    return (a == 0 or "x" in pattern) and (b == 0 or "w" in pattern)
