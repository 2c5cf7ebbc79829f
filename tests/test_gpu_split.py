"""GPU (-m gpu): ay_conv_fwd_split and precision="bf16x3" / "bf16x6" (THE SPLIT RULE, include/amyloid_yolo.h).

  1. geometry: the integer cases of the fp32 kernel (operands exact in bf16: p1 = p2 = 0) must give conv_exact_reference's bits;
  2. plane wiring: operands whose planes are (1, 2^-9, 2^-17) against the float64 sum of the INCLUDED plane products, bit for bit
     (tests/split_reference.py; tests/test_split_cpu.py holds the conditions): a product wired to the wrong plane, left out, or added
     where nsplit = 2 must leave it out, changes at least half of the outputs;
  3. random operands against float64 with the bound derived from the dropped terms;
  4. / 5. the whole model against the reference fixtures (bf16x6) and against the fp32 and fp16 paths (bf16x3);
  6. stability."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_exact_reference as R
import golden_cases as gc
import split_reference as SR
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd import utils as ay
from amyloid_yolo_paper_amd._lib import ConvDesc, check, ptr
from test_gpu_conv_exact import Guarded
from test_gpu_parity import F32_CASES, TOL, build_models, close, load

pytestmark = pytest.mark.gpu
ids = lambda c: "x".join(str(int(v)) for v in c)
NSPLITS = [2, 3]
AY_ERR_ARG = -1


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def refused(case):
    """a route whose first source is not a multiple of the 16-channel stage"""
    return case[1] > 0 and case[0] % 16 != 0


def call_split(dev, case, r, nsplit, out):
    """-> return code of ay_conv_fwd_split on the operands r[x1, x2, w, scale, shift, res] of a case in the rectangular f32 form"""
    cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B = case
    Ho, Wo = R._out_hw(k, stride, H, W)
    d = ConvDesc(B, cin1 + cin2, cout, H, W, Ho, Wo, k, stride, int(leaky), 0, cout)
    x1d, wd, scd, shd = (r[k_].to(dev) for k_ in ("x1", "w", "scale", "shift"))
    x2d = None if r["x2"] is None else r["x2"].to(dev)
    rd = None if r["res"] is None else r["res"].to(dev)
    rc = _lib.lib().ay_conv_fwd_split(C.byref(d), ptr(x1d), cin1, up1, ptr(x2d), ptr(wd), ptr(scd), ptr(shd), ptr(rd), ptr(out), nsplit,
                                     _lib.stream_ptr())
    torch.cuda.synchronize()
    return rc


def assert_refused(dev, case, r, nsplit):
    cin1, cin2, up1, cout, k, stride, H, W, leaky, has_res, B = case
    Ho, Wo = R._out_hw(k, stride, H, W)
    out = Guarded((B, cout, Ho, Wo), "f32", dev)
    rc = call_split(dev, case, r, nsplit, out.t)
    assert rc == AY_ERR_ARG
    assert len(_lib.lib().ay_last_error()) > 0
    assert bool(torch.isnan(out.t).all()) and out.intact()      # untouched: still the NaN fill


# ------------------------------------------------------------------------------------------- 1. geometry
def run_geometry(dev, case, nsplit):
    r = R.f32_reference(case)
    if refused(case):
        return assert_refused(dev, case, r, nsplit)
    out = Guarded(tuple(r["out"].shape), "f32", dev)
    assert call_split(dev, case, r, nsplit, out.t) == 0, _lib.lib().ay_last_error()
    got = out.t.cpu()
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"ay_conv_fwd_split nsplit={nsplit} {ids(case)}")


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("case", [R.f32_case(c) for c in F32_CASES], ids=ids)
def test_split_geometry_exact(dev, case, nsplit):
    """integer operands in [-4, 4] are exact in bf16: the lower planes are zero and the result is the fp32 kernel's, bit for bit
    (the route with cin1 = 24 is refused: AY_ERR_ARG, a message, the output untouched)"""
    run_geometry(dev, case, nsplit)


@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("case", R.RECT_F32_CASES, ids=ids)
def test_split_geometry_exact_rect(dev, case, nsplit):
    run_geometry(dev, case, nsplit)


def test_split_refusals(dev):
    """what the kernel does not cover is refused, never run on another arithmetic"""
    L = _lib.lib()
    t = torch.zeros(1 << 16, device=dev)
    out = torch.full((1 << 16,), float("nan"), device=dev)

    def rc(d, cin1=None, nsplit=3, src2=None):
        r = L.ay_conv_fwd_split(C.byref(d), ptr(t), d.cin if cin1 is None else cin1, 0, ptr(src2), ptr(t), ptr(t), ptr(t), None, ptr(out),
                                nsplit, _lib.stream_ptr())
        torch.cuda.synchronize()
        return r

    ok = ConvDesc(1, 16, 16, 8, 8, 8, 8, 3, 1, 1, 0, 16)
    for nsplit in (0, 1, 4, 6):
        assert rc(ok, nsplit=nsplit) == AY_ERR_ARG and b"nsplit" in L.ay_last_error()
    assert rc(ConvDesc(1, 16, 16, 8, 8, 8, 8, 5, 1, 1, 0, 16)) == AY_ERR_ARG and len(L.ay_last_error()) > 0      # 5x5
    assert rc(ConvDesc(1, 16, 16, 8, 8, 4, 4, 1, 2, 1, 0, 16)) == AY_ERR_ARG and len(L.ay_last_error()) > 0      # 1x1 stride 2
    assert rc(ConvDesc(1, 32, 16, 8, 8, 8, 8, 1, 1, 1, 0, 16), cin1=8, src2=t) == AY_ERR_ARG and b"16" in L.ay_last_error()
    assert rc(ConvDesc(1, 1 << 10, 16, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 1, 1, 1, 0, 16)) == AY_ERR_ARG        # 4 GiB image
    assert b"32-bit" in L.ay_last_error()
    assert bool(torch.isnan(out).all())


# ------------------------------------------------------------------------------------------- 2. plane wiring
@pytest.mark.parametrize("nsplit", NSPLITS)
@pytest.mark.parametrize("pattern", SR.PATTERNS)
@pytest.mark.parametrize("case", SR.WIRING_CASES, ids=ids)
def test_split_plane_wiring_exact(dev, case, pattern, nsplit):
    r = SR.wiring_reference(case, pattern, nsplit)
    out = Guarded(tuple(r["out"].shape), "f32", dev)
    assert call_split(dev, case, r, nsplit, out.t) == 0, _lib.lib().ay_last_error()
    got = out.t.cpu()
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"ay_conv_fwd_split nsplit={nsplit} {pattern} {ids(case)}")


# ------------------------------------------------------------------------------------------- 3. random operands
DROPPED = {2: 3 * 2.0 ** -16, 3: 2.0 ** -22}     # the plane products a mode leaves out, relative to |x| |w| (the rule's residual bounds)


def random_operands(case):
    """the operands of test_gpu_parity.test_conv_f32_mfma_kernel (same generator, same order of draws)"""
    cin1, cin2, up1, cout, k, stride, H, leaky, has_res, B = case
    g = torch.Generator().manual_seed(cin1 * 3 + cin2 + cout + k + H)
    cin = cin1 + cin2
    h1 = H >> up1
    x1 = torch.randn(B, cin1, h1, h1, generator=g)
    x2 = torch.randn(B, cin2, H, H, generator=g) if cin2 else None
    w = torch.randn(cout, cin, k, k, generator=g) * (1.0 / np.sqrt(cin * k * k))
    scale = torch.rand(cout, generator=g) + 0.5
    shift = torch.randn(cout, generator=g) * 0.1
    pad = (k - 1) // 2
    Ho = (H + 2 * pad - k) // stride + 1
    res = torch.randn(B, cout, Ho, Ho, generator=g) if has_res else None
    return dict(x1=x1, x2=x2, w=w, scale=scale, shift=shift, res=res)


@pytest.mark.parametrize("case", F32_CASES, ids=ids)
def test_split_random_operands_bound(dev, case):
    """|err| <= c * sum |x| |w| * |scale| + 2 * E32 per element against float64: c = the dropped plane products (3 * 2^-16 | 2^-22),
    E32 = the largest error of ay_conv_fwd_f32 on the same operands against the same reference, measured here; the factor 2 covers
    six accumulated terms per product where fp32 has one"""
    cin1, cin2, up1, cout, k, stride, H, leaky, has_res, B = case
    rect = R.f32_case(case)
    r = random_operands(case)
    if refused(rect):
        for nsplit in NSPLITS:
            assert_refused(dev, rect, r, nsplit)
        return
    L = _lib.lib()
    xin = r["x1"].repeat_interleave(2, 2).repeat_interleave(2, 3) if up1 else r["x1"]
    if cin2:
        xin = torch.cat([xin, r["x2"]], 1)
    pad = (k - 1) // 2
    sc, sh = r["scale"].double().view(1, -1, 1, 1), r["shift"].double().view(1, -1, 1, 1)
    ref = F.conv2d(xin.double(), r["w"].double(), None, stride, pad) * sc + sh
    if leaky:
        ref = F.leaky_relu(ref, 0.1)
    if has_res:
        ref = ref + r["res"].double()
    mag = F.conv2d(xin.double().abs(), r["w"].double().abs(), None, stride, pad) * sc.abs()
    Ho = ref.shape[2]
    d = ConvDesc(B, cin1 + cin2, cout, H, H, Ho, Ho, k, stride, int(leaky), 0, cout)
    x1d, wd, scd, shd = (r[k_].to(dev) for k_ in ("x1", "w", "scale", "shift"))
    x2d = None if r["x2"] is None else r["x2"].to(dev)
    rd = None if r["res"] is None else r["res"].to(dev)
    out = torch.full(tuple(ref.shape), float("nan"), device=dev)
    check(L.ay_conv_fwd_f32(C.byref(d), ptr(x1d), cin1, up1, ptr(x2d), ptr(wd), ptr(scd), ptr(shd), ptr(rd), ptr(out), _lib.stream_ptr()),
          "ay_conv_fwd_f32")
    e32 = float((out.cpu().double() - ref).abs().max())
    worst = {}
    for nsplit in NSPLITS:
        out.fill_(float("nan"))
        assert call_split(dev, rect, r, nsplit, out) == 0, L.ay_last_error()
        got = out.cpu().double()
        assert bool(torch.isfinite(got).all())
        err = (got - ref).abs()
        bound = DROPPED[nsplit] * mag + 2.0 * e32
        worst[nsplit] = float(err.max())
        print(f"split random {ids(case)} nsplit={nsplit}: max err {worst[nsplit]:.3e}, E32 {e32:.3e}, max err/bound {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (nsplit, worst[nsplit], e32, float((err / bound).max()))
    if k == 3 and cin1 + cin2 >= 128:
        assert worst[2] > worst[3], worst       # the two modes cannot be the same code


# ------------------------------------------------------------------------------------------- 4. model, bf16x6
def inference(m, x):
    """m(x) in eval mode; test_gpu_parity.build_models caches its models per session and another module may have left one in
    training mode, which is put back"""
    was = m.training
    m.eval()
    try:
        return m(x)
    finally:
        m.train(was)


@pytest.mark.parametrize("case", gc.MODEL_CASES, ids=lambda c: c[0])
def test_model_bf16x6_vs_reference_fixtures(golden_dir, tmp_cfg_dir, dev, case):
    """precision='bf16x6' meets the fp32 path's bar against the reference's CPU path: boxes and sampled layer outputs within 1e-4,
    NMS counts equal, kept indices bit-exact (the assertions of test_gpu_parity.test_model_fp32_vs_reference_fixtures, same TOL).

    The value that decides is on c2_s160_b1: in the merged NMS rows the corner y1 = cy - h/2 = 0.0045 of a box that touches the top edge
    (row 8; cy = h/2 = 134.4) is compared absolutely because |y1| < 1, so the bar is 6.5 units of 2^-16, the last place of the two
    numbers y1 is the difference of.  With all six plane products in one accumulator set the kernel was 14 units away and this case
    failed; the correction products have had an accumulator set of their own since (profiles/split_path.txt)."""
    name, C_, S, B, start = case
    z = load(golden_dir, "model_" + name)
    m, _ = build_models(C_, tmp_cfg_dir, dev, "bf16x6")
    m.keep_layer_outputs = True
    try:
        x = torch.from_numpy(gc.model_inputs(S, B, start))
        out = inference(m, x)
        assert not out.is_cuda and out.shape == (B, m.num_boxes(S), 5 + C_)
        if "out" in z:
            close(out.numpy(), z["out"], TOL, "boxes")
        else:
            close(out.numpy()[:, z["out_rows"]], z["out_sel"], TOL, "boxes")
        for k, li in enumerate(z["layer_idx"]):
            li = int(li)
            if li not in m.layer_outputs:
                continue  # conv fused into the following shortcut: its own output is never materialised
            f = m.layer_output_nchw(li).cpu().numpy().reshape(-1)
            close(f[z["samp_idx"][k]], z["samp_val"][k], TOL, f"layer {li}")
        res = ay.non_max_suppression(out, 0.5, 0.4)
        for b in range(B):
            n = int(z[f"nms_n{b}"])
            assert (0 if res[b] is None else res[b].shape[0]) == n
            if n:
                np.testing.assert_array_equal(res.keep_idx[b], z[f"nms_keep{b}"])   # bit-exact box indices after NMS
                close(res[b].numpy(), z[f"nms_rows{b}"], TOL, "nms rows")
    finally:
        m.keep_layer_outputs = False


# ------------------------------------------------------------------------------------------- 5. model, bf16x3
def deviation(a, b):
    """largest |a - b| / max(1, |b|): the measure of test_gpu_parity.close"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max(initial=0.0))


@pytest.mark.parametrize("case", [c for c in gc.MODEL_CASES if c[2] <= 416], ids=lambda c: c[0])
def test_model_bf16x3_between_fp32_and_fp16(tmp_cfg_dir, dev, case):
    """rows the fp32 path gives a confidence above 0.5: bf16x3 deviates from the fp32 path by at most 1/8 of what fp16 does (the
    rounding steps are 2^-16 and 2^-11: a ratio of 2^-5, times 4 for propagation through the activations)"""
    name, C_, S, B, start = case
    x = torch.from_numpy(gc.model_inputs(S, B, start))
    outs = {}
    for precision in ("fp32", "bf16x3", "fp16"):
        m, _ = build_models(C_, tmp_cfg_dir, dev, precision)
        outs[precision] = inference(m, x)
    sel = outs["fp32"][..., 4] > 0.5
    assert int(sel.sum()) > 0, "no confident row in this fixture"
    ref = outs["fp32"][sel].numpy()
    d3, d16 = deviation(outs["bf16x3"][sel].numpy(), ref), deviation(outs["fp16"][sel].numpy(), ref)
    keep = {p: ay.non_max_suppression(o, 0.5, 0.4).keep_idx for p, o in outs.items()}
    same = all(np.array_equal(a, b) for a, b in zip(keep["bf16x3"], keep["fp32"]))
    dconf = float((outs["bf16x3"][..., 4] - outs["fp32"][..., 4]).abs().max())
    print(f"bf16x3 {name}: {int(sel.sum())} rows, deviation {d3:.3e} (fp16 {d16:.3e}, ratio {d3 / max(d16, 1e-300):.4f}), "
          f"kept indices equal to fp32's: {same}, largest confidence difference {dconf:.3e}")
    assert d3 <= d16 / 8.0, (d3, d16)


# ------------------------------------------------------------------------------------------- 6. stability
def test_split_modes_are_stable_and_independent(tmp_cfg_dir, dev):
    """a second forward returns identical bits; interleaving models of other precisions built from the same weights changes none"""
    name, C_, S, B, start = gc.MODEL_CASES[1]
    x = torch.from_numpy(gc.model_inputs(S, B, start))
    order = ["bf16x6", "bf16x6", "fp32", "bf16x3", "bf16x6", "bf16", "bf16x3", "fp32", "bf16x3"]
    first = {}
    for precision in order:
        m, _ = build_models(C_, tmp_cfg_dir, dev, precision)
        out = inference(m, x).clone()
        assert bool(torch.isfinite(out).all())
        if precision in first:
            assert torch.equal(out, first[precision]), precision
        first[precision] = out
    assert not torch.equal(first["bf16x3"], first["bf16x6"])     # the modes are different arithmetic
