"""CPU (no GPU needed): the conditions the exact convolution tests rest on, asserted on the REFERENCE of every case of every list
tests/test_gpu_conv_exact.py runs (tests/conv_exact_reference.py, module docstring):

  * headroom: no output needs more than 2^20 grid units of sum |a_i| |b_i| -- fp32 holds every partial sum in any order, with 4 bits
    to spare;
  * order independence, demonstrated: an fp32 convolution and an fp32 sum taken in REVERSED channel order both equal the float64
    result bit for bit (what lets one reference serve MFMA shapes, split-K slabs, atomics and fmaf chains alike);
  * the rounding of the storage type is exercised: LeakyReLU cases have at least 25 % of the outputs not representable before
    the rounding, every 16-bit case has at least 100 exact ties; bfloat16 intermediates of the two-layer kernels change under
    their rounding in at least 1 % of the values.

`PYTHONPATH=. python tests/test_conv_exact_cpu.py` prints the per-case table kept in profiles/conv_exact_margins.txt."""
import pytest
import torch
import torch.nn.functional as F

import conv_exact_reference as R
from test_gpu_parity import CONV_CASES, F32_CASES
from test_gpu_train_bf16 import WGRAD_CASES

SINGLE = [R.conv_case(c) for c in CONV_CASES] + R.SQUARE_CONV_CASES + R.RECT_CONV_CASES
SINGLE += [c for c in R.M16_CASES + R.M16_RECT_CASES if c not in SINGLE]      # the direct ay_conv3x3_m16_fwd_* calls
FP32 = [R.f32_case(c) for c in F32_CASES] + R.RECT_F32_CASES
GRADS = [R.wgrad_case(c) for c in WGRAD_CASES] + R.RECT_WGRAD_CASES + R.F32_GRAD_CASES
ids = lambda c: "x".join(str(int(v)) for v in c)


def order_independent(x, w, stride, acc64):
    """fp32 convolution, and fp32 with the input channels (hence the order of the sum) reversed: both the float64 bits"""
    pad = (w.shape[-1] - 1) // 2
    a = F.conv2d(x, w, None, stride, pad)
    b = F.conv2d(x.flip(1).contiguous(), w.flip(1).contiguous(), None, stride, pad)
    return torch.equal(a.double(), acc64) and torch.equal(b.double(), acc64)


def rounding_exercised(r, store, leaky):
    if store == "f32":
        return
    assert r["ties"] >= R.MIN_TIES, r["ties"]
    if leaky:
        assert r["inexact"] >= R.MIN_INEXACT_LEAKY, r["inexact"]
    # the stored values are those of the storage type, and the reference disagrees with truncation somewhere
    assert torch.equal(r["out"], r["out"].to(R.STORE[store]).float())
    shift = 16 if store == "bf16" else 13
    trunc = ((r["o"].contiguous().view(torch.int32) >> shift) << shift).view(torch.float32)
    assert bool((trunc != r["out"]).any())


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("case", SINGLE, ids=ids)
def test_single_layer_reference(case, store):
    cin, cout, k, stride, H, W, leaky, has_res, out_f32, B = case
    r = R.conv_reference(case, store)
    assert r["bits"] <= R.HEADROOM_BITS, r["bits"]
    x, w, res, acc, _ = R.conv_operands(case)
    assert order_independent(x, w, stride, acc)
    for t in (x, w) + ((res,) if has_res else ()):      # operands are exact in the storage type
        assert torch.equal(t, t.to(R.STORE[store]).float())
    rounding_exercised(r, r["store"], leaky)


@pytest.mark.parametrize("case", FP32, ids=ids)
def test_f32_reference(case):
    r = R.f32_reference(case)
    assert r["bits"] <= R.HEADROOM_BITS
    assert order_independent(r["xin"], r["w"], case[5], R.conv_acc(r["xin"], r["w"], case[5]))


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("case", R.CAT_CASES, ids=ids)
def test_route_reference(case, store):
    r = R.cat_reference(case, store)
    assert r["bits"] <= R.HEADROOM_BITS
    assert order_independent(r["xin"], r["w"], 1, R.conv_acc(r["xin"], r["w"]))
    rounding_exercised(r, store, True)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("case", R.STEM_CONV_CASES, ids=ids)
def test_stem_conv_reference(case, store):
    r = R.stem_conv_reference(case, store)
    assert r["bits"] <= R.HEADROOM_BITS
    assert order_independent(r["x"], r["w"], 1, R.conv_acc(r["x"], r["w"]))
    rounding_exercised(r, store, True)


def two_layer(r, store, w_first, w_second, stride2, leaky2):
    assert r["bits1"] <= R.HEADROOM_BITS and r["bits"] <= R.HEADROOM_BITS, (r["bits1"], r["bits"])
    assert order_independent(r["x"], w_first, 1, R.conv_acc(r["x"], w_first))
    mid = r["mid"]
    assert torch.equal(mid, mid.to(R.STORE[store]).float())
    assert order_independent(mid, w_second, stride2, R.conv_acc(mid, w_second, stride2))
    if store == "bf16":     # (a half holds every intermediate of these ranges exactly: its 11 bits are more than the first stage needs)
        assert r["mid_inexact"] >= 0.01, r["mid_inexact"]
    rounding_exercised(r, store, leaky2)


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("case", R.RESBLOCK_CASES, ids=ids)
def test_resblock_reference(case, store):
    r = R.resblock_reference(case, store)
    assert r["grid"] >= 2.0 ** -3      # the x10 scales keep the intermediate on the grid 2^-3 through the LeakyReLU
    two_layer(r, store, r["w1"], r["w2"], 1, case[5])


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("case", R.STEM_FUSED_CASES, ids=ids)
def test_stem_fused_reference(case, store):
    r = R.stem_fused_reference(case, store)
    assert r["grid"] >= 2.0 ** -7      # image on 1/16, scales 10 * 2^-e, e <= 3
    two_layer(r, store, r["w0"], r["w1"], 2, True)


@pytest.mark.parametrize("case", GRADS, ids=ids)
def test_gradient_reference(case):
    """dW and dx of float64 autograd are integers fp32 holds, and fp32 autograd (another order again) gives the same bits"""
    cin, cout, k, s, H, W, B = case
    r = R.grad_reference(case)
    assert r["bits_dw"] <= R.HEADROOM_BITS and r["bits_dx"] <= R.HEADROOM_BITS, (r["bits_dw"], r["bits_dx"])
    for flip in (False, True):
        x = (r["x"].flip(1) if flip else r["x"]).clone().requires_grad_(True)
        w = (r["w"].flip(1) if flip else r["w"]).clone().requires_grad_(True)
        F.conv2d(x, w, None, s, (k - 1) // 2).backward(r["dz"])
        assert torch.equal(w.grad.flip(1) if flip else w.grad, r["dw"]) and torch.equal(x.grad.flip(1) if flip else x.grad, r["dx"])


@pytest.mark.parametrize("case", [(c, 2) for c in R.DGRAD_S2_CASES] + [(c, 1) for c in R.DGRAD_S1_CASES], ids=lambda c: f"s{c[1]}_" + ids(c[0]))
def test_data_gradient_reference(case):
    r = R.dgrad_reference(*case)
    assert r["bits"] <= R.HEADROOM_BITS
    assert r["ties"] >= R.MIN_TIES, r["ties"]       # sums beyond 256 meet bfloat16's rounding; no LeakyReLU here
    assert torch.equal(r["out"], r["out"].to(torch.bfloat16).float())


@pytest.mark.parametrize("case", R.DGRAD_S1_ACC_1X1_CASES, ids=ids)
def test_accumulating_1x1_data_gradient_reference(case):
    """the 1x1 data gradient onto a gradient already in dx: dx + prev is exact in fp32 and meets bfloat16's rounding (ties), and the
    two wrong kernels an exact comparison must tell from the right one each differ from it in at least 100 values"""
    cin, cout, k, H, W, has_prev = case
    assert k == 1 and has_prev
    r = R.dgrad_reference(case, 1)
    assert r["bits"] <= R.HEADROOM_BITS
    for t in (r["dz"], r["w"], r["prev"]):      # operands are exact in bfloat16
        assert torch.equal(t, t.to(torch.bfloat16).float())
    assert torch.equal(R.to_f32_exact(r["dx"].double() + r["prev"].double(), "dx + prev"), r["o"])
    assert r["ties"] >= R.MIN_TIES, r["ties"]
    rounds_first = R.round_store(R.round_store(r["dx"], "bf16") + r["prev"], "bf16")      # (a) rounds before the residual add
    drops_residual = R.round_store(r["dx"], "bf16")                                         # (b) no residual
    assert int((rounds_first != r["out"]).sum()) >= 100, int((rounds_first != r["out"]).sum())
    assert int((drops_residual != r["out"]).sum()) >= 100, int((drops_residual != r["out"]).sum())


@pytest.mark.parametrize("case", R.STEM_TRAIN_CASES, ids=ids)
def test_stem_train_reference(case):
    r = R.stem_train_reference(case)
    assert r["bits"] <= R.HEADROOM_BITS and r["bits_dw"] <= R.HEADROOM_BITS, (r["bits"], r["bits_dw"])
    assert torch.equal(r["x"], r["x"].to(torch.bfloat16).float())
    assert r["ties"] >= R.MIN_TIES and r["inexact"] >= 0.1, (r["ties"], r["inexact"])
    assert order_independent(r["x"], r["w"], 1, R.conv_acc(r["x"], r["w"]))


def margins():
    rows = ["# per case, measured on the reference alone: bits = log2(max sum|a||b| / grid) (limit 20), inexact = share of outputs the",
            "# storage type cannot hold before the rounding, ties = outputs exactly half way between two stored values, e_hi = largest",
            "# scale exponent after widening (3..e_hi), mid_inexact = share of the 16-bit intermediates changed by their rounding",
            "# PYTHONPATH=. python tests/test_conv_exact_cpu.py > profiles/conv_exact_margins.txt"]
    for store in ("bf16", "f16"):
        for c in SINGLE:
            r = R.conv_reference(c, store)
            rows.append(f"conv_fwd {store} {ids(c)}: bits {r['bits']:.1f} e_hi {r['e_hi']} inexact {r['inexact']:.3f} ties {r['ties']} of {r['o'].numel()}")
        for name, cases, fn in (("cat1x1", R.CAT_CASES, R.cat_reference), ("stem_conv", R.STEM_CONV_CASES, R.stem_conv_reference)):
            for c in cases:
                r = fn(c, store)
                rows.append(f"{name} {store} {ids(c)}: bits {r['bits']:.1f} e_hi {r['e_hi']} inexact {r['inexact']:.3f} ties {r['ties']} of {r['o'].numel()}")
        for name, cases, fn in (("resblock", R.RESBLOCK_CASES, R.resblock_reference), ("stem_fused", R.STEM_FUSED_CASES, R.stem_fused_reference)):
            for c in cases:
                r = fn(c, store)
                rows.append(f"{name} {store} {ids(c)}: bits stage1 {r['bits1']:.1f} stage2 {r['bits']:.1f} (grid 2^{int(torch.log2(torch.tensor(r['grid'])))}) "
                            f"mid_inexact {r['mid_inexact']:.3f} e_hi {r['e_hi']} inexact {r['inexact']:.3f} ties {r['ties']} of {r['o'].numel()}")
    for c in FP32:
        rows.append(f"conv_f32 {ids(c)}: bits {R.f32_reference(c)['bits']:.1f}")
    for c in GRADS:
        r = R.grad_reference(c)
        rows.append(f"grad {ids(c)}: bits dW {r['bits_dw']:.1f} dx {r['bits_dx']:.1f}")
    for s, cases in ((2, R.DGRAD_S2_CASES), (1, R.DGRAD_S1_CASES)):
        for c in cases:
            r = R.dgrad_reference(c, s)
            rows.append(f"dgrad_s{s} bf16 {ids(c)}: bits {r['bits']:.1f} inexact {r['inexact']:.3f} ties {r['ties']} of {r['o'].numel()}")
    for c in R.STEM_TRAIN_CASES:
        r = R.stem_train_reference(c)
        rows.append(f"stem_train bf16 {ids(c)}: bits z {r['bits']:.1f} dW {r['bits_dw']:.1f} inexact {r['inexact']:.3f} ties {r['ties']} of {r['o'].numel()}")
    return rows


if __name__ == "__main__":
    print("\n".join(margins()))
