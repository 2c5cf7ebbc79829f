"""GPU (-m gpu): the gradient plumbing of the bf16 training step -- ay_accumulate_bf16, ay_slice_accumulate_bf16,
ay_zero_insert_bf16 (csrc/ay_train_bf16.hip) -- against the EXACT reference of tests/plumbing_reference.py: integer operands in
[-255, 255], every sum exact in fp32 in any order, so the comparison is equality with the float64 sum rounded once to bfloat16 (no
tolerance).  tests/test_grad_plumbing_cpu.py holds the conditions this rests on (ties, and the mutants each case separates).

What this pins beyond test_bn_train_bf16_fwd_bwd_and_plumbing (one call each, the upsample backward within 2e-2): fp32 adds and ONE
rounding, to nearest even; the upsample backward ONTO a gradient (what the engine issues whenever the source already has one) and from
a slice that does not start at channel 0; rectangles; the plane offset (channels outside the slice hold a large value); a destination
that is written, not added to, without `accumulate` (it starts as NaN); the grid-stride second pass beyond 65535 workgroups; stores
confined to the destination (guard bands) and sources left alone."""
import pytest
import torch

import conv_exact_reference as R
import plumbing_reference as P
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from test_gpu_conv_exact import Guarded, blocked, ids, unblocked

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


@pytest.mark.parametrize("case", P.SLICE_CASES, ids=ids)
def test_slice_accumulate_exact(dev, case):
    """route backward (up = 0) and upsample backward (up = 1), written and accumulated, slices at channel 0, 16 and 32 of 64"""
    up, acc, c0, csrc, h, w = case
    L = _lib.lib()
    r = P.slice_reference(case)
    doutb = blocked("bf16", r["dout"], dev)
    kept = doutb.clone()
    dsrc = Guarded((P.BATCH, csrc // 16, h >> up, w >> up, 16), "bf16", dev)      # NaN unless a gradient is already there
    if acc:
        dsrc.t.copy_(blocked("bf16", r["prev"], dev))
    check(L.ay_slice_accumulate_bf16(ptr(doutb), ptr(dsrc.t), P.BATCH, csrc, P.SLICE_CTOTAL, c0, h, w, up, acc, _lib.stream_ptr()), "slice_accumulate")
    got = unblocked("bf16", dsrc.t, csrc)
    assert dsrc.intact(), "stores outside the destination"
    assert torch.equal(doutb, kept), "the source changed"
    R.assert_same_numbers(got, r["out"], f"slice_accumulate {ids(case)}")


def test_accumulate_exact_ragged(dev):
    """a unit count that is no multiple of the 256 units of a workgroup"""
    L = _lib.lib()
    a, b, _, want = P.accumulate_small()
    dst = Guarded((P.ACC_SMALL,), "bf16", dev)
    dst.t.copy_(a.to(dev))
    src = b.to(dev).to(torch.bfloat16)
    kept = src.clone()
    check(L.ay_accumulate_bf16(ptr(dst.t), ptr(src), P.ACC_SMALL, _lib.stream_ptr()), "accumulate")
    got = dst.t.float().cpu()
    assert dst.intact(), "stores outside the destination"
    assert torch.equal(src, kept), "the source changed"
    R.assert_same_numbers(got, want, "accumulate, ragged")


def test_accumulate_exact_second_pass(dev):
    """65535 * 256 + 1000 units: the launch is capped at 65535 workgroups, so the last 1000 units belong to the grid-stride loop's
    second pass.  Operands and reference are one pattern of ACC_PERIOD elements tiled over the tensor; every element is compared on the
    device, and the first and last 2^20 elements and a strided sample once more on the CPU."""
    L = _lib.lib()
    n, period = P.ACC_LARGE, P.ACC_PERIOD
    a, b, _, want = P.accumulate_pattern()
    reps = -(-n // period)
    tiled = lambda t: t.to(dev).to(torch.bfloat16).repeat(reps)[:n]
    dst = Guarded((n,), "bf16", dev)
    dst.t.copy_(tiled(a))
    src = tiled(b)
    check(L.ay_accumulate_bf16(ptr(dst.t), ptr(src), n, _lib.stream_ptr()), "accumulate")
    torch.cuda.synchronize()
    assert dst.intact(), "stores outside the destination"
    bad = dst.t != tiled(want)
    if bool(bad.any()):
        first = int(bad.nonzero()[0])
        raise AssertionError(f"accumulate, second pass: {int(bad.sum())} of {n} values differ; first at element {first} (unit {first // 8}): "
                             f"got {float(dst.t[first])!r}, want {float(want[first % period])!r}")
    assert not bool(torch.isnan(dst.t).any())
    edge = 1 << 20
    for name, index in (("first", torch.arange(0, edge)), ("last", torch.arange(n - edge, n)), ("strided", torch.arange(0, n, 4099))):
        R.assert_same_numbers(dst.t[index.to(dev)].float().cpu(), want[index % period], f"accumulate, second pass, {name} elements")


@pytest.mark.parametrize("case", P.ZERO_INSERT_CASES, ids=ids)
def test_zero_insert_exact(dev, case):
    """the input at the even positions, exact zeros everywhere else, for an output of 2h x 2w, 2h-1 x 2w-1 and a larger one"""
    h, w, ho, wo = case
    L = _lib.lib()
    x, want = P.zero_insert_reference(case)
    B, Cc = x.shape[:2]
    xb = blocked("bf16", x, dev)
    kept = xb.clone()
    out = Guarded((B, Cc // 16, ho, wo, 16), "bf16", dev)
    check(L.ay_zero_insert_bf16(ptr(xb), ptr(out.t), B, Cc, h, w, ho, wo, _lib.stream_ptr()), "zero_insert")
    got = unblocked("bf16", out.t, Cc)
    assert out.intact(), "stores outside the output"
    assert torch.equal(xb, kept), "the source changed"
    R.assert_same_numbers(got, want, f"zero_insert {ids(case)}")
