"""CPU (no GPU needed): the conditions the exact tests of the gradient plumbing rest on, asserted on the REFERENCE of every case
tests/test_gpu_grad_plumbing_exact.py runs (tests/plumbing_reference.py, module docstring):

  * operands are exact in bfloat16, every sum is exact in fp32 (`once` asserts it) and an fp32 sum in the reversed order gives the
    same bits: one reference serves any order of the adds;
  * up = 1 (five or four terms, up to 11 bits): at least 100 exact ties per case, and a bfloat16 accumulator -- the mutant that
    rounds after every add -- differs from the reference in at least 100 values, with and without an accumulated value;
  * up = 0 has two terms at most, so "rounds after every add" IS the reference there and a tie count would mean nothing.  The
    mutants to separate are "accumulate ignored" and "wrong c0": each differs from the reference almost everywhere (>= 90 %);
  * ay_accumulate_bf16: ties in both cases, and "dst unchanged" / "dst = src" differ from the reference almost everywhere."""
import pytest
import torch

import plumbing_reference as P
from conv_exact_reference import MIN_TIES, round_store

ids = lambda c: "x".join(str(int(v)) for v in c)
MIN_DIFFER = 100


def exact_in_bf16(*ts):
    return all(torch.equal(t, t.to(torch.bfloat16).float()) for t in ts if t is not None)


@pytest.mark.parametrize("case", P.SLICE_CASES, ids=ids)
def test_slice_accumulate_reference(case):
    up, acc, c0, csrc, h, w = case
    r = P.slice_reference(case)
    assert exact_in_bf16(r["dout"], r["prev"])
    back = sum(t for t in reversed(r["terms"]))          # fp32, the other order
    assert torch.equal(back, r["o"])
    assert float(r["o"].abs().max()) < 2 ** 11
    n = r["out"].numel()
    if up:
        assert r["ties"] >= MIN_TIES, r["ties"]
        assert int((P.rounded_every_add(r["terms"]) != r["out"]).sum()) >= MIN_DIFFER
    else:
        # two terms at most: the mutants that matter ignore the accumulated value or read another slice
        if acc:
            ignored = round_store(r["dout"][:, c0:c0 + csrc], "bf16")
            assert int((ignored != r["out"]).sum()) >= 0.9 * n
        other = c0 + 16 if c0 + 16 + csrc <= P.SLICE_CTOTAL else c0 - 16
        wrong = r["dout"][:, other:other + csrc] + (r["prev"] if acc else 0.0)
        assert int((round_store(wrong, "bf16") != r["out"]).sum()) >= 0.9 * n
    # a wrong plane offset under up = 1 as well: every sum that takes a plane outside the slice is off by OUTSIDE or more
    assert float(r["o"].abs().max()) < P.OUTSIDE / 4


def test_accumulate_reference():
    for a_, b_, o, out in (P.accumulate_small(), P.accumulate_pattern()):
        assert exact_in_bf16(a_, b_)
        assert torch.equal(b_ + a_, o)
        assert P.rounding_stats(o, "bf16")[1] >= MIN_TIES
        n = out.numel()
        assert int((a_ != out).sum()) >= 0.9 * n and int((b_ != out).sum()) >= 0.9 * n
    assert P.ACC_SMALL % 8 == 0 and (P.ACC_SMALL // 8) % 256 != 0
    assert P.ACC_LARGE // 8 > 65535 * 256            # beyond one pass of the capped grid
    assert P.ACC_LARGE % P.ACC_PERIOD != 0 and P.ACC_PERIOD % 8 != 0


@pytest.mark.parametrize("case", P.ZERO_INSERT_CASES, ids=ids)
def test_zero_insert_reference(case):
    h, w, ho, wo = case
    assert ho >= 2 * h - 1 and wo >= 2 * w - 1
    x, out = P.zero_insert_reference(case)
    assert exact_in_bf16(x) and out.shape[2:] == (ho, wo)
    assert torch.equal(out[:, :, 0:2 * h:2, 0:2 * w:2], x)
    assert float(out.abs().sum()) == float(x.abs().sum())      # nothing anywhere else
