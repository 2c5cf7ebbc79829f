"""CPU (no GPU needed): the conditions tests/test_gpu_streams.py rests on, asserted on the REFERENCE of every base case, both
periods and both storage types (tests/streams_reference.py, module docstring):

  * conv_reference found its rounding condition: at least 100 exact ties, LeakyReLU cases at least 25 % of the values not
    representable before the rounding (its own assertion, as in tests/test_conv_exact_cpu.py);
  * headroom: no output needs more than 2^20 grid units of sum |a_i| |b_i|;
  * images tell apart in every tile: for every pair of distinct base images and every output tile of the kernel's tile size at
    least 90 % of the tile's values differ (measured here: 96.9 % at the least, ring3x3s2 with P = 7; the other four cases 98.2 % or more);
  * the blocked reference tensors hold the reference's numbers exactly, and the periodic batch is image i = base[i % P].

`PYTHONPATH=. python tests/test_streams_cpu.py` prints the per-case table."""
import pytest
import torch

import conv_exact_reference as R
import streams_reference as SR

CASES = [(name, P) for name in SR.BASE_CASES for P in SR.PERIODS]


@pytest.mark.parametrize("store", ["bf16", "f16"])
@pytest.mark.parametrize("name,P", CASES, ids=lambda v: str(v))
def test_periodic_reference(name, P, store):
    leaky = SR.BASE_CASES[name][1][6]
    r = SR.reference(name, P, store)
    assert r["x"].shape[0] == P and r["out"].shape[0] == P
    assert r["ties"] >= R.MIN_TIES, r["ties"]
    if leaky:
        assert r["inexact"] >= R.MIN_INEXACT_LEAKY, r["inexact"]
    assert r["bits"] <= R.HEADROOM_BITS, r["bits"]
    share = SR.min_tile_difference(r["out"], SR.tile_rows(name))
    print(f"{name} P={P} {store}: ties {r['ties']}, inexact {r['inexact']:.3f}, bits {r['bits']:.1f}, least tile difference {share:.4f}")
    assert share >= SR.MIN_TILE_DIFFERENCE, share


def test_the_two_operand_sets_differ():
    """B = P is part of the generator's key: filters, images and affine differ between the operands of the two streams"""
    for name in SR.BASE_CASES:
        a, b = (SR.reference(name, P, "bf16") for P in SR.PERIODS)
        assert not torch.equal(a["w"], b["w"])
        assert not torch.equal(a["x"][:5], b["x"][:5])


def test_blocked_layout_and_periodic_batch():
    """blocked_cpu: channel c of pixel (y, x) at [c // 16][y][x][c % 16], padded channels zero; periodic: image i = base[i % P]"""
    g = R.gen(3, 1, 4)
    t = R.ints(g, (3, 20, 5, 7), 4)
    b = SR.blocked_cpu(t, "bf16", 32)
    assert b.shape == (3, 2, 5, 7, 16) and b.dtype == torch.bfloat16
    for (i, c, y, x) in ((0, 0, 0, 0), (2, 19, 4, 6), (1, 16, 2, 3), (1, 15, 0, 6)):
        assert float(b[i, c // 16, y, x, c % 16]) == float(t[i, c, y, x])
    assert not bool(b[:, 1, :, :, 4:].any())
    p = SR.periodic(b, 8)
    assert p.shape[0] == 8 and all(torch.equal(p[i], b[i % 3]) for i in range(8))


def test_counter_condition():
    """more than half of the items from the counter: n - D * workgroups > n // 2"""
    assert SR.counter_deals_most(2048, 256, 3) and not SR.counter_deals_most(2048, 256, 5)
    assert SR.counter_deals_most(2561, 256, 5) and not SR.counter_deals_most(2560, 256, 5)


if __name__ == "__main__":
    for name_, P_ in CASES:
        for store_ in ("bf16", "f16"):
            test_periodic_reference(name_, P_, store_)
