"""Exact references for the gradient plumbing of the bf16 training step (TEST INFRASTRUCTURE ONLY -- never imported by the product):
ay_accumulate_bf16, ay_slice_accumulate_bf16 and ay_zero_insert_bf16 (csrc/ay_train_bf16.hip), and the case lists that
tests/test_grad_plumbing_cpu.py and tests/test_gpu_grad_plumbing_exact.py share.

The kernels' contract (source comment): fp32 adds, ONE rounding to bfloat16 (nearest even).  Operands here are integers in
[-255, 255], exact in bfloat16.  The sum of an accumulated value and the four children of an upsampled pixel is an integer of at most
11 bits: exact in fp32 in ANY order of the adds, so the float64 sum rounded once is the value the kernel must store, bit for bit.
An 11-bit integer does not fit bfloat16's 8 bits, so that one rounding is exercised (ties counted per case)."""
import functools

import torch

from conv_exact_reference import gen, ints, round_store, rounding_stats, to_f32_exact

RANGE = 255
OUTSIDE = 16384.0     # channels of dout outside the slice: a wrong plane offset moves a sum far away (exact in bfloat16)
BATCH = 3

# up, accumulate, c0, csrc, h, w (of dout; ctotal = 64): the route backward (up = 0: a channel slice) and the upsample backward
# (up = 1: the four children of a pixel), onto nothing and onto a gradient already there, on a rectangle and a square
SLICE_CTOTAL = 64
SLICE_CASES = [(up, acc, c0, csrc, h, w) for (h, w) in ((26, 10), (8, 8)) for up in (0, 1) for acc in (0, 1) for c0 in (0, 16, 32) for csrc in (16, 32)]

# elements of ay_accumulate_bf16 (8 per unit, 256 units per workgroup): a ragged last workgroup; and one unit count beyond the
# 65535 workgroups the launch is capped at, so that the grid-stride loop makes a second pass (268 MB per operand)
ACC_SMALL = 8 * (3 * 256 + 77)
ACC_LARGE = 8 * (65535 * 256 + 1000)
ACC_PERIOD = 32771    # elements of the pattern the large case tiles (a prime: the pattern drifts against units and workgroups)

# h, w, ho, wo of ay_zero_insert_bf16 (ho >= 2h - 1, wo >= 2w - 1): B = 2, 32 channels
ZERO_INSERT_CASES = [(13, 5, 26, 10), (13, 5, 25, 9), (13, 5, 29, 11)]


def once(sum64):
    """the float64 sum -> (its fp32 value, asserted exact; that value rounded once to bfloat16)"""
    o = to_f32_exact(sum64, "sum")
    return o, round_store(o, "bf16")


def children(t, up):
    """[B, C, H, W] -> list of the (1 << up)^2 child planes [B, C, H >> up, W >> up], row-major as the kernel walks them"""
    if not up:
        return [t]
    return [t[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)]


@functools.lru_cache(maxsize=None)
def slice_reference(case):
    """-> dict(dout, prev (None without accumulate), terms, o, out, ties): out[b][c][y][x] = bf16(prev + sum of the children of
    dout[b][c0 + c]); channels of dout outside [c0, c0 + csrc) hold OUTSIDE"""
    up, acc, c0, csrc, h, w = case
    g = gen(up, acc, c0, csrc, h, w, 61)
    dout = torch.full((BATCH, SLICE_CTOTAL, h, w), OUTSIDE)
    dout[:, c0:c0 + csrc] = ints(g, (BATCH, csrc, h, w), RANGE)
    prev = ints(g, (BATCH, csrc, h >> up, w >> up), RANGE) if acc else None
    terms = ([prev] if acc else []) + children(dout[:, c0:c0 + csrc], up)
    o, out = once(sum(t.double() for t in terms))
    return dict(dout=dout, prev=prev, terms=terms, o=o, out=out, ties=rounding_stats(o, "bf16")[1])


def rounded_every_add(terms):
    """MUTANT: a bfloat16 accumulator -- rounds after every add, in the kernel's order (accumulated value first)"""
    a = terms[0].clone()
    for t in terms[1:]:
        a = round_store(a + t, "bf16")
    return a


def accumulate_reference(a, b):
    """dst += src: the sum of two integers in [-255, 255] (9 bits), rounded once"""
    return once(a.double() + b.double())


@functools.lru_cache(maxsize=None)
def accumulate_pattern():
    """(a, b, o, out) of ACC_PERIOD elements: the large case tiles them"""
    g = gen(ACC_PERIOD, 67)
    a, b = ints(g, (ACC_PERIOD,), RANGE), ints(g, (ACC_PERIOD,), RANGE)
    o, out = accumulate_reference(a, b)
    return a, b, o, out


@functools.lru_cache(maxsize=None)
def zero_insert_reference(case):
    """-> (x, out): out[b][c][2y][2x] = x[b][c][y][x], exact zeros elsewhere"""
    h, w, ho, wo = case
    x = ints(gen(h, w, ho, wo, 79), (2, 32, h, w), RANGE)
    out = torch.zeros(2, 32, ho, wo)
    out[:, :, 0:2 * h:2, 0:2 * w:2] = x
    return x, out


@functools.lru_cache(maxsize=None)
def accumulate_small():
    """(a, b, o, out) of ACC_SMALL elements"""
    g = gen(ACC_SMALL, 73)
    a, b = ints(g, (ACC_SMALL,), RANGE), ints(g, (ACC_SMALL,), RANGE)
    return (a, b) + accumulate_reference(a, b)
