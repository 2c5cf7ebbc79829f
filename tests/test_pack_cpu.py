"""CPU: tests/pack_reference.py (the packed-filter layouts the GPU packers are held to) against the properties include/amyloid_yolo.h
documents -- image sizes, every filter value exactly once, +0 in every padding position, and the tap table of the stride-2 parity
classes.  Filters hold distinct integers that bf16 (8-bit significand) and half store exactly."""
import numpy as np
import pytest

import pack_reference as P


def _distinct(cout, cin, k):
    """OIHW filter of distinct non-zero integers that an 8-bit significand holds exactly (1 .. 256, then every 2nd, 4th, ...), both
    signs, in a scrambled order"""
    n = cout * cin * k * k
    exact = np.array([v for v in range(1, 1 << 15) if v % (1 << max(0, v.bit_length() - 8)) == 0], np.float32)
    v = np.concatenate([exact, -exact])
    assert n <= v.size
    return np.random.default_rng(n).permutation(v[np.argsort(np.abs(v), kind="stable")][:n]).reshape(cout, cin, k, k)


def _check_holds_filter_once(img, w, dtype="bf16"):
    b = P.bits(img, dtype)
    v = P.values(b, dtype)
    assert np.array_equal(np.sort(v[v != 0]), np.sort(w.reshape(-1))), "every filter value exactly once, nothing else"
    assert not b[v == 0].any(), "padding is +0"
    return b


# (cout, cout_pad, cin, k): padded and unpadded output channels, one and two input chunks, k = 1 and 3
@pytest.mark.parametrize("spec", [(12, 16, 16, 3), (5, 32, 32, 1), (16, 16, 32, 1), (3, 16, 16, 3)], ids=str)
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_forward_image(spec, dtype):
    cout, cout_pad, cin, k = spec
    w = _distinct(cout, cin, k)
    img = P.forward_image(w, cout_pad)
    assert img.shape == (cin // 16, k * k, 2, cout_pad, 8)
    b = _check_holds_filter_once(img, w, dtype)
    assert b.nbytes == (cin // 16) * k * k * 2 * cout_pad * 8 * 2
    for co, ci, kh, kw in [(0, 0, 0, 0), (cout - 1, cin - 1, k - 1, k - 1), (cout // 2, 9, k // 2, 0)]:
        assert img[ci // 16, kh * k + kw, (ci % 16) // 8, co, ci % 8] == w[co, ci, kh, kw]
    assert not img[:, :, :, cout:].any()


# (cout, cin, cin_pad, k): ragged cout chunk, padded input channels, cin_pad beyond ceil16(cin)
@pytest.mark.parametrize("spec", [(10, 5, 32, 3), (24, 20, 32, 1), (17, 3, 64, 3), (16, 32, 32, 1)], ids=str)
def test_dgrad_image(spec):
    cout, cin, cin_pad, k = spec
    w = _distinct(cout, cin, k)
    img = P.dgrad_image(w, cin_pad)
    chunks = (cout + 15) // 16
    assert img.shape == (chunks, k * k, 2, cin_pad, 8)
    b = _check_holds_filter_once(img, w)
    assert b.nbytes == chunks * k * k * 2 * cin_pad * 8 * 2
    for co, ci, kh, kw in [(0, 0, 0, 0), (cout - 1, cin - 1, k - 1, 0), (cout // 2, cin // 2, k // 2, k - 1)]:
        # W'[ci][co][kh][kw] = W[co][ci][k-1-kh][k-1-kw]
        assert img[co // 16, kh * k + kw, (co % 16) // 8, ci, co % 8] == w[co, ci, k - 1 - kh, k - 1 - kw]
    assert not img[:, :, :, cin:].any()


# (cout, cout_pad, cin, cin_pad)
@pytest.mark.parametrize("spec", [(6, 16, 5, 32), (11, 32, 4, 32), (16, 16, 3, 64)], ids=str)
def test_dgrad_s2_images(spec):
    cout, cout_pad, cin, cin_pad = spec
    w = _distinct(cout, cin, 3)
    img = P.dgrad_s2_images(w, cout_pad, cin_pad)
    assert img.shape == (4, cout_pad // 16, 4, 2, cin_pad, 8)
    b = _check_holds_filter_once(img, w)     # the four classes together hold each of the 9 taps of every (co, ci) exactly once
    assert b.nbytes == 4 * (cout_pad // 16) * 4 * 2 * cin_pad * 8 * 2
    empty = [(cls, tap) for cls in range(4) for tap in range(4) if not img[cls, :, tap].any()]
    assert len(empty) == 7 and (0, 0) not in empty, empty
    # class (py, px), window (oy, ox) -> filter tap: py = 0: oy 0 -> kh 1, oy 1 -> none; py = 1: oy 0 -> kh 2, oy 1 -> kh 0; columns alike
    co, ci = cout - 1, cin - 1
    at = lambda cls, tap: img[cls, co // 16, tap, (co % 16) // 8, ci, co % 8]  # noqa: E731
    assert at(0, 0) == w[co, ci, 1, 1]
    assert at(1, 0) == w[co, ci, 1, 2] and at(1, 1) == w[co, ci, 1, 0]
    assert at(2, 0) == w[co, ci, 2, 1] and at(2, 2) == w[co, ci, 0, 1]
    assert [at(3, t) for t in range(4)] == [w[co, ci, 2, 2], w[co, ci, 2, 0], w[co, ci, 0, 2], w[co, ci, 0, 0]]


def test_rounding_is_nearest_even():
    """bits(): ties go to the even 16-bit neighbour, in both storage types"""
    x = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11], np.float32)
    assert list(P.values(P.bits(x, "bf16"), "bf16")[:2]) == [1.0, 1 + 2.0 ** -6]
    assert list(P.values(P.bits(x, "f16"), "f16")[2:]) == [1.0, 1 + 2.0 ** -9]
