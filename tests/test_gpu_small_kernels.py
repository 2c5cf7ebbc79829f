"""The library's oldest small kernels against tests/small_kernels_reference.py, through the C ABI: ay_yolo_decode (both layouts) and
the fused ay_head_decode_fwd_*, the box math, ay_match_detections, the fp32 train-mode BatchNorm, ay_fold_bn, the layout converters,
ay_concat_upsample_bf16 and the fp32 graph plumbing.

The rule (small_kernels_reference.py, profiles/small_kernels_margins.txt): a kernel whose float32 twin uses only + - * / sqrt min max
and comparisons EQUALS the twin bit for bit; the decode and the BatchNorm are held to float64 under bar = max(4 E, 2^-22) relative to the
class scale, E the twin's own distance from float64.  Every output lies between guard bands in a buffer prefilled with a sentinel: what
the kernel does not own comes back untouched.

`PYTHONPATH=. python tests/test_gpu_small_kernels.py` prints the table E / bar / device of every decode, BatchNorm and GIoU class."""
import ctypes as ct
import functools

import numpy as np
import pytest
import torch

import small_kernels_reference as skr
from amyloid_yolo_paper_amd import _lib, stats
from amyloid_yolo_paper_amd._lib import AyError, ConvDesc, check, ptr
from oracle import boxes_oracle as bo

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
GUARD = 4096            # elements on either side of an output
SENT = -777.25          # float outputs are prefilled with it; no case produces it
SENT16 = 0x5A5A         # 16-bit outputs
ROWS = []               # (case, class, E, device): the margins table


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def _guarded(shape, dev, dtype=torch.float32):
    """(buffer, view of `shape` in its middle), all of it the sentinel"""
    n = int(np.prod(shape))
    buf = torch.empty(n + 2 * GUARD, device=dev, dtype=dtype)
    buf.fill_(SENT16 if dtype == torch.int16 else 77 if dtype == torch.int32 else SENT)
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _guards_ok(buf):
    torch.cuda.synchronize()
    s = buf[0].item()
    n = buf.numel() - 2 * GUARD
    assert bool((buf[:GUARD] == s).all()) and bool((buf[GUARD + n:] == s).all()), "guard band overwritten"


def _p(out, buf):
    """pointer of an output view; an empty one points into its buffer (never NULL)"""
    return ptr(out) if out.numel() else ptr(buf[GUARD:])


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_bits(got, want, what=""):
    """bit equality; NaN equals NaN of any payload"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = _bits(got) != _bits(want)
    if got.dtype.kind == "f":
        bad &= ~(np.isnan(got) & np.isnan(want))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])


def _record(case, cls, E, device):
    """one line of the margins table; the assertion of the bar"""
    ROWS.append((case, cls, float(E), float(device)))
    assert device <= skr.bar(E), (case, cls, "E %.3e bar %.3e device %.3e" % (E, skr.bar(E), device))


def _anc(anchors):
    return (ct.c_float * (2 * len(anchors)))(*[float(v) for a in anchors for v in a])


# ================================================================================================ decode
def _decode(L, dev, head, layout, case, anchors=None):
    """ay_yolo_decode into rows [5, 5 + A G G) of a sentinel tensor -> those rows; the other rows and the guards are checked"""
    A, C, G, B, img = case
    K, n_rows = 5 + C, A * G * G
    n_total = n_rows + skr.ROW_EXTRA
    hd = _up(skr.blocked_head(head) if layout else head, dev)
    buf, out = _guarded((B, n_total, K), dev)
    check(L.ay_yolo_decode(ptr(hd), layout, ptr(out), B, A, C, G, img, _anc(anchors or skr.anchors_of(A)), n_total, skr.ROW_OFFSET,
                           _lib.stream_ptr()), "ay_yolo_decode")
    _guards_ok(buf)
    assert bool((out[:, :skr.ROW_OFFSET] == SENT).all()) and bool((out[:, skr.ROW_OFFSET + n_rows:] == SENT).all()), "rows of other heads written"
    return out[:, skr.ROW_OFFSET:skr.ROW_OFFSET + n_rows].cpu().numpy()


def _decode_under_bar(name, got, head, case):
    A, C, G, B, img = case
    anchors = skr.anchors_of(A)
    ref = skr.decode_f64(head, anchors, C, img)
    E = skr.decode_errors(skr.decode_twin(head, anchors, C, img), ref, A, G, img)
    D = skr.decode_errors(got, ref, A, G, img)
    for cls in E:
        _record(name, cls, E[cls], D[cls])


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("case", skr.DECODE_CASES, ids=skr.decode_id)
def test_decode_vs_float64(dev, case, layout):
    """ay_yolo_decode, nchw and blocked heads (NaN in the pad lanes), rows [5, 5 + A G G) of A G G + 7.  Bar: max(4 E, 2^-22) per class
    (xy relative to stride (g + 1), wh and the sigmoids to the value)."""
    head = skr.decode_head(case)
    got = _decode(_lib.lib(), dev, head, layout, case)
    _decode_under_bar("decode L%d %s" % (layout, skr.decode_id(case)), got, head, case)


def _exact_head_operands(case, cin, seed):
    """small-integer activations and filters whose sums are exact in fp32 (and in either 16-bit type): x in -2 .. 2, w in (-2 .. 2) / 8,
    bias in multiples of 1 / 8 -> (x, w, bias, the head they give, exactly)"""
    A, C, G, B, _ = case
    cout = A * (5 + C)
    r = skr.rng(seed)
    xi = r.integers(-2, 3, (B, cin, G, G))
    wi = r.integers(-2, 3, (cout, cin))
    bi = r.integers(-16, 17, cout)
    head = (np.einsum("oc,bchw->bohw", wi, xi) + bi[None, :, None, None]).astype(F64) / 8.0
    assert np.abs(head).max() < 2 ** 10
    return xi.astype(F32), (wi.astype(F32) / 8).reshape(cout, cin, 1, 1), (bi / 8.0).astype(F32), head.astype(F32)


def _fused(L, dev, dtype, case, cin, x, w, bias, num_anchors=None):
    """ay_head_decode_fwd_<dtype> -> (rc, rows [5, 5 + A G G) or the whole sentinel tensor on refusal)"""
    A, C, G, B, img = case
    K, cout = 5 + C, A * (5 + C)
    cpad = (cout + 31) // 32 * 32
    st = _lib.stream_ptr()
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    xd, wd = _up(x, dev), _up(w, dev)
    xb = torch.empty(B, cin // 16, G, G, 16, device=dev, dtype=tdt)
    check(getattr(L, f"ay_nchw_f32_to_blocked_{dtype}")(ptr(xd), ptr(xb), B, cin, G, G, st))
    packed = torch.empty(L.ay_packed_weight_bytes(cpad, cin, 1), device=dev, dtype=torch.uint8)
    check(getattr(L, f"ay_pack_conv_weights_{dtype}")(ptr(wd), ptr(packed), cout, cpad, cin, 1, st))
    sc, sh = torch.zeros(cpad, device=dev), torch.zeros(cpad, device=dev)
    sc[:cout], sh[:cout] = 1.0, _up(bias, dev)
    n_rows = A * G * G
    n_total = n_rows + skr.ROW_EXTRA
    buf, out = _guarded((B, n_total, K), dev)
    d = ConvDesc(B, cin, cout, G, G, G, G, 1, 1, 0, 1, cpad)
    nA = A if num_anchors is None else num_anchors
    rc = getattr(L, f"ay_head_decode_fwd_{dtype}")(ct.byref(d), ptr(xb), ptr(packed), ptr(sc), ptr(sh), nA, C, img,
                                                   _anc(skr.anchors_of(max(A, nA))), ptr(out), n_total, skr.ROW_OFFSET, st)
    _guards_ok(buf)
    if rc != 0:
        return rc, out.cpu().numpy()
    assert bool((out[:, :skr.ROW_OFFSET] == SENT).all()) and bool((out[:, skr.ROW_OFFSET + n_rows:] == SENT).all()), "rows of other heads written"
    return rc, out[:, skr.ROW_OFFSET:skr.ROW_OFFSET + n_rows].cpu().numpy()


@pytest.mark.parametrize("case", skr.DECODE_CASES[:-1], ids=skr.decode_id)
def test_fused_head_decode_on_exact_logits(dev, case):
    """ay_head_decode_fwd_{bf16,f16} where the head value is exact, so the decode alone is under test: (a) zero input, shift = the
    logits; (b) small-integer operands.  Both cin % 64 forms.  Bar: max(4 E, 2^-22) per class against float64; and the bits of
    ay_yolo_decode on the same head."""
    A, C, G, B, img = case
    L = _lib.lib()
    cout = A * (5 + C)
    for cin in (64, 48):
        logits = skr.rng(cin + cout).normal(0, 3, cout).astype(F32)
        zero_x, zero_w = np.zeros((B, cin, G, G), F32), np.zeros((cout, cin, 1, 1), F32)
        head_a = np.broadcast_to(logits[None, :, None, None], (B, cout, G, G)).copy()
        x, w, bias, head_b = _exact_head_operands(case, cin, cin + G)
        for tag, (xx, ww, bb, head) in (("shift", (zero_x, zero_w, logits, head_a)), ("ints", (x, w, bias, head_b))):
            want = _decode(L, dev, head, 0, case)
            for dtype in ("bf16", "f16"):
                rc, got = _fused(L, dev, dtype, case, cin, xx, ww, bb)
                assert rc == 0, L.ay_last_error()
                _same_bits(got, want, (tag, dtype, cin))
                _decode_under_bar("fused %s %s cin%d %s" % (dtype, tag, cin, skr.decode_id(case)), got, head, case)


def test_decode_refusals_leave_the_output_alone(dev):
    """17 anchors (ay_yolo_decode) and 7 (the fused entry points) are refused with AY_ERR_ARG and a message; nothing is written"""
    L = _lib.lib()
    case = (17, 1, 3, 1, 96)
    A, C, G, B, img = case
    head = _up(np.zeros((B, A * 6, G, G), F32), dev)
    buf, out = _guarded((B, A * G * G, 6), dev)
    anc = (ct.c_float * 34)(*([8.0] * 34))
    rc = L.ay_yolo_decode(ptr(head), 0, ptr(out), B, A, C, G, img, anc, A * G * G, 0, _lib.stream_ptr())
    assert rc == -1 and L.ay_last_error()
    _guards_ok(buf)
    assert bool((out == SENT).all())
    case7 = (7, 1, 3, 1, 96)
    for dtype in ("bf16", "f16"):
        rc, whole = _fused(L, dev, dtype, case7, 64, np.zeros((1, 64, 3, 3), F32), np.zeros((42, 64, 1, 1), F32), np.zeros(42, F32))
        assert rc == -1 and b"anchors" in L.ay_last_error() and (whole == F32(SENT)).all()


@functools.lru_cache(maxsize=1)
def _grid_stride_reference():
    case = skr.DECODE_GRID_STRIDE_CASE
    A, C, G, B, img = case
    head = skr.decode_head(case)
    anchors = skr.anchors_of(A)
    ref = skr.decode_f64(head, anchors, C, img)
    E = skr.decode_errors(skr.decode_twin(head, anchors, C, img), ref, A, G, img)
    return head, ref, E


@pytest.mark.parametrize("layout", [0, 1])
def test_decode_grid_stride_pass(dev, layout):
    """16 x 513 x 513 cells: more than the 16384 x 256 threads of a launch, so the last 16 400 cells come from the second pass of the
    grid-stride loop.  Bar: max(4 E, 2^-22) per class against float64."""
    case = skr.DECODE_GRID_STRIDE_CASE
    A, C, G, B, img = case
    assert B * A * G * G > 16384 * 256
    head, ref, E = _grid_stride_reference()
    got = _decode(_lib.lib(), dev, head, layout, case)
    D = skr.decode_errors(got, ref, A, G, img)
    for cls in E:
        _record("decode L%d grid-stride %s" % (layout, skr.decode_id(case)), cls, E[cls], D[cls])


def _assert_extreme(got0, got1, classes, anchors, G, img, bars, who):
    """the assertions of the extreme table: got0 = the decode of the unplanted head, got1 = of the planted one ([1, A G G, K]); classes
    = skr.extreme_classes of the planted (cell, slot, value) entries"""
    mask = np.ones(got0.shape, bool)
    s = float(img) / G
    for cell, k, v, cls, r in classes:
        mask[0, cell, k] = False
        g = float(got1[0, cell, k])
        what = (who, cell, k, v, cls, r, g)
        if cls == "nan":
            assert np.isnan(g), what
        elif k in (2, 3):
            anc = anchors[cell // (G * G)][k - 2]
            if cls == "inf":
                assert g == np.inf, what
            elif cls == "tiny":
                assert 0.0 <= g <= 2 * skr.FLT_MIN * anc, what
            else:
                assert abs(g - r) <= bars["wh"] * r, what
        elif k in (0, 1):
            gc = (cell % G) if k == 0 else (cell // G) % G
            assert gc * s <= g <= (gc + 1) * s and abs(g - (r + gc) * s) <= bars["xy"] * s * (gc + 1), what
        else:
            assert 0.0 <= g <= 1.0, what
            if cls == "one":
                assert abs(g - 1.0) <= bars["sig"], what
            elif cls in ("zero", "tiny"):
                assert g <= 2 * skr.FLT_MIN, what
            else:
                assert abs(g - r) <= bars["sig"] * r, what
    _same_bits(got1[mask], got0[mask], (who, "slots beside a planted logit"))
    assert np.isfinite(got0).all()


@pytest.mark.parametrize("layout", [0, 1])
def test_decode_extreme_logits(dev, layout):
    """ay_yolo_decode: +-0, +-1e-40, +-87, +-88.5, +-89, +-104, +-inf and NaN in every one of the 5 + C slots.  From float64: a w / h
    that rounds to a float32 infinity is +inf; one below FLT_MIN x anchor lies in [0, 2 FLT_MIN anchor]; a sigmoid lies in [0, 1], within
    the bar of 1 or of its value, in [0, 2 FLT_MIN] below FLT_MIN (fp32 has no relative precision there); NaN gives NaN in its slot;
    every other slot has the bits of the unplanted head's decode.  Bar: max(4 E, 2^-22) of the unplanted head, per class.  (The fused
    entry points get the same table in test_fused_head_decode_extreme_logits.)"""
    case = skr.EXTREME_CASE
    A, C, G, B, img = case
    L = _lib.lib()
    anchors = skr.anchors_of(A)
    base, planted, plan = skr.extreme_head()
    got0, got1 = _decode(L, dev, base, layout, case), _decode(L, dev, planted, layout, case)
    ref0 = skr.decode_f64(base, anchors, C, img)
    E = skr.decode_errors(skr.decode_twin(base, anchors, C, img), ref0, A, G, img)
    _assert_extreme(got0, got1, skr.extreme_classes(plan, anchors, img, G), anchors, G, img, {k: skr.bar(v) for k, v in E.items()}, layout)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_fused_head_decode_extreme_logits(dev, dtype):
    """The same table through head_decode_epilogue (ay_head_decode_fwd_{bf16,f16}), which is its own implementation of the decode: zero
    input, shift = the logits, so 0 * w * 1 + shift is exact, +-inf and NaN included.  The logits are per channel, so a run plants ONE
    slot of every anchor (anchor a gets value j + 5 a of the table) and every cell of the grid shows it; 15 x (5 + C) runs put every value
    into every (anchor, slot) channel.  Same assertions and bar as test_decode_extreme_logits; both cin % 64 forms alternate."""
    case = skr.FUSED_EXTREME_CASE
    A, C, G, B, img = case
    K = 5 + C
    L = _lib.lib()
    anchors = skr.anchors_of(A)
    base = skr.rng(91).normal(0, 2, A * K).astype(F32)
    head0 = np.broadcast_to(base[None, :, None, None], (B, A * K, G, G)).copy()
    # the bar of test_decode_extreme_logits: E of the twin on that test's unplanted head (same anchors, same stride 32, 756 random
    # logits; the per-channel logits here are only A K distinct values)
    eA, eC, eG, _, eimg = skr.EXTREME_CASE
    assert anchors == skr.anchors_of(eA) and float(eimg) / eG == float(img) / G
    ebase = skr.extreme_head()[0]
    E = skr.decode_errors(skr.decode_twin(ebase, anchors, eC, eimg), skr.decode_f64(ebase, anchors, eC, eimg), eA, eG, eimg)
    bars = {k: skr.bar(v) for k, v in E.items()}
    got0 = {}
    for cin in (64, 48):
        rc, got0[cin] = _fused(L, dev, dtype, case, cin, np.zeros((B, cin, G, G), F32), np.zeros((A * K, cin, 1, 1), F32), base)
        assert rc == 0, L.ay_last_error()
        _same_bits(got0[cin], _decode(L, dev, head0, 0, case), (dtype, cin, "unplanted"))
    seen = set()
    for j in range(len(skr.EXTREME)):
        for k in range(K):
            cin = 64 if (j + k) % 2 else 48
            logits, plan = skr.fused_extreme_logits(base, A, K, G, j, k)
            rc, got1 = _fused(L, dev, dtype, case, cin, np.zeros((B, cin, G, G), F32), np.zeros((A * K, cin, 1, 1), F32), logits)
            assert rc == 0, L.ay_last_error()
            _assert_extreme(got0[cin], got1, skr.extreme_classes(plan, anchors, img, G), anchors, G, img, bars, (dtype, cin, j, k))
            seen |= {(cell // (G * G), kk, repr(v)) for cell, kk, v in plan}
    assert len(seen) == A * K * len(skr.EXTREME)          # every value in every (anchor, slot) channel


# ================================================================================================ box math
SIZES = (0, 1, 255, 256, 257)


def _subset(n):
    a, b = skr.all_boxes()
    N = len(a)
    idx = (np.arange(n) * max(N // max(n, 1), 1)) % N
    return a[idx], b[idx]


def _iou(L, dev, b1, b2, xyxy, mode):
    n2 = len(b2)
    buf, out = _guarded((n2,), dev)
    d1, d2 = _up(b1 if len(b1) else np.zeros((1, 4), F32), dev), _up(b2 if n2 else np.zeros((1, 4), F32), dev)
    check(L.ay_box_iou(ptr(d1), len(b1), ptr(d2), n2, xyxy, mode, _p(out, buf), _lib.stream_ptr()), "ay_box_iou")
    _guards_ok(buf)
    return out.cpu().numpy()


def _iou_twin(b1, b2, xyxy, mode):
    if len(b2) == 0:
        return np.zeros(0, F32)
    if mode == 0:
        return skr.iou_twin(b1, b2, x1y1x2y2=bool(xyxy))
    if not xyxy:
        b1, b2 = skr.xywh2xyxy_twin(b1), skr.xywh2xyxy_twin(b2)
    return skr.giou_twin(np.broadcast_to(b1, b2.shape) if len(b1) == 1 else b1, b2)


@pytest.mark.parametrize("mode", [0, 1], ids=["iou", "giou"])
@pytest.mark.parametrize("xyxy", [1, 0], ids=["xyxy", "cxcywh"])
def test_box_iou_equals_twin(dev, mode, xyxy):
    """ay_box_iou, every box class (zero size, inverted, touching, disjoint, identical, nested, slide-scale coordinates), elementwise and
    n1 == 1 broadcast, n in {0, 1, 255, 256, 257}, all 600-odd at once, and (corner boxes) one n above 16384 x 256 -- this launch has one
    thread per box and no grid-stride loop, so that n checks the uncapped grid: the twin's bits, no bar."""
    L = _lib.lib()
    a, b = skr.all_boxes()
    for n in SIZES + (len(a),):
        p, q = (a, b) if n == len(a) else _subset(n)
        if not xyxy:
            p, q = skr.to_cxcywh(p), skr.to_cxcywh(q)
        _same_bits(_iou(L, dev, p, q, xyxy, mode), _iou_twin(p, q, xyxy, mode), ("elementwise", n))
        if n:
            _same_bits(_iou(L, dev, p[n // 2:n // 2 + 1], q, xyxy, mode), _iou_twin(p[n // 2:n // 2 + 1], q, xyxy, mode), ("broadcast", n))
    if xyxy:
        n = 16384 * 256 + 257
        p, q = np.resize(a, (n, 4)), np.resize(b[::-1], (n, 4))
        _same_bits(_iou(L, dev, p, q, xyxy, mode), _iou_twin(p, q, xyxy, mode), ("elementwise", n))


def test_giou_margins_and_zero_area_boxes(dev):
    """GIoU per box class: the kernel equals the twin, so its distance from float64 IS E (printed with the bar it would have to meet);
    two zero-area boxes are decided by the 1e-16 terms exactly as the twin decides them."""
    L = _lib.lib()
    for name, (a, b) in skr.box_classes().items():
        got = _iou(L, dev, a, b, 1, 1)
        twin, ref = skr.giou_twin(a, b), skr.giou_f64(a, b)
        _same_bits(got, twin, name)
        _record("giou " + name, "giou", np.abs(twin.astype(F64) - ref).max(), np.abs(got.astype(F64) - ref).max())
    a, b = skr.box_classes()["zero_same_point"]
    assert (_iou(L, dev, a, b, 1, 1) == 0).all()


def _pairwise(L, dev, b1, b2, mode):
    buf, out = _guarded((len(b1), len(b2)), dev)
    d1, d2 = _up(b1 if len(b1) else np.zeros((1, 4), F32), dev), _up(b2 if len(b2) else np.zeros((1, 4), F32), dev)
    check(L.ay_box_iou_pairwise(ptr(d1), len(b1), ptr(d2), len(b2), mode, _p(out, buf), _lib.stream_ptr()), "ay_box_iou_pairwise")
    _guards_ok(buf)
    return out.cpu().numpy()


def _pairwise_twin(b1, b2, mode):
    if not len(b1) or not len(b2):
        return np.zeros((len(b1), len(b2)), F32)
    p, q = np.repeat(b1, len(b2), 0), np.tile(b2, (len(b1), 1))
    return (skr.iou_twin(p, q) if mode == 0 else skr.giou_twin(p, q)).reshape(len(b1), len(b2))


@pytest.mark.parametrize("mode", [0, 1], ids=["iou", "giou"])
def test_box_iou_pairwise_equals_twin(dev, mode):
    """ay_box_iou_pairwise: 2049 x 2049 pairs are one full pass of the 16384 x 256 threads and a tail of 4097; 0 x n, n x 0, 1 x 1,
    257 x 3 beside it.  The twin's bits."""
    L = _lib.lib()
    a, b = skr.all_boxes()
    big1, big2 = np.resize(a, (2049, 4)), np.resize(b[::-1], (2049, 4))
    assert 2049 * 2049 > 16384 * 256
    for b1, b2 in ((big1, big2), (a[:0], b[:5]), (a[:5], b[:0]), (a[:1], b[:1]), (a[100:357], b[300:303])):
        _same_bits(_pairwise(L, dev, b1, b2, mode), _pairwise_twin(b1, b2, mode), (len(b1), len(b2)))


@pytest.mark.parametrize("row_stride", [4, 7, 8])
def test_xywh2xyxy_in_place_equals_twin(dev, row_stride):
    """ay_xywh2xyxy in place on rows of 4, 7 and 8 floats: the first four columns get the twin's bits, the others and the guard bands
    stay; n in {0, 1, 255, 256, 257}, and for row_stride 4 and 7 one n above 16384 x 256 rows (a second grid-stride pass, row
    offsets beyond 2^24 floats)."""
    L = _lib.lib()
    for n in SIZES + ((16384 * 256 + 257,) if row_stride in (4, 7) else ()):
        boxes = skr.to_cxcywh(_subset(n)[0]) if n else np.zeros((0, 4), F32)
        rows = np.full((n, row_stride), SENT, F32)
        rows[:, :4] = boxes
        buf, out = _guarded((n, row_stride), dev)
        if n:
            out.copy_(_up(rows, dev))
        check(L.ay_xywh2xyxy(_p(out, buf), n, row_stride, _lib.stream_ptr()), "ay_xywh2xyxy")
        _guards_ok(buf)
        if n:
            want = rows.copy()
            want[:, :4] = skr.xywh2xyxy_twin(boxes)
            _same_bits(out.cpu().numpy(), want, n)


# ================================================================================================ ay_match_detections
def _match(L, dev, rows, count, targets, thr):
    B, max_det = rows.shape[:2]
    rd, cd = _up(rows, dev), _up(np.asarray(count, np.int32), dev)
    td = _up(targets, dev) if len(targets) else None
    buf, tp = _guarded((B, max_det), dev)
    obuf, ovf = _guarded((1,), dev, torch.int32)
    check(L.ay_match_detections(ptr(rd), ptr(cd), B, max_det, ptr(td), len(targets), ct.c_float(thr), ptr(tp), ptr(ovf), _lib.stream_ptr()),
          "ay_match_detections")
    _guards_ok(buf)
    _guards_ok(obuf)
    return tp.cpu().numpy(), int(ovf.item())


def _through_stats(case):
    B, max_det = case["rows"].shape[:2]
    outs = [torch.from_numpy(case["rows"][b, :int(case["count"][b])].copy()) if 0 < case["count"][b] <= max_det else None for b in range(B)]
    return outs, stats.get_batch_statistics(outs, torch.from_numpy(case["targets"]), case["thr"])


@pytest.mark.parametrize("name", sorted(skr.match_cases()))
def test_match_detections_equals_oracle(dev, name):
    """ay_match_detections on the named edge (no targets / count 0 / count > max_det / absent label / early stop / duplicate targets
    at t, t + 1, t + 64, t + 65 / IoU exactly at and just below the threshold / NaN boxes / sample index >= batch / B = 65): tp flags
    equal to the oracle's get_batch_statistics, 0 beyond count, overflow 0; through the C ABI and through stats.get_batch_statistics."""
    c = skr.match_cases()[name]
    want, _, _ = skr.match_batch(c["rows"], c["count"], c["targets"], c["thr"])
    got, ovf = _match(_lib.lib(), dev, c["rows"], c["count"], c["targets"], c["thr"])
    assert ovf == 0
    _same_bits(got, want, name)
    if (c["count"] <= c["rows"].shape[1]).all():
        outs, metrics = _through_stats(c)
        ref = bo.get_batch_statistics([None if o is None else o.numpy() for o in outs], c["targets"], c["thr"])
        assert len(metrics) == len(ref)
        for m, r in zip(metrics, ref):
            assert np.array_equal(np.asarray(m[0]), r[0])


def test_match_detections_without_targets(dev):
    """n_targets = 0 with a null pointer: every flag 0, overflow 0"""
    c = skr.match_cases()["absent_label"]
    got, ovf = _match(_lib.lib(), dev, c["rows"], c["count"], np.zeros((0, 6), F32), 0.5)
    assert ovf == 0 and not got.any()


@pytest.mark.parametrize("n", [2048, 2049])
def test_match_detections_target_cap(dev, n):
    """2048 targets in one image: overflow 0 and every detection matched; 2049: overflow 1, the first 2048 (in target order) matched as
    the oracle matches them, and AyError from stats.get_batch_statistics."""
    c = skr.cap_case(n)
    want, want_ovf, _ = skr.match_batch(c["rows"], c["count"], c["targets"], c["thr"])
    got, ovf = _match(_lib.lib(), dev, c["rows"], c["count"], c["targets"], c["thr"])
    assert ovf == want_ovf == int(n > 2048) and int(got.sum()) == 2048
    _same_bits(got, want, n)
    if n > 2048:
        with pytest.raises(AyError):
            _through_stats(c)
    else:
        assert int(sum(m[0].sum() for m in _through_stats(c)[1])) == 2048


# ================================================================================================ fp32 BatchNorm
def _bn_fwd(L, dev, z, gamma, beta, rm, rv, mom, leaky):
    B, C, HW = z.shape
    zd, gd, bd = _up(z, dev), _up(gamma, dev), _up(beta, dev)
    ybuf, y = _guarded((B, C, HW), dev)
    sbuf, small = _guarded((4, C), dev)
    small[2].copy_(_up(rm, dev))
    small[3].copy_(_up(rv, dev))
    check(L.ay_bn_train_fwd_f32(ptr(zd), ptr(gd), ptr(bd), ptr(small[2]), ptr(small[3]), ct.c_float(mom), ct.c_float(skr.BN_EPS), leaky,
                                ptr(y), ptr(small[0]), ptr(small[1]), B, C, HW, _lib.stream_ptr()), "ay_bn_train_fwd_f32")
    _guards_ok(ybuf)
    _guards_ok(sbuf)
    s = small.cpu().numpy()
    return dict(y=y.cpu().numpy(), save_mean=s[0], save_invstd=s[1], running_mean=s[2], running_var=s[3])


def _bn_bwd(L, dev, dy, y, z, gamma, mean, invstd, leaky):
    B, C, HW = z.shape
    ins = [_up(v, dev) for v in (dy, y, z, gamma, mean, invstd)]
    zbuf, dz = _guarded((B, C, HW), dev)
    sbuf, small = _guarded((2, C), dev)
    check(L.ay_bn_train_bwd_f32(*[ptr(t) for t in ins], leaky, ptr(dz), ptr(small[0]), ptr(small[1]), B, C, HW, _lib.stream_ptr()),
          "ay_bn_train_bwd_f32")
    _guards_ok(zbuf)
    _guards_ok(sbuf)
    s = small.cpu().numpy()
    return dict(dz=dz.cpu().numpy(), dgamma=s[0], dbeta=s[1])


def _per_channel(name, got, ref, twin, keys, table=True):
    """every quantity, every channel: device <= max(4 E_c, 2^-22) with E_c the twin's error IN THAT CHANNEL; the table gets the channel
    that comes closest to its bar (table=False: asserted, not listed -- y, save_mean and save_invstd do not depend on the momentum)"""
    for k in keys:
        E = skr.channel_errors(twin[k], ref[k], ref["scale"][k])
        D = skr.channel_errors(got[k], ref[k], ref["scale"][k])
        barc = np.maximum(4 * E, skr.FLOOR)
        worst = int(np.argmax(D / barc))
        if table:
            ROWS.append((name, k, float(E[worst]), float(D[worst])))
        assert (D <= barc).all(), (name, k, worst, "E %.3e bar %.3e device %.3e" % (E[worst], barc[worst], D[worst]))


# the zero_y pattern (-a, 0, a, 0) needs n % 4 == 0
BN_PARAMS = [(s, k) for s in skr.BN_SHAPES for k in ("random", "cancel", "const", "zero_y") if k != "zero_y" or (s[0] * s[2]) % 4 == 0]


@pytest.mark.parametrize("shape,kind", BN_PARAMS, ids=lambda v: skr.bn_id(v) if isinstance(v, tuple) else v)
def test_bn_train_f32_vs_float64(dev, shape, kind):
    """ay_bn_train_fwd_f32 / ay_bn_train_bwd_f32 per channel against float64: y, save_mean, save_invstd, both running statistics
    (momentum 0, 0.1, 1; unbiased n / (n - 1), biased at n = 1), dz, dgamma, dbeta; leaky 0 and 1; random channels, channels of mean
    1e4 with standard deviation 1e-2 (save_invstd and running_var relative to the float64 variance), constant channels (invstd =
    1 / sqrt(eps)), and channels with pixels at z == mean, beta = 0 (y == 0: slope 0.1).  Every leaky x momentum pair runs.  Bar:
    max(4 E, 2^-22) per channel and quantity.  On top, y EQUALS ((z - mean) * invstd) * gamma + beta, leaky, formed in float32 from the
    mean and invstd the kernel saved: in the cancel cases the bar on y is wide (the mean's rounding to float32), this equality is not."""
    L = _lib.lib()
    z, gamma, beta, rm, rv, dy = skr.bn_inputs(shape, kind)
    name = "bn %s %s" % (skr.bn_id(shape), kind)
    for leaky in (0, 1):
        for i, mom in enumerate(skr.BN_MOMENTA):
            got = _bn_fwd(L, dev, z, gamma, beta, rm, rv, mom, leaky)
            ref = skr.bn_fwd_f64(z, gamma, beta, rm, rv, mom, skr.BN_EPS, leaky)
            twin = skr.bn_fwd_twin(z, gamma, beta, rm, rv, mom, skr.BN_EPS, leaky)
            _per_channel("%s leaky%d" % (name, leaky), got, ref, twin, ("y", "save_mean", "save_invstd"), table=i == 0)
            _per_channel("%s leaky%d m%g" % (name, leaky, mom), got, ref, twin, ("running_mean", "running_var"))
            _same_bits(got["y"], skr.bn_apply_twin(z, got["save_mean"], got["save_invstd"], gamma, beta, leaky), (name, leaky, mom, "y"))
            if kind == "const":
                assert (got["save_invstd"] == F32(1.0 / np.sqrt(F64(F32(skr.BN_EPS))))).all()
            if kind == "zero_y":
                assert (got["y"][z == 0] == 0).all() and (z == 0).any()
        # backward as a function of ITS inputs: the y, mean and invstd the forward kernel produced
        args = (dy, got["y"], z, gamma, got["save_mean"], got["save_invstd"], leaky)
        gb = _bn_bwd(L, dev, *args)
        _per_channel("%s leaky%d" % (name, leaky), gb, skr.bn_bwd_f64(*args), skr.bn_bwd_twin(*args), ("dz", "dgamma", "dbeta"))


# ================================================================================================ ay_fold_bn
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_fold_bn_equals_twin(dev, n):
    """ay_fold_bn, the three forms (BatchNorm | bias only | neither), n_pad in {n, n rounded up to 32, n + 300} with exact +0 in
    [n, n_pad), var = 0, and eps = 0 with a tiny var: the twin's bits (IEEE division and square root)."""
    L = _lib.lib()
    r = skr.rng(n)
    g, b, m, bias = (r.normal(0, 1, n).astype(F32) for _ in range(4))
    var = np.abs(r.normal(0, 1, n)).astype(F32)
    var[::5] = 0
    tiny = np.full(n, 1e-30, F32) * r.uniform(1, 2, n).astype(F32)
    forms = (("bn", g, b, m, var, None, 1e-5), ("bn eps0", g, b, m, tiny, None, 0.0), ("bias", None, None, None, None, bias, 1e-5),
             ("none", None, None, None, None, None, 1e-5), ("bn+bias", g, b, m, var, bias, 1e-5))
    for n_pad in (n, (n + 31) // 32 * 32, n + 300):
        for tag, gg, bb, mm, vv, bi, eps in forms:
            buf, out = _guarded((2, n_pad), dev)
            ins = [None if v is None else _up(v, dev) for v in (gg, bb, mm, vv, bi)]
            check(L.ay_fold_bn(*[ptr(t) for t in ins], ct.c_float(eps), ptr(out[0]), ptr(out[1]), n, n_pad, _lib.stream_ptr()), "ay_fold_bn")
            _guards_ok(buf)
            o = out.cpu().numpy()
            ws, wt = skr.fold_bn_twin(gg, bb, mm, vv, bi, eps, n, n_pad)
            _same_bits(o[0], ws, (tag, "scale", n_pad))
            _same_bits(o[1], wt, (tag, "shift", n_pad))
            assert not _bits(o[:, n:]).any()          # +0, not -0


# ================================================================================================ layout converters
def _f32_from_bits(u):
    return np.ascontiguousarray(u).view(F32)


def _torch_16(x_f32, dtype):
    """float32 array -> uint16 bits of torch-CPU's conversion (half: with the converter's documented saturation)"""
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    out = torch.from_numpy(np.ascontiguousarray(x_f32)).to(tdt).view(torch.int16).numpy().view(np.uint16)
    return skr.half_bits_device_rule(_bits(x_f32), out) if dtype == "f16" else out


def _to_blocked(L, dev, x, dtype):
    B, C, H, W = x.shape
    CP = (C + 15) // 16
    buf, out = _guarded((B, CP, H, W, 16), dev, torch.int16)
    xd = _up(x, dev)
    check(getattr(L, f"ay_nchw_f32_to_blocked_{dtype}")(ptr(xd), ptr(out), B, C, H, W, _lib.stream_ptr()), "to blocked")
    _guards_ok(buf)
    return out.cpu().numpy().view(np.uint16)


def _check_16(got, x, dtype, what):
    want = skr.to_blocked(_torch_16(x, dtype))
    nan = skr.to_blocked(np.isnan(x))
    is_nan16 = ((got & 0x7FFF) > 0x7F80) if dtype == "bf16" else ((got & 0x7FFF) > 0x7C00)
    assert is_nan16[nan].all(), (what, "a NaN came out as a number")
    bad = (got != want) & ~nan
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), [hex(v) for v in got[bad][:4]], [hex(v) for v in want[bad][:4]])


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_nchw_to_blocked_rounding_sweeps(dev, dtype):
    """ay_nchw_f32_to_blocked_{bf16,f16} over the sweeps of test_small_kernels_cpu.py (every bfloat16 pattern with six low halves; every
    half midpoint and its neighbours, subnormals included), as [1, 16, H, W]: the bits of torch-CPU's round-to-nearest-even (half:
    finite values beyond 65504 saturate, the documented rule); NaN stays NaN."""
    L = _lib.lib()
    for sweep in (skr.bf16_sweep(), skr.f16_sweep()):
        x = _f32_from_bits(sweep).reshape(1, 16, -1, 128)
        _check_16(_to_blocked(L, dev, x, dtype), x, dtype, (dtype, sweep.size))


def _layout_input(shape):
    r = skr.rng(sum(shape))
    x = (r.normal(0, 1, shape) * np.exp2(r.integers(-20, 12, shape))).astype(F32)
    flat = x.reshape(-1)
    flat[::11] = _f32_from_bits(r.integers(1, 0x00800000, flat[::11].size).astype(np.uint32))     # fp32 subnormals
    flat[3::13] *= F32(2.0 ** -120)
    return x


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", skr.LAYOUT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layout_round_trip_shapes(dev, shape, dtype):
    """rectangular images, C % 16 != 0: nchw -> blocked has torch-CPU's bits and exact +0 in the pad lanes (fp32 subnormals and values
    that become 16-bit subnormals included); blocked -> nchw reads them back (the pad lanes of the source hold NaN) for the 16-bit type
    and for blocked f32."""
    L = _lib.lib()
    B, C, H, W = shape
    x = _layout_input(shape)
    got = _to_blocked(L, dev, x, dtype)
    _check_16(got, x, dtype, shape)
    if C % 16:
        assert not got[:, -1, :, :, C % 16:].any(), "pad lanes are not +0"
    # back: 16-bit source with NaN pad lanes
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float16
    src16 = skr.to_blocked(_torch_16(x, dtype), fill=0x7FFF)
    buf, out = _guarded(shape, dev)
    sd = _up(src16.view(np.int16), dev)
    check(getattr(L, f"ay_blocked_{dtype}_to_nchw_f32")(ptr(sd), ptr(out), B, C, H, W, _lib.stream_ptr()))
    _guards_ok(buf)
    _same_bits(out.cpu().numpy(), torch.from_numpy(_torch_16(x, dtype).view(np.int16)).view(tdt).float().numpy(), (shape, dtype, "back"))
    if dtype == "bf16":
        src32 = skr.to_blocked(x, fill=np.nan)
        buf, out = _guarded(shape, dev)
        sd = _up(src32, dev)
        check(L.ay_blocked_f32_to_nchw_f32(ptr(sd), ptr(out), B, C, H, W, _lib.stream_ptr()))
        _guards_ok(buf)
        _same_bits(out.cpu().numpy(), x, (shape, "f32 back"))


def test_blocked_to_nchw_every_pattern(dev):
    """the three blocked -> nchw converters on all 65 536 patterns of each 16-bit type (and 65 536 float32 patterns through the f32
    one): torch-CPU's widening; NaN compared as NaN"""
    L = _lib.lib()
    pat = np.arange(65536, dtype=np.uint16).reshape(1, 16, 64, 64)
    for dtype, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        buf, out = _guarded(pat.shape, dev)
        sd = _up(skr.to_blocked(pat).view(np.int16), dev)
        check(getattr(L, f"ay_blocked_{dtype}_to_nchw_f32")(ptr(sd), ptr(out), 1, 16, 64, 64, _lib.stream_ptr()))
        _guards_ok(buf)
        _same_bits(out.cpu().numpy(), torch.from_numpy(pat.view(np.int16)).view(tdt).float().numpy(), dtype)
    p32 = ((pat.astype(np.uint32) << 16) | skr.rng(9).integers(0, 65536, pat.shape).astype(np.uint32))
    keep = ~skr.is_nan32(p32)                                   # a copy keeps every bit; NaN payloads are left out of the comparison
    buf, out = _guarded(pat.shape, dev)
    sd = _up(skr.to_blocked(p32).view(np.int32), dev)
    check(L.ay_blocked_f32_to_nchw_f32(ptr(sd), ptr(out), 1, 16, 64, 64, _lib.stream_ptr()))
    _guards_ok(buf)
    got = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[keep], p32[keep]) and skr.is_nan32(got[~keep]).all()


def test_layout_converters_grid_stride(dev):
    """one element count above the 65536 x 256 threads of a launch in each direction (the tail comes from the second grid-stride pass):
    [1, 17, 513, 1024] to blocked (both types), [1, 33, 500, 1024] from blocked (bf16, f16, f32)"""
    L = _lib.lib()
    st = _lib.stream_ptr()
    shape = (1, 17, 513, 1024)
    assert 32 * 513 * 1024 > 65536 * 256
    x = skr.rng(1).normal(0, 1, shape).astype(F32)
    for dtype in ("bf16", "f16"):
        _check_16(_to_blocked(L, dev, x, dtype), x, dtype, ("grid-stride", dtype))
    shape = (1, 33, 500, 1024)
    assert 33 * 500 * 1024 > 65536 * 256
    x = skr.rng(2).normal(0, 1, shape).astype(F32)
    for dtype, tdt in (("bf16", torch.bfloat16), ("f16", torch.float16), ("f32", None)):
        if tdt is None:
            src, want = skr.to_blocked(x, fill=np.nan), x
        else:
            b16 = _torch_16(x, dtype)
            src, want = skr.to_blocked(b16, fill=0x7FFF).view(np.int16), torch.from_numpy(b16.view(np.int16)).view(tdt).float().numpy()
        buf, out = _guarded(shape, dev)
        sd = _up(src, dev)
        check(getattr(L, f"ay_blocked_{dtype}_to_nchw_f32")(ptr(sd), ptr(out), *shape, st))
        _guards_ok(buf)
        wd = _up(want, dev)
        assert torch.equal(out.view(torch.int32), wd.view(torch.int32)), dtype


@pytest.mark.parametrize("up1", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("c1c2", [(32, 48), (16, 0), (64, 16)], ids=lambda c: "c%d+%d" % c)
def test_concat_upsample_is_a_pure_copy(dev, c1c2, B, up1):
    """ay_concat_upsample_bf16 moves 16-bit elements untouched: random 16-bit patterns (half patterns and NaN payloads among them)
    compared as int16, a 6 x 10 output, up1 0 and 1, c2 = 0 with a null src2"""
    L = _lib.lib()
    c1, c2 = c1c2
    H, W = 6, 10
    r = skr.rng(c1 + c2 + B + up1)
    s1 = r.integers(0, 65536, (B, c1 // 16, H >> up1, W >> up1, 16)).astype(np.uint16)
    s2 = r.integers(0, 65536, (B, c2 // 16, H, W, 16)).astype(np.uint16) if c2 else None
    s1[0, 0, 0, 0, :4] = [0x7FC1, 0xFF81, 0x7C01, 0xFE00]     # NaN payloads of either type
    buf, out = _guarded((B, (c1 + c2) // 16, H, W, 16), dev, torch.int16)
    d1 = _up(s1.view(np.int16), dev)
    d2 = _up(s2.view(np.int16), dev) if c2 else None
    check(L.ay_concat_upsample_bf16(ptr(d1), c1, up1, ptr(d2), c2, ptr(out), B, H, W, _lib.stream_ptr()), "ay_concat_upsample_bf16")
    _guards_ok(buf)
    assert np.array_equal(out.cpu().numpy().view(np.uint16), skr.concat_upsample_twin(s1, up1, s2))


# ================================================================================================ fp32 plumbing
@pytest.mark.parametrize("c0", [0, 3])
@pytest.mark.parametrize("up", [0, 1])
def test_copy_channels_and_slice_accumulate_f32(dev, up, c0):
    """ay_copy_channels_f32 / ay_slice_accumulate_f32: B = 3, 4 of 9 channels at c0 = 0 and mid, a 5 x 7 (up 0) or 6 x 10 (up 1) image
    (a ragged last block), the other channels untouched; the accumulate onto a non-zero destination, twice.  NumPy's bits."""
    L = _lib.lib()
    st = _lib.stream_ptr()
    B, csrc, ctotal = 3, 4, 9
    H, W = (6, 10) if up else (5, 7)
    r = skr.rng(10 * up + c0)
    src = r.normal(0, 1, (B, csrc, H >> up, W >> up)).astype(F32)
    buf, out = _guarded((B, ctotal, H, W), dev)
    sd = _up(src, dev)
    check(L.ay_copy_channels_f32(ptr(sd), ptr(out), B, csrc, ctotal, c0, H, W, up, st), "ay_copy_channels_f32")
    _guards_ok(buf)
    _same_bits(out.cpu().numpy(), skr.copy_channels_twin(src, np.full((B, ctotal, H, W), SENT, F32), c0, up), "copy")
    dout = r.normal(0, 1, (B, ctotal, H, W)).astype(F32)
    acc0 = r.normal(0, 1, src.shape).astype(F32)
    buf, acc = _guarded(src.shape, dev)
    acc.copy_(_up(acc0, dev))
    dd = _up(dout, dev)
    want = acc0
    for _ in range(2):
        check(L.ay_slice_accumulate_f32(ptr(dd), ptr(acc), B, csrc, ctotal, c0, H, W, up, st), "ay_slice_accumulate_f32")
        want = skr.slice_accumulate_twin(dout, want, c0, up)
    _guards_ok(buf)
    _same_bits(acc.cpu().numpy(), want, "accumulate twice")


def test_add_and_accumulate_f32(dev):
    """ay_add_f32 / ay_accumulate_f32 at n in {0, 1, 1000} and one n above the launch's 32768 x 256 threads: NumPy's bits, guards intact"""
    L = _lib.lib()
    st = _lib.stream_ptr()
    for n in (0, 1, 1000, 32768 * 256 + 1001):
        r = skr.rng(n % 1000)
        a, b = r.normal(0, 1, max(n, 1)).astype(F32), r.normal(0, 1, max(n, 1)).astype(F32)
        ad, bd = _up(a, dev), _up(b, dev)
        buf, out = _guarded((n,), dev)
        check(L.ay_add_f32(ptr(ad), ptr(bd), _p(out, buf), n, st), "ay_add_f32")
        _guards_ok(buf)
        buf2, acc = _guarded((n,), dev)
        if n:
            acc.copy_(ad[:n])
        check(L.ay_accumulate_f32(_p(acc, buf2), ptr(bd), n, st), "ay_accumulate_f32")
        _guards_ok(buf2)
        if n:
            want = _up(a[:n] + b[:n], dev).view(torch.int32)
            assert torch.equal(out.view(torch.int32), want) and torch.equal(acc.view(torch.int32), want), n


# ================================================================================================ the margins table
def _print_margins():
    d = torch.device("cuda", 0)
    for case in skr.DECODE_CASES:
        for layout in (0, 1):
            test_decode_vs_float64(d, case, layout)
    for case in skr.DECODE_CASES[:-1]:
        test_fused_head_decode_on_exact_logits(d, case)
    for layout in (0, 1):
        test_decode_grid_stride_pass(d, layout)
    test_giou_margins_and_zero_area_boxes(d)
    for shape, kind in BN_PARAMS:
        test_bn_train_f32_vs_float64(d, shape, kind)
    w = max(len(r[0]) for r in ROWS)
    print("%-*s %-13s %-28s %-21s %s" % (w, "case", "class", "E (float32 twin vs float64)", "bar = max(4 E, 2^-22)", "device vs float64"))
    for case, cls, E, D in ROWS:
        print("%-*s %-13s E %9.2e  bar %9.2e  device %9.2e%s" % (w, case, cls, E, skr.bar(E), D, "" if D <= skr.bar(E) else "   OUTSIDE"))


if __name__ == "__main__":
    _print_margins()
