"""Traversal direction of the persistent convolution launches (ConvArgs::reverse, ItemRange::item_of): a launch that walks each
XCD's item range from the top down computes the same items as one that walks it upward, so forward and reversed runs on the same
random operands must give the same BITS (torch.equal on the raw 16-bit / fp32 outputs) -- the only bar in this file.  What can go
wrong is an id used unmapped somewhere (the look-ahead DMA of the next item's first stage, the stem's tile ring two items ahead, the
fused block's loader across item boundaries): a tile is then computed from another tile's input, or not at all.  Outputs start
as NaNs, so a tile that no workgroup wrote shows as well.

Item-count conditions, derived from the launch geometry (8 XCDs x min(items per XCD, CUs per XCD) workgroups, ay_conv_common.h):
  dyn     every workgroup the launch can start has at least 8 items: past the statically dealt ones (3 or 5) into the counter
  uneven  the item count is no multiple of 8: the last XCD's range is shorter than the others
  few     fewer items than workgroups: some workgroups of the last XCD have nothing to do
Shapes: the smallest each entry point takes -- the 16x16x32 kernel needs cin % 32 == 0 (cin = 16 runs through ay_conv_fwd, which
gives it the 32x32x16 ring kernel on the same 16x32 tile), the 1x1 ring kernel cin % 64 == 0 (64 -> 32; a 32 -> 32 layer and the
head + decode are one-workgroup-per-item launches, which take their grid from the far end when reversed: run here as well)."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_cases as gc
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ConvDesc, check, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def _cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus - cus % 8


def _canvas_items(B, ho, wo, th, tw, in_bytes, out_bytes, s1_same):
    """tiles of the batch as the launcher cuts them (canvas_plan in ay_conv_bf16.hip): image by image, or on a canvas if that
    saves a tenth of the tiles"""
    per_image = B * -(-ho // th) * -(-wo // tw)
    if B < 2 or not s1_same or in_bytes >= 1 << 31 or out_bytes >= 1 << 31:
        return per_image
    best = per_image
    for gx in range(1, min(B, 64) + 1):
        rows = -(-B // gx)
        best = min(best, -(-gx * (wo + 1) // tw) * -(-rows * (ho + 1) // th))
    return best if best * 10 <= per_image * 9 else per_image


def _pick_batch(cond, items_of):
    """smallest batch that meets the item-count condition `cond`; items_of(B) -> items of the launch"""
    slots = _cus() // 8
    for B in range(1, 4096):
        n = items_of(B)
        wgs = 8 * min(-(-n // 8), slots)
        if cond == "dyn" and n >= 8 * wgs and wgs == 8 * slots:
            return B, n, wgs
        if cond == "uneven" and n % 8 != 0 and n >= 3 * 8 * slots:
            return B, n, wgs
        if cond == "few" and n < wgs:
            return B, n, wgs
    raise AssertionError(f"no batch gives the condition {cond}")


def _both_directions(run, out_shape, dtype, dev):
    """run(out) forward and reversed into NaN-filled outputs -> the two outputs as raw integers"""
    L = _lib.lib()
    outs = []
    try:
        for rev in (0, 1):
            out = torch.full(out_shape, float("nan"), device=dev, dtype=dtype)
            L.ay_conv_set_traversal(rev)
            assert L.ay_conv_get_traversal() == rev
            run(out)
            outs.append(out)
    finally:
        L.ay_conv_set_traversal(0)
    torch.cuda.synchronize()
    fwd, rev = outs
    assert bool(torch.isfinite(fwd.float()).all()), "the forward run left elements unwritten"
    raw = torch.int16 if dtype != torch.float32 else torch.int32
    assert torch.equal(fwd.view(raw), rev.view(raw)), "reversed launch differs from the forward one"


def _operands(dev, cin, cout, k, seed):
    L, st = _lib.lib(), _lib.stream_ptr()
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(cout, cin, k, k, generator=g) / np.sqrt(cin * k * k)).to(dev)
    packed = torch.empty(L.ay_packed_weight_bytes(cout, cin, k), device=dev, dtype=torch.uint8)
    check(L.ay_pack_conv_weights_bf16(ptr(w), ptr(packed), cout, cout, cin, k, st))
    return g, packed, (torch.rand(cout, generator=g) + 0.5).to(dev), (torch.randn(cout, generator=g) * 0.1).to(dev)


def _blocked(g, B, c, h, w, dev):
    """random bf16 activations [B][c/16][h][w][16]; a few distinct images repeated (the generator is on the CPU)"""
    u = torch.randn(min(B, 3), c // 16, h, w, 16, generator=g).to(torch.bfloat16).to(dev)
    return u.repeat(-(-B // u.shape[0]), 1, 1, 1, 1)[:B].contiguous()


# entry, cin, cout, k, stride, H, W, residual, tile rows
CONV_SHAPES = {
    "m16": ("ay_conv3x3_m16_fwd_bf16", 32, 128, 3, 1, 128, 128, False, 16),
    "m16-res": ("ay_conv3x3_m16_fwd_bf16", 32, 128, 3, 1, 128, 128, True, 16),
    "m16-rect": ("ay_conv3x3_m16_fwd_bf16", 32, 128, 3, 1, 48, 160, False, 16),      # 3 x 5 tiles, none of them whole in both directions
    "m16-rect-res": ("ay_conv3x3_m16_fwd_bf16", 32, 128, 3, 1, 48, 160, True, 16),
    "ring3x3-cin16": ("ay_conv_fwd_bf16", 16, 128, 3, 1, 128, 128, True, 16),          # one stage per item
    "ring3x3-cin16-rect": ("ay_conv_fwd_bf16", 16, 128, 3, 1, 48, 160, True, 16),
    "ring1x1": ("ay_conv_fwd_bf16", 64, 32, 1, 1, 24, 40, False, 8),                   # 3 x 2 tiles, the right ones 8 wide
    "ring3x3s2-odd": ("ay_conv_fwd_bf16", 16, 64, 3, 2, 65, 65, False, 8),             # 33 x 33 out
}
CONV_CASES = [("m16", "dyn"), ("m16-res", "dyn"), ("m16-rect", "uneven"), ("m16-rect-res", "uneven"), ("m16-rect", "few"),
              ("m16-rect-res", "few"), ("ring3x3-cin16", "dyn"), ("ring3x3-cin16-rect", "uneven"), ("ring3x3-cin16-rect", "few"), ("ring1x1", "dyn"), ("ring1x1", "uneven"),
              ("ring1x1", "few"), ("ring3x3s2-odd", "dyn"), ("ring3x3s2-odd", "uneven"), ("ring3x3s2-odd", "few")]


@pytest.mark.parametrize("shape,cond", CONV_CASES, ids=lambda v: v)
def test_conv_kernels_forward_equals_reversed(dev, shape, cond):
    entry, cin, cout, k, stride, H, W, has_res, th = CONV_SHAPES[shape]
    L, st = _lib.lib(), _lib.stream_ptr()
    pad = (k - 1) // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    same = (H, W) == ((Ho, Wo) if stride == 1 else (2 * Ho, 2 * Wo))
    canvas = "m16" not in shape   # the 16x16x32 entry point always tiles image by image
    # (every shape here is one channel group: its cout is the width of the tile its kernel uses)
    items_of = lambda B: (_canvas_items(B, Ho, Wo, th, 32, H * W * B * cin * 2, Ho * Wo * B * cout * 2, same) if canvas
                          else B * -(-Ho // th) * -(-Wo // 32))
    B, n_items, wgs = _pick_batch(cond, items_of)
    print(f"{shape} {cond}: batch {B}, {n_items} items, {wgs} workgroups")
    g, packed, sc, sh = _operands(dev, cin, cout, k, cin * 7 + cout + k + H)
    x = _blocked(g, B, cin, H, W, dev)
    res = _blocked(g, B, cout, Ho, Wo, dev) if has_res else None
    d = ConvDesc(B, cin, cout, H, W, Ho, Wo, k, stride, 1, 0, cout)
    fn = getattr(L, entry)
    _both_directions(lambda out: check(fn(C.byref(d), ptr(x), ptr(packed), ptr(sc), ptr(sh), ptr(res) if has_res else None, ptr(out), st), entry),
                     (B, cout // 16, Ho, Wo, 16), torch.bfloat16, dev)


def test_one_workgroup_per_item_1x1_forward_equals_reversed(dev):
    """1x1 32 -> 32: cin % 64 != 0 takes the register-staged kernel, whose grid is one workgroup per item"""
    L, st = _lib.lib(), _lib.stream_ptr()
    B, H, W = 5, 24, 40
    g, packed, sc, sh = _operands(dev, 32, 32, 1, 3232)
    x = _blocked(g, B, 32, H, W, dev)
    d = ConvDesc(B, 32, 32, H, W, H, W, 1, 1, 1, 0, 32)
    _both_directions(lambda out: check(L.ay_conv_fwd_bf16(C.byref(d), ptr(x), ptr(packed), ptr(sc), ptr(sh), None, ptr(out), st), "1x1"),
                     (B, 2, H, W, 16), torch.bfloat16, dev)


@pytest.mark.parametrize("cond", ["dyn", "uneven", "few"])
def test_cat_kernel_forward_equals_reversed(dev, cond):
    """route [upsampled x2 | direct] folded into the 1x1 (static dealing, never on a canvas); 24 x 40: 3 x 2 tiles per image"""
    L, st = _lib.lib(), _lib.stream_ptr()
    c1, c2, cout, H, W = 64, 64, 128, 24, 40
    B, n_items, wgs = _pick_batch(cond, lambda B: B * 6)
    g, packed, sc, sh = _operands(dev, c1 + c2, cout, 1, 6464)
    a_half, b_full = _blocked(g, B, c1, H // 2, W // 2, dev), _blocked(g, B, c2, H, W, dev)
    d = ConvDesc(B, c1 + c2, cout, H, W, H, W, 1, 1, 1, 0, cout)
    _both_directions(lambda out: check(L.ay_conv1x1_cat_fwd_bf16(C.byref(d), ptr(a_half), c1, ptr(b_full), ptr(packed), ptr(sc), ptr(sh), ptr(out), st),
                                       "cat"), (B, cout // 16, H, W, 16), torch.bfloat16, dev)


def test_head_decode_forward_equals_reversed(dev):
    """a 24-channel head (3 anchors x (5 + 3 classes), padded to 32) with its decode: prediction rows, fp32"""
    L, st = _lib.lib(), _lib.stream_ptr()
    B, cin, G, A, NC = 5, 64, 40, 3, 3
    g, packed, sc, sh = _operands(dev, cin, 32, 1, 2424)
    sc.fill_(1.0)
    x = _blocked(g, B, cin, G, G, dev)
    anchors = (C.c_float * 6)(10, 13, 16, 30, 33, 23)
    d = ConvDesc(B, cin, A * (5 + NC), G, G, G, G, 1, 1, 0, 1, 32)
    n_total = A * G * G + 7
    _both_directions(lambda out: (out[:, A * G * G:].zero_(),   # rows of other heads: not this launch's
                                  check(L.ay_head_decode_fwd_bf16(C.byref(d), ptr(x), ptr(packed), ptr(sc), ptr(sh), A, NC, 32 * G, anchors, ptr(out),
                                                                  n_total, 0, st), "head + decode")),
                     (B, n_total, 5 + NC), torch.float32, dev)


@pytest.mark.parametrize("cond", ["B3", "dyn"])
def test_fused_block_forward_equals_reversed(dev, cond):
    """fused C = 64 residual block at 64 x 64, 4 x 2 tiles of 16 x 32 per image, static dealing.  B = 3: 24 items, one per
    workgroup; dyn: 8 items per workgroup, the loader running across item boundaries"""
    L, st = _lib.lib(), _lib.stream_ptr()
    Cc, H = 64, 64
    B = 3 if cond == "B3" else _pick_batch("dyn", lambda B: B * 8)[0]
    g, p1, s1, t1 = _operands(dev, Cc, Cc // 2, 1, 641)
    _, p2, s2, t2 = _operands(dev, Cc // 2, Cc, 3, 643)
    x = _blocked(g, B, Cc, H, H, dev)
    _both_directions(lambda out: check(L.ay_resblock_fwd_bf16(ptr(x), ptr(p1), ptr(s1), ptr(t1), 1, ptr(p2), ptr(s2), ptr(t2), 1, ptr(out), B, Cc, H, H, st),
                                       "resblock"), (B, Cc // 16, H, H, 16), torch.bfloat16, dev)


@pytest.mark.parametrize("size", [(64, 64), (64, 66)], ids=["pipelined-64x64", "serial-64x66"])
def test_fused_stem_forward_equals_reversed(dev, size):
    """both stem kernels (W % 4 != 0 takes the serial-phase one), enough images that every workgroup has several items, so that
    the tile ring two items ahead wraps"""
    L, st = _lib.lib(), _lib.stream_ptr()
    H, W = size
    Ho, Wo = H // 2, W // 2
    th = 4 if W % 4 == 0 else 8
    B, n_items, wgs = _pick_batch("dyn", lambda B: B * -(-Ho // th) * -(-Wo // 32))
    g, packed, s1, t1 = _operands(dev, 32, 64, 3, H * 3 + W)
    x = torch.rand(3, 3, H, W, generator=g).to(dev).repeat(-(-B // 3), 1, 1, 1)[:B].contiguous()
    w0 = torch.zeros(32, 32)
    w0[:, :27] = torch.randn(32, 27, generator=g) * 0.3
    w0 = w0.to(torch.bfloat16).to(dev)
    s0, t0 = (torch.rand(32, generator=g) + 0.5).to(dev), (torch.randn(32, generator=g) * 0.2).to(dev)
    _both_directions(lambda out: check(L.ay_stem_s2_fused_fwd(ptr(x), ptr(w0), ptr(s0), ptr(t0), 1, ptr(packed), ptr(s1), ptr(t1), 1, ptr(out), B, H, W, st),
                                       "fused stem"), (B, 4, Ho, Wo, 16), torch.bfloat16, dev)


def _model(tmp_cfg_dir, dev):
    from test_gpu_parity import build_models
    return build_models(3, tmp_cfg_dir, dev, "bf16")[0]


@pytest.mark.parametrize("S,B", [(128, 2), (416, 1)])
def test_model_alternating_plan_equals_forward_plan(tmp_cfg_dir, dev, S, B):
    """the whole network through the plan with alternation off and on: decode output and merge-NMS result identical; the plan
    reverses some but not all launches, the first one (which reads the image) never"""
    from amyloid_yolo_paper_amd.utils import nms_device
    m = _model(tmp_cfg_dir, dev)
    saved = (m.alternate_traversal, m.use_plan)
    try:
        m.use_plan = True
        x = torch.from_numpy(gc.model_inputs(S, B, 5)).to(dev)
        res = {}
        for alt in (False, True):
            m.alternate_traversal = alt
            out = m.forward_device(x).clone()
            res[alt] = (out, [t.clone() for t in nms_device(out, 0.5, 0.4, 512, slot=4)])
            plan = m._plan(B, S, m._prepare(dev), dev)
            rev = [_lib.lib().ay_plan_op_reversed(plan.handle, i) for i in range(len(plan.ops))]
            assert (0 < sum(rev) < len(rev) and rev[0] == 0) if alt else sum(rev) == 0, rev
            assert _lib.lib().ay_conv_get_traversal() == 0, "the plan leaves the thread's direction forward"
        assert torch.equal(res[False][0], res[True][0])
        for a, b in zip(res[False][1], res[True][1]):
            assert torch.equal(a, b)
    finally:
        m.alternate_traversal, m.use_plan = saved


def test_graph_replay_of_the_alternating_plan(tmp_cfg_dir, dev):
    """one captured forward of the alternating plan, replayed once, equals the eager run (the directions live in the kernel nodes)"""
    from amyloid_yolo_paper_amd import utils as ay
    m = _model(tmp_cfg_dir, dev)
    saved = (m.alternate_traversal, m.use_plan)
    try:
        m.use_plan, m.alternate_traversal = True, True
        S, B = 128, 2
        x = torch.from_numpy(gc.model_inputs(S, B, 9)).to(dev)
        ref = m.forward_device(x, out_slot=0).clone()
        torch.cuda.synchronize()
        static_x = torch.zeros_like(x)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            out = m.forward_device(static_x, out_slot=0)
        torch.cuda.synchronize()
        static_x.copy_(x)
        ay.graph_replay(g)
        torch.cuda.synchronize()
        assert torch.equal(out, ref)
    finally:
        m.alternate_traversal, m.use_plan = saved
