"""Exact reference for LARGE batches of the persistent convolution launches (TEST INFRASTRUCTURE ONLY -- never imported by the
product): tests/test_streams_cpu.py asserts the conditions below on the reference alone, tests/test_gpu_streams.py compares the
kernels with it.

A convolution treats every image of a batch on its own, so the exact output of a batch of B images with image[i] = base[i % P] is
the P-image reference of conv_exact_reference.conv_reference indexed the same way.  P = 7 for the operands of one stream and P = 5
for those of a second one: both are coprime to the 8 XCD ranges a launch is cut into and to the power-of-two tile counts, so no two
items that lie a whole number of ranges, rows of tiles or workgroups apart belong to images of the same residue class.  B = P is
part of conv_reference's generator key: the two operand sets differ in their filters as well.

What makes "computed from the wrong image" visible: for every pair of distinct base images and every output tile of the kernel's
tile size at least 90 % of the tile's values differ between the two images (min_tile_difference; measured: DESIGN.md, the record
of the dealing protocol), so a tile computed from a neighbouring image's pixels, or left over from one, fails in that tile.

BASE_CASES: the shapes of test_gpu_traversal.CONV_SHAPES that have a ragged last tile -- the smallest each entry point takes.
geometry(): the batch of an item-count condition of that module (dyn, uneven, few), from its _pick_batch and _canvas_items."""
import ctypes as C

import torch

import conv_exact_reference as R

PERIODS = (7, 5)
MIN_TILE_DIFFERENCE = 0.9

# name: (entry point, (cin, cout, k, stride, H, W, leaky, residual, out_f32), tile rows, canvas allowed, multiple of cout_pad, D)
# D = the statically dealt items of a workgroup (ItemDealer's fetch-ahead distance): 3 for the 16x16x32 kernel, and for the ring
# kernel 3 with two or more stages per item, 5 with one (cin / (16 NK) < 2: all three ring shapes here)
BASE_CASES = {
    "m16": ("ay_conv3x3_m16_fwd", (32, 128, 3, 1, 48, 160, True, False, False), 16, False, 128, 3),
    "m16-res": ("ay_conv3x3_m16_fwd", (32, 128, 3, 1, 48, 160, True, True, False), 16, False, 128, 3),
    "ring3x3": ("ay_conv_fwd", (16, 128, 3, 1, 48, 160, True, True, False), 16, True, 32, 5),     # 16x32 ring tile, one stage per item
    "ring1x1": ("ay_conv_fwd", (64, 32, 1, 1, 24, 40, True, False, False), 8, True, 32, 5),       # launch<1, 1, 32, .., RING>
    "ring3x3s2": ("ay_conv_fwd", (16, 64, 3, 2, 65, 65, True, False, False), 8, True, 32, 5),     # 33 x 33 out
}
TILE_COLS = 32


def case_of(name, P):
    """the conv_exact_reference case (cin, cout, k, stride, H, W, leaky, residual, out_f32, B = P)"""
    return BASE_CASES[name][1] + (P,)


def tile_rows(name):
    return BASE_CASES[name][2]


def reference(name, P, store):
    return R.conv_reference(case_of(name, P), store)


def min_tile_difference(out, th, tw=TILE_COLS):
    """out [P, C, H, W]: over every pair of distinct images and every th x tw tile (all channels; ragged tiles at the edges as they
    are), the smallest share of the tile's values that differ between the two images"""
    P, _, H, W = out.shape
    worst = 1.0
    for i in range(P):
        for j in range(i + 1, P):
            d = (out[i] != out[j]).to(torch.float64)
            for y0 in range(0, H, th):
                for x0 in range(0, W, tw):
                    worst = min(worst, float(d[:, y0:y0 + th, x0:x0 + tw].mean()))
    return worst


def geometry(name, cond):
    """(B, items, workgroups) of the smallest batch that meets the item-count condition `cond` of test_gpu_traversal (needs the
    device's CU count).  dyn asks for at least 8 items per workgroup; with D = 5 static items that alone leaves 3 / 8 of the items
    to the counter, so the batch then grows until the counter deals more than half of them (still dyn: more items per workgroup)."""
    import test_gpu_traversal as T
    _, (cin, cout, k, stride, H, W, _, _, _), th, canvas, _, D = BASE_CASES[name]
    Ho, Wo = R._out_hw(k, stride, H, W)
    same = (H, W) == ((Ho, Wo) if stride == 1 else (2 * Ho, 2 * Wo))
    # (one channel group per case: cout is the width of the tile its kernel uses)
    items_of = lambda B: (T._canvas_items(B, Ho, Wo, th, TILE_COLS, H * W * B * cin * 2, Ho * Wo * B * cout * 2, same) if canvas
                          else B * -(-Ho // th) * -(-Wo // TILE_COLS))
    B, n, wgs = T._pick_batch(cond, items_of)
    while cond == "dyn" and not counter_deals_most(n, wgs, D):
        B += 1
        n = items_of(B)
    return B, n, wgs


def counter_deals_most(n_items, wgs, D):
    return n_items - D * wgs > n_items // 2


def blocked_cpu(t, dtype, cpad=None):
    """NCHW float32 (values the storage type holds exactly) -> blocked [B][cpad/16][H][W][16] in the storage type, in plain torch;
    channels beyond C are zero"""
    B, Cc, H, W = t.shape
    cpad = -(-Cc // 16) * 16 if cpad is None else cpad
    if cpad != Cc:
        t = torch.cat([t, torch.zeros(B, cpad - Cc, H, W)], 1)
    b = t.view(B, cpad // 16, 16, H, W).permute(0, 1, 3, 4, 2).contiguous().to(R.STORE[dtype])
    assert torch.equal(b.float().permute(0, 1, 4, 2, 3).reshape(B, cpad, H, W), t), "not exact in the storage type"
    return b


def periodic(base, B):
    """device tensor of P images -> B images, image i = base[i % P] (repeated on the device)"""
    P = base.shape[0]
    return base.repeat((-(-B // P),) + (1,) * (base.dim() - 1))[:B].contiguous()


class Prepared:
    """One base case with the operands of period P, for a batch of B images, in three steps that can be interleaved between
    streams: (1) the constructor builds and uploads the operands and the reference and synchronises; (2) launch() issues one launch
    on the CURRENT stream into a NaN-filled guarded output of its own, without any synchronisation; (3) verify(out), after the
    caller has synchronised: every image equals the reference of its residue class (no NaN, equality as numbers, compared on the
    device) and the guard bands are intact."""

    def __init__(self, dev, name, P, dtype, B):
        from amyloid_yolo_paper_amd import _lib
        entry, (cin, cout, k, stride, H, W, leaky, has_res, _), _, _, mult, _ = BASE_CASES[name]
        r = reference(name, P, dtype)
        Ho, Wo = r["out"].shape[2:]
        cpad = -(-cout // mult) * mult
        L = _lib.lib()
        self.name, self.P, self.dtype, self.B, self.dev = name, P, dtype, B, dev
        self.what = f"{entry}_{dtype} {name} P={P} B={B}"
        self.x = periodic(blocked_cpu(r["x"], dtype).to(dev), B)
        self.res = periodic(blocked_cpu(r["res"], dtype, cpad).to(dev), B) if has_res else None
        self.want = blocked_cpu(r["out"], dtype, cpad).to(dev)      # [P][cpad/16][Ho][Wo][16]: padded channels exact zeros
        w = r["w"].contiguous().to(dev)
        self.packed = torch.empty(L.ay_packed_weight_bytes(cpad, cin, k), device=dev, dtype=torch.uint8)
        _lib.check(getattr(L, f"ay_pack_conv_weights_{dtype}")(_lib.ptr(w), _lib.ptr(self.packed), cout, cpad, cin, k, _lib.stream_ptr()))
        self.scale, self.shift = torch.zeros(cpad, device=dev), torch.zeros(cpad, device=dev)
        self.scale[:cout], self.shift[:cout] = r["scale"].to(dev), r["shift"].to(dev)
        self.desc = _lib.ConvDesc(B, cin, cout, H, W, Ho, Wo, k, stride, int(leaky), 0, cpad)
        self.shape = (B, cpad // 16, Ho, Wo, 16)
        self.fn = getattr(L, f"{entry}_{dtype}")
        torch.cuda.synchronize()

    def launch(self):
        from amyloid_yolo_paper_amd import _lib
        from test_gpu_conv_exact import Guarded
        out = Guarded(self.shape, self.dtype, self.dev)
        _lib.check(self.fn(C.byref(self.desc), _lib.ptr(self.x), _lib.ptr(self.packed), _lib.ptr(self.scale), _lib.ptr(self.shift),
                           _lib.ptr(self.res), _lib.ptr(out.t), _lib.stream_ptr()), self.what)
        return out

    def verify(self, out, what=""):
        what = f"{self.what} {what}"
        got = out.t
        n_nan = int(torch.isnan(got).sum())
        assert n_nan == 0, (what, "NaN in the result", n_nan)
        for r in range(min(self.P, self.B)):
            bad = got[r::self.P] != self.want[r]
            if bool(bad.any()):
                idx = [int(v) for v in bad.nonzero()[0]]
                image = r + self.P * idx[0]
                g_, w_ = float(got[(image,) + tuple(idx[1:])]), float(self.want[(r,) + tuple(idx[1:])])
                raise AssertionError(f"{what}: {int(bad.sum())} values of the images of class {r} differ; first in image {image} at "
                                     f"[plane, y, x, lane] = {idx[1:]}: got {g_!r}, want {w_!r}")
        assert out.intact(), (what, "stores outside the output tensor")
