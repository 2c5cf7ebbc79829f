"""Training augmentation on the device, fused into the tile ingest (``ay_augment_ingest_u8``, csrc/ay_augment.hip).

The reference trains every model behind an imgaug pipeline (``utils/augmentations.py``): Dropout, Sharpen,
Affine (rotate ±20°, translate ±20 %), AddToBrightness, AddToHue, Fliplr.  imgaug, torchvision and cv2 are not installed where
this project is built, so **parity with imgaug is unpinned**: what this module does is defined by THE AUGMENTATION RULE in
``include/amyloid_yolo.h`` and restated in NumPy by ``tests/augment_reference.py``.  Where it knowingly departs from the reference:

* sharpen and dropout act on the warped image at output resolution, not on the source before the warp;
* brightness is an additive offset on R, G and B;
* hue is a rotation about the grey axis (a 3x3 matrix computed here in float64), not an HSV round trip.  imgaug's hue unit is
  taken as 1/255 of a full turn (its documentation projects ±255 onto OpenCV's 0..180 hue range, i.e. 360°), so ±20 units are
  ±28.2°.  This mapping is a choice, not a pinned fact;
* imgaug's exact kernels and colour spaces are not restated.

The host draws one parameter record per image (``sample_params``) and moves the labels (``transform_labels``); the device applies
the records in one pass over the uploaded uint8 tiles (``augment_ingest_device``).  Nothing random happens on the device.
"""
import ctypes as C
import math
from dataclasses import dataclass

import numpy as np
import torch

from . import _lib
from ._lib import AyError, check
from .upload import pack_records, pinned, record_offset

# numpy mirror of ay_aug_params (include/amyloid_yolo.h; _lib.AugParams is the ctypes mirror)
AUG_DTYPE = np.dtype([("src_offset", "<i8"), ("h", "<i4"), ("w", "<i4"), ("inv", "<f4", (6,)), ("flip", "<i4"),
                      ("sharpen_alpha", "<f4"), ("drop_threshold", "<u4"), ("drop_seed", "<u4"), ("color", "<f4", (9,)),
                      ("bright", "<f4")], align=True)
# numpy mirror of ay_aug_window_params (THE WINDOW RULE; _lib.AugWindowParams is the ctypes mirror)
AUG_WINDOW_DTYPE = np.dtype([("src_offset", "<i8"), ("row_stride", "<i8"), ("bh", "<i4"), ("bw", "<i4"), ("x0", "<i4"), ("y0", "<i4"),
                             ("context", "<i4"), ("fill", "<f4"), ("aug", AUG_DTYPE)], align=True)
HUE_UNIT_DEGREES = 360.0 / 255.0
# footprint(): what the fp32 evaluation of step 3 can differ by from its float64 value, in pixels.  With every coordinate below 2^17
# in magnitude (sizes up to 32768, the kernel's limit, turned and shifted within the default ranges) each of the six fp32 roundings
# of sx is at most half an ulp of 2^17 = 2^-8, and rounding the three float64 coefficients to fp32 moves sx by at most 3 * 2^-24 *
# 2^17: 6 * 2^-8 + 3 * 2^-7 = 0.047 < 1/16.
FOOTPRINT_MARGIN = 0.0625


@dataclass
class AugmentRanges:
    """The reference's ranges.  Every one can be overridden; 0 switches that operation off (identity value)."""
    rotate: float = 20.0        # degrees, drawn from [-rotate, rotate]
    translate: float = 0.2      # fraction of the width and of the height, drawn independently from [-translate, translate]
    brightness: float = 30.0    # added to R, G and B (0..255 units), from [-brightness, brightness]
    hue: float = 20.0           # imgaug hue units (HUE_UNIT_DEGREES each; unpinned), from [-hue, hue]
    dropout: float = 0.01       # per-pixel drop probability p, from [0, dropout]
    sharpen: float = 0.2        # sharpen alpha, from [0, sharpen]
    fliplr: float = 0.5         # probability of a horizontal flip


OFF = AugmentRanges(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def hue_matrix(degrees):
    """rotation of RGB about the grey axis (1,1,1) by `degrees`, float64 [3,3]; 0 gives the identity exactly"""
    t = math.radians(degrees)
    c, s = math.cos(t), math.sin(t)
    k = np.array([[0.0, -1.0, 1.0], [1.0, 0.0, -1.0], [-1.0, 1.0, 0.0]])
    return c * np.eye(3) + ((1.0 - c) / 3.0) * np.ones((3, 3)) + (s / math.sqrt(3.0)) * k


def forward_matrix(degrees, tx, ty):
    """A [2,3] float64: p' = A[:, :2] @ (p - centre) + A[:, 2] + centre, a rotation by `degrees` (from +x towards +y, i.e.
    clockwise on the screen) followed by a translation of (tx, ty) pixels"""
    t = math.radians(degrees)
    c, s = math.cos(t), math.sin(t)
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float64)


def inverse_matrix(A):
    """float64 inverse of the 2x3 affine A, as 2x3"""
    return np.linalg.inv(np.vstack([A, [0.0, 0.0, 1.0]]))[:2]


class AugRecord:
    """one image's parameters: `A` (forward matrix, float64 [2,3], used for the labels) and `dev` (its ay_aug_params row)"""

    def __init__(self, A, dev):
        self.A, self.dev = A, dev

    @property
    def flip(self):
        return int(self.dev["flip"])


class AugTable:
    """the records of a batch: `dev` (structured array of AUG_DTYPE, what the kernel reads) and `A` (float64 [B,2,3])"""

    def __init__(self, dev, A):
        self.dev, self.A = dev, A

    def __len__(self):
        return len(self.dev)

    def __getitem__(self, i):
        return AugRecord(self.A[i], self.dev[i])


def make_table(sizes, A=None, flip=None, sharpen_alpha=None, drop_p=None, drop_seed=None, hue_degrees=None, bright=None):
    """Records for images of `sizes` [(h, w), ...] from explicit values (anything left out is the identity); the images are taken
    to lie one after another, so src_offset is the running sum of h * w * 3."""
    B = len(sizes)
    dev = np.zeros(B, AUG_DTYPE)
    As = np.zeros((B, 2, 3))
    off = 0
    for i, (h, w) in enumerate(sizes):
        r = dev[i]
        r["src_offset"], r["h"], r["w"] = off, h, w
        off += int(h) * int(w) * 3
        As[i] = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) if A is None else A[i]
        r["inv"] = (inverse_matrix(As[i]) + 0.0).astype(np.float32).ravel()     # (+ 0.0: a -0 becomes +0)
        r["flip"] = 0 if flip is None else int(flip[i])
        r["sharpen_alpha"] = 0.0 if sharpen_alpha is None else sharpen_alpha[i] + 0.0
        p = 0.0 if drop_p is None else float(drop_p[i])
        r["drop_threshold"] = min(int(math.floor(p * 2.0 ** 32)), 2 ** 32 - 1)
        r["drop_seed"] = 0 if drop_seed is None else int(drop_seed[i])
        r["color"] = hue_matrix(0.0 if hue_degrees is None else float(hue_degrees[i])).astype(np.float32).ravel() + 0.0
        r["bright"] = 0.0 if bright is None else bright[i] + 0.0
    return AugTable(dev, As)


def identity_params(sizes):
    """records under which ay_augment_ingest_u8 equals ay_ingest_tiles_u8(pad_value=0) bit for bit"""
    return make_table(sizes)


def sample_params(rng, sizes, ranges=None):
    """One record per image of `sizes` [(h, w), ...] from a numpy.random.Generator.  Every image consumes the same draws in the
    same order whatever is switched off, so switching one operation off leaves the others' values as they were."""
    g = ranges or AugmentRanges()
    B = len(sizes)
    A, flip, alpha, p, seed, hue, bright = [], [], [], [], [], [], []
    for h, w in sizes:
        deg = rng.uniform(-1.0, 1.0) * g.rotate
        tx = rng.uniform(-1.0, 1.0) * g.translate * w
        ty = rng.uniform(-1.0, 1.0) * g.translate * h
        A.append(forward_matrix(deg, tx, ty))
        bright.append(rng.uniform(-1.0, 1.0) * g.brightness)
        hue.append(rng.uniform(-1.0, 1.0) * g.hue * HUE_UNIT_DEGREES)
        p.append(rng.uniform(0.0, 1.0) * g.dropout)
        seed.append(int(rng.integers(0, 2 ** 32, dtype=np.uint64)))
        alpha.append(rng.uniform(0.0, 1.0) * g.sharpen)
        flip.append(int(rng.uniform(0.0, 1.0) < g.fliplr))
    return make_table(sizes, A if B else None, flip, alpha, p, seed, hue, bright)


def transform_labels(boxes, h, w, rec, min_visible=0.0):
    """Labels ``class cx cy w h`` (normalised to the h x w tile) moved with the image: in continuous coordinates (pixel i spans
    [i, i+1), centre (w/2, h/2)) the four corners go through rec.A, then through the flip x -> w - x; the axis-aligned bounding
    box of the result (as imgaug does) is clipped to the image, a box whose clipped width or height is <= 0 is dropped, and what
    remains gets the pad offsets and the re-normalisation by D = max(h, w) of ``datasets.default_transform``.  -> float64 [m,5]
    ``min_visible`` > 0 also drops a box whose clipped area is below that fraction of the area of its unclipped transformed bounding
    box (what the clip left of it is too little to be called the object); the default drops nothing more."""
    b = np.array(boxes, dtype=np.float64, copy=True).reshape(-1, 5)
    if not len(b):
        return b
    x1, x2 = w * (b[:, 1] - b[:, 3] / 2), w * (b[:, 1] + b[:, 3] / 2)
    y1, y2 = h * (b[:, 2] - b[:, 4] / 2), h * (b[:, 2] + b[:, 4] / 2)
    cx, cy = w / 2.0, h / 2.0
    xs = np.stack([x1, x2, x1, x2], 1) - cx
    ys = np.stack([y1, y1, y2, y2], 1) - cy
    A = rec.A
    px = A[0, 0] * xs + A[0, 1] * ys + A[0, 2] + cx
    py = A[1, 0] * xs + A[1, 1] * ys + A[1, 2] + cy
    if rec.flip:
        px = w - px
    x1, x2 = np.clip(px.min(1), 0.0, w), np.clip(px.max(1), 0.0, w)
    y1, y2 = np.clip(py.min(1), 0.0, h), np.clip(py.max(1), 0.0, h)
    keep = (x2 - x1 > 0) & (y2 - y1 > 0)
    if min_visible > 0.0:
        full = (px.max(1) - px.min(1)) * (py.max(1) - py.min(1))
        keep &= (x2 - x1) * (y2 - y1) >= min_visible * full
    b, x1, x2, y1, y2 = b[keep], x1[keep], x2[keep], y1[keep], y2[keep]
    D = max(h, w)
    p1 = abs(h - w) // 2
    left, top = (0, p1) if h <= w else (p1, 0)
    b[:, 1] = ((x1 + x2) / 2 + left) / D
    b[:, 2] = ((y1 + y2) / 2 + top) / D
    b[:, 3] = (x2 - x1) / D
    b[:, 4] = (y2 - y1) / D
    return b


def _as_u8(t):
    t = torch.as_tensor(t)
    assert t.dtype == torch.uint8 and t.dim() == 3 and t.shape[-1] == 3, "uint8 [H,W,3] tiles"
    return t


def augment_ingest_device(tiles, params, img_size, out=None):
    """uint8 HWC tiles (a list of [H,W,3] arrays or tensors of any sizes, or one [B,H,W,3] tensor) + their records (an AugTable or a
    structured array of AUG_DTYPE) -> float32 [B,3,S,S] on the current HIP device.  Host tiles and the records go up in ONE copy (the
    records ride behind the pixels), then one kernel call (``ay_augment_ingest_u8``).  src_offset of the records is set here, from
    the order of `tiles`.  No CPU fallback."""
    if not torch.cuda.is_available():
        raise AyError("no HIP device: augment_ingest_device has no CPU fallback")
    resident = None
    if isinstance(tiles, (list, tuple)):
        tiles = [_as_u8(t) for t in tiles]
    else:
        t = torch.as_tensor(tiles)
        assert t.dtype == torch.uint8 and t.dim() == 4 and t.shape[-1] == 3, "uint8 [B,H,W,3] tiles"
        if t.is_cuda:
            resident = t.contiguous().reshape(-1)
        tiles = list(t.unbind(0))
    B = len(tiles)
    recs = np.array(params.dev if isinstance(params, AugTable) else params, dtype=AUG_DTYPE, copy=True)
    assert B > 0 and recs.shape == (B,), "one record per tile"
    offs = np.concatenate([[0], np.cumsum([t.numel() for t in tiles])]).astype(np.int64)
    for i, t in enumerate(tiles):
        assert (int(recs[i]["h"]), int(recs[i]["w"])) == (t.shape[0], t.shape[1]), "record %d is for another tile size" % i
    recs["src_offset"] = offs[:B]
    n_img = int(offs[B])
    rec_bytes = torch.from_numpy(recs.view(np.uint8).reshape(-1))
    dev = torch.device("cuda", torch.cuda.current_device())
    if resident is None and all(t.is_cuda for t in tiles):
        resident = torch.cat([t.reshape(-1) for t in tiles])
    if resident is not None:                   # the pixels are on the device already: only the table goes up
        table = rec_bytes.to(dev, non_blocking=True)
        src_ptr, table_ptr = resident.data_ptr(), table.data_ptr()
    else:
        host = pinned(record_offset(n_img) + rec_bytes.numel())
        for i, t in enumerate(tiles):
            host[int(offs[i]):int(offs[i + 1])].copy_(t.reshape(-1))
        tab = pack_records(host.numpy(), n_img, recs)
        resident = host.to(dev, non_blocking=True)
        src_ptr, table_ptr = resident.data_ptr(), resident.data_ptr() + tab
    if out is None:
        out = torch.empty(B, 3, img_size, img_size, device=dev, dtype=torch.float32)
    assert out.shape == (B, 3, img_size, img_size) and out.is_contiguous() and out.dtype == torch.float32 and out.is_cuda
    check(_lib.lib().ay_augment_ingest_u8(C.c_void_p(src_ptr), n_img, C.c_void_p(table_ptr), B, img_size, _lib.ptr(out),
                                          _lib.stream_ptr()), "ay_augment_ingest_u8")
    return out


class WindowTable:
    """the window records of a batch: `dev` (structured array of AUG_WINDOW_DTYPE, what ay_augment_ingest_window_u8 reads) and `A`
    (float64 [B,2,3], the forward matrices for the labels)"""

    def __init__(self, dev, A):
        self.dev, self.A = dev, A

    def __len__(self):
        return len(self.dev)

    def __getitem__(self, i):
        return AugRecord(self.A[i], self.dev[i]["aug"])


def make_window_table(table, blocks, origins, context=True, fill=255.0, src_offsets=None, row_strides=None):
    """Window records (THE WINDOW RULE) from an AugTable whose ``h, w`` are the windows' sizes: ``blocks`` [(bh, bw), ...] are the
    pixels that may be read and ``origins`` [(x0, y0), ...] the windows' origins in block pixels.  ``row_strides`` default to
    ``3 * bw`` and ``src_offsets`` to the blocks lying one after another (empty blocks take no room)."""
    B = len(table)
    assert len(blocks) == B and len(origins) == B
    dev = np.zeros(B, AUG_WINDOW_DTYPE)
    dev["aug"] = table.dev
    dev["aug"]["src_offset"] = 0
    off = 0
    for i, ((bh, bw), (x0, y0)) in enumerate(zip(blocks, origins)):
        r = dev[i]
        r["bh"], r["bw"], r["x0"], r["y0"] = bh, bw, x0, y0
        r["row_stride"] = 3 * max(int(bw), 0) if row_strides is None else row_strides[i]
        r["src_offset"] = off if src_offsets is None else src_offsets[i]
        if bh > 0 and bw > 0:
            off += (int(bh) - 1) * int(r["row_stride"]) + 3 * int(bw)
    dev["context"] = np.asarray(context, dtype=bool).astype(np.int32)
    dev["fill"] = fill
    return WindowTable(dev, np.array(table.A, dtype=np.float64, copy=True))


def footprint(rec, tile, img_size):
    """The integer bounding box ``(x1, y1, x2, y2)`` (half open, in window coordinates, of any sign) of every tap step 4 can touch
    for this record on an ``(h, w) = tile`` window (an int for a square one) at output size ``img_size``.  Steps 1-2 give integer
    positions inside ``[-left, D - 1 - left] x [-top, D - 1 - top]`` (mirrored by the flip); step 3 is affine, so its extremes lie
    at the corners of that rectangle; they are computed here in float64 from the float64 inverse of ``rec.A`` and widened by
    ``FOOTPRINT_MARGIN`` for the kernel's fp32 evaluation; the taps are ``floor`` and ``floor + 1`` of the result."""
    h, w = (int(tile), int(tile)) if np.isscalar(tile) else (int(tile[0]), int(tile[1]))
    assert 0 < h <= 32768 and 0 < w <= 32768 and img_size > 0
    D = max(h, w)
    top = (w - h) // 2 if h <= w else 0
    left = (h - w) // 2 if h > w else 0
    qx = np.array([-left, D - 1 - left], dtype=np.float64)
    if rec.flip:
        qx = (w - 1) - qx
    qy = np.array([-top, D - 1 - top], dtype=np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    inv = inverse_matrix(rec.A)
    xc, yc = np.meshgrid(qx - cx, qy - cy)
    sx = inv[0, 0] * xc + inv[0, 1] * yc + inv[0, 2] + cx
    sy = inv[1, 0] * xc + inv[1, 1] * yc + inv[1, 2] + cy
    m = FOOTPRINT_MARGIN
    return (int(math.floor(sx.min() - m)), int(math.floor(sy.min() - m)),
            int(math.floor(sx.max() + m)) + 2, int(math.floor(sy.max() + m)) + 2)


def launch_windows(src_ptr, src_bytes, table_ptr, B, img_size, out):
    """one call of ``ay_augment_ingest_window_u8`` on the current stream (raw device addresses)"""
    assert out.shape == (B, 3, img_size, img_size) and out.is_contiguous() and out.dtype == torch.float32 and out.is_cuda
    check(_lib.lib().ay_augment_ingest_window_u8(C.c_void_p(src_ptr), src_bytes, C.c_void_p(table_ptr), B, img_size, _lib.ptr(out),
                                                 _lib.stream_ptr()), "ay_augment_ingest_window_u8")
    return out


def augment_ingest_windows_device(src, table, img_size, out=None):
    """Windows of one source buffer -> float32 [B,3,S,S] on the current HIP device (``ay_augment_ingest_window_u8``).  ``src``: a
    uint8 tensor of any shape, taken as its bytes; on the device it is read in place and only the records go up, on the host
    (pinned or not) it goes up in ONE copy with the records behind it.  ``table``: a WindowTable or a structured array of
    AUG_WINDOW_DTYPE, used as it is (``src_offset`` counts from the first byte of ``src``).  No CPU fallback."""
    if not torch.cuda.is_available():
        raise AyError("no HIP device: augment_ingest_windows_device has no CPU fallback")
    src = torch.as_tensor(src)
    assert src.dtype == torch.uint8 and src.is_contiguous() and src.numel() > 0, "a contiguous uint8 buffer"
    recs = np.array(table.dev if isinstance(table, WindowTable) else table, dtype=AUG_WINDOW_DTYPE, copy=True)
    B, n = len(recs), src.numel()
    assert B > 0 and recs.ndim == 1
    rec_bytes = torch.from_numpy(recs.view(np.uint8).reshape(-1))
    dev = torch.device("cuda", torch.cuda.current_device())
    if src.is_cuda:
        resident, tab_dev = src, rec_bytes.to(dev, non_blocking=True)
        src_ptr, table_ptr = src.data_ptr(), tab_dev.data_ptr()
    else:
        host = pinned(record_offset(n) + rec_bytes.numel())
        host[:n].copy_(src.reshape(-1))
        tab = pack_records(host.numpy(), n, recs)
        resident = host.to(dev, non_blocking=True)
        src_ptr, table_ptr = resident.data_ptr(), resident.data_ptr() + tab
    if out is None:
        out = torch.empty(B, 3, img_size, img_size, device=dev, dtype=torch.float32)
    return launch_windows(src_ptr, n, table_ptr, B, img_size, out)


class DeviceAugmenter:
    """The training stream's augmenter: ``aug(tiles, boxes_per_tile, img_size) -> (imgs [B,3,S,S] fp32, targets [n,6])``, both on
    the device, the sample index in column 0 of the targets as ``ListDataset.collate_fn`` writes it.  The parameter stream is
    ``numpy.random.default_rng([seed, rank])``: ranks augment differently and a run is reproducible.  Callables appended to
    ``hooks`` see every ``(imgs, targets)`` that leaves."""

    def __init__(self, seed, rank=0, ranges=None):
        self.rng = np.random.default_rng([seed, rank])
        self.ranges = ranges or AugmentRanges()
        self.hooks = []

    def __call__(self, tiles, boxes_per_tile, img_size):
        tiles = [_as_u8(t) for t in tiles]
        assert len(tiles) == len(boxes_per_tile)
        sizes = [(t.shape[0], t.shape[1]) for t in tiles]
        table = sample_params(self.rng, sizes, self.ranges)
        imgs = augment_ingest_device(tiles, table, img_size)
        rows = [np.zeros((0, 6))]
        for k, (boxes, (h, w)) in enumerate(zip(boxes_per_tile, sizes)):
            b = transform_labels(np.asarray(boxes, dtype=np.float64), h, w, table[k])
            rows.append(np.concatenate([np.full((len(b), 1), float(k)), b], 1))
        targets = torch.from_numpy(np.concatenate(rows, 0)).float().to(imgs.device)
        for hook in self.hooks:
            hook(imgs, targets)
        return imgs, targets
