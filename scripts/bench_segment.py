"""Cost of plaque segmentation (THE SEGMENT RULE, include/amyloid_yolo.h; csrc/ay_segment.hip), one process, the contenders of every
part taken in turn inside one timed loop, median (min .. max) over the rounds:
  (a) ordinary boxes   4 096 boxes of 44 .. 52 px, margin 8, on a resident synthetic strip (harness.synthetic_strip, TX tiles):
                       ay_box_segments_u8 beside ay_stain_load_u8's box pass on the same rows.  The box pass is the yardstick: it
                       reads the same pixels without labelling them.  The calls rotate over COPIES copies of the strip.
  (b) worst windows    one 255 x 255 window per call: full, checkerboard, one-pixel spiral, serpentine (and an empty one: the floor of
                       a call, two launches).  The number that says whether the labelling is sane.
  (c) end to end       wsi.segment_boxes beside wsi.stain_load(raster, rows) on scripts/bench_wsi.py's slide (TY x TX tiles in host
                       memory): wall time with a device synchronisation, the share of strips visited; once with the boxes all over the
                       slide, once with the boxes in its top quarter.
bg_level 170 as in the other benches on the synthetic tiles.
usage: timeout 600 python scripts/bench_segment.py [TX] [TY] [--reps 20] [--warm 3] [--copies 3] [--out profiles/segment.txt]"""
import argparse
import statistics
import time

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import StainMap, segment_boxes, stain_load

ap = argparse.ArgumentParser()
ap.add_argument("tx", nargs="?", type=int, default=16)
ap.add_argument("ty", nargs="?", type=int, default=4)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--copies", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
TX, TY, tile, BG, THRES_BIN, CORE_BIN, MARGIN, N_BOXES = a.tx, a.ty, 1536, 170, 10, 64, 8, 4096
report = harness.Report()
say = report.say


def boxes_in(n, H, W, seed, y_hi=None):
    """n rows [n, 7]: boxes of 44 .. 52 px whose windows lie inside the H x W slide (above row y_hi)"""
    rng = np.random.default_rng(seed)
    side = rng.uniform(44, 52, (n, 2))
    x = rng.uniform(MARGIN, W - MARGIN - 52, n)
    y = rng.uniform(MARGIN, (y_hi or H) - MARGIN - 52, n)
    rows = np.zeros((n, 7), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3], rows[:, 4:6] = x, y, x + side[:, 0], y + side[:, 1], 0.9
    return rows


dev = torch.device("cuda:0")
L, sp = _lib.lib(), _lib.stream_ptr()
identity = StainMap.identity()
params = identity.params
strip_h = harness.synthetic_strip(TX, tile)
say("%s; bg_level %d, thres_bin %d, core_bin %d, margin %d; %d warm + %d timed rounds" % (torch.cuda.get_device_name(0), BG, THRES_BIN, CORE_BIN,
                                                                                         MARGIN, a.warm, a.reps))

# ---- (a) ordinary boxes on a resident strip ---------------------------------------------------------------------------------------
strips = harness.Rotation(torch.from_numpy(strip_h).to(dev), a.copies)
next_strip = strips.next
H, W = strip_h.shape[:2]
rows_h = boxes_in(N_BOXES, H, W, 1)
rows = torch.from_numpy(rows_h).to(dev)
seg = torch.zeros(N_BOXES, 20, device=dev, dtype=torch.int32)
box = torch.zeros(N_BOXES, 4, device=dev, dtype=torch.int64)
flags = torch.zeros(1, device=dev, dtype=torch.int32)


def segments(region, h, w, r, n, out):
    check(L.ay_box_segments_u8(region, h, w, w * 3, 1, 0, 0, h, w, 0, h, BG, ptr(params), 1, THRES_BIN, CORE_BIN, MARGIN, 1, ptr(r), n, ptr(out),
                               ptr(flags), sp), "ay_box_segments_u8")


ms = harness.time_calls([lambda: segments(next_strip(), H, W, rows, N_BOXES, seg),
                         lambda: check(L.ay_stain_load_u8(next_strip(), H, W, W * 3, 1, 0, 0, H, W, BG, ptr(params), 1, THRES_BIN, 128, None, ptr(rows),
                                                          N_BOXES, ptr(box), ptr(flags), sp), "ay_stain_load_u8")], a.warm, a.reps)
s = seg.cpu().numpy()
say("(a) %d boxes of 44 .. 52 px on a resident strip of %d x %d, over %d copies" % (N_BOXES, H, W, a.copies))
say("    ay_box_segments_u8           : %s per call, %.2f us per box" % (harness.fmt_round(ms[0]), 1e3 * statistics.median(ms[0]) / N_BOXES))
say("    ay_stain_load_u8 boxes only  : %s per call, %.2f us per box" % (harness.fmt_round(ms[1]), 1e3 * statistics.median(ms[1]) / N_BOXES))
say("    segments / box pass = %.2f (medians); %d rows with a selected component, median area %d px, median %d positive pixels per window, "
    "flags %d" % (statistics.median(ms[0]) / statistics.median(ms[1]), int((s[:, 7] > 0).sum()), int(np.median(s[s[:, 7] > 0, 7])) if (s[:, 7] > 0).any() else 0,
                  int(np.median(s[:, 5])), int(flags.item())))
assert not int(flags.item()) and (s[:, 0] == 0).all()
del strips, next_strip

# ---- (b) the worst windows, one per call ----------------------------------------------------------------------------------------------
n = 255
yy, xx = np.mgrid[0:n, 0:n]


def spiral():
    m = np.zeros((n, n), bool)
    x = y = d = 0
    m[0, 0] = True
    inside = lambda u, v: 0 <= u < n and 0 <= v < n
    while True:
        dx, dy = ((1, 0), (0, 1), (-1, 0), (0, -1))[d]
        moved = False
        while inside(x + dx, y + dy) and not m[y + dy, x + dx] and not (inside(x + 2 * dx, y + 2 * dy) and m[y + 2 * dy, x + 2 * dx]):
            x, y, moved = x + dx, y + dy, True
            m[y, x] = True
        if not moved:
            return m
        d = (d + 1) % 4


serp = np.zeros((n, n), bool)
serp[0::2], serp[1::4, n - 1], serp[3::4, 0] = True, True, True
patterns = [("empty", np.zeros((n, n), bool)), ("full", np.ones((n, n), bool)), ("checkerboard", (xx + yy) % 2 == 0), ("spiral", spiral()),
            ("serpentine", serp)]
windows, outs = [], []
for name, m in patterns:
    r = np.empty((n, n, 3), np.uint8)
    r[:] = (150, 150, 200)
    r[m] = (150, 110, 70)
    windows.append(torch.from_numpy(r).to(dev))
    outs.append(torch.zeros(1, 20, device=dev, dtype=torch.int32))
one = torch.tensor([[100, 100, 155, 155, 1, 1, 0]], dtype=torch.float32, device=dev)


def window_call(k):
    check(L.ay_box_segments_u8(ptr(windows[k]), n, n, n * 3, 1, 0, 0, n, n, 0, n, 220, ptr(params), 1, THRES_BIN, CORE_BIN, 100, 1, ptr(one), 1,
                               ptr(outs[k]), ptr(flags), sp), "ay_box_segments_u8")


ms = harness.time_calls([lambda k=k: window_call(k) for k in range(len(patterns))], a.warm, a.reps)
say("(b) one 255 x 255 window per call (one workgroup; two launches)")
for k, (name, m) in enumerate(patterns):
    o = outs[k].cpu().numpy()[0]
    assert o[0] == 0 and o[5] == int(m.sum()) and o[7] == (int(m.sum()) if m.any() else 0)
    say("    %-13s: %s, %d positive pixels in one component" % (name, harness.fmt_round(ms[k]), int(o[7])))

# ---- (c) end to end on a slide in host memory ---------------------------------------------------------------------------------------
raster = np.concatenate([np.roll(strip_h, 97 * j, 1) for j in range(TY)], 0)
SH, SW = raster.shape[:2]
say("(c) a slide of %d x %d (%.2f GB) in host memory, %d boxes; wall time with a device synchronisation" % (SH, SW, raster.nbytes / 1e9, N_BOXES))
for what, rws in (("boxes all over the slide ", boxes_in(N_BOXES, SH, SW, 2)), ("boxes in the top quarter ", boxes_in(N_BOXES, SH, SW, 3, SH // 4))):
    wall = {"segment_boxes": [], "stain_load   ": []}
    visited = None
    for i in range(1 + max(2, a.reps // 6)):
        for name, call in (("segment_boxes", lambda: segment_boxes(raster, rws, MARGIN, 1, BG, THRES_BIN / 64, CORE_BIN / 64)),
                           ("stain_load   ", lambda: stain_load(raster, rws, 128, 1, BG, THRES_BIN / 64))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = call()
            torch.cuda.synchronize()
            if i:
                wall[name].append(1e3 * (time.perf_counter() - t0))
            if "strips" in res:
                visited = res["strips"]
                assert res["flags"] == 0
    for name, v in wall.items():
        say("    %s %s: %s" % (what, name, harness.fmt_round(v)))
    say("    %s segment_boxes visited %d of %d strips; segment_boxes / stain_load = %.2f (medians)"
        % (what, visited[0], visited[1], statistics.median(wall["segment_boxes"]) / statistics.median(wall["stain_load   "])))
report.write(a.out)
