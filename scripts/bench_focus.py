"""Cost of the focus pass (THE FOCUS RULE, include/amyloid_yolo.h) on the synthetic strip (harness.synthetic_strip): one resident strip
of TX 1536-px tiles, one process, five calls taken in turn inside one timed loop:
  ay_tile_tissue_u8      one tile row (the floor: a minimum and a compare per pixel)
  ay_stain_load_u8       cells only (cell 128): the yardstick, a read stream over the same bytes with the same items
  ay_focus_u8            cells only (cell 128) | boxes only | both
The strip lies at rows STRIP_ROW .. of a 70 000-px square slide and the focus calls own all of its rows but the first and the last (what
a strip of wsi.focus_map owns); the rows are harness.slide_rows' (250 000 boxes of 8..47 px all over the slide: most miss the strip).
CALL time: after WARM warm rounds, REPS rounds, two device events around each call; median (min .. max).  Calls are kernel launches
only, so this is launch overhead plus kernels.  GB/s of READS: 3 B per source pixel of the strip over the median (the focus cell pass
reads two halo rows per band of 32 on top, 6 % more than that; the box pass reads only the pixels of its boxes: for it the figure is
not a bandwidth and is not printed).  bg_level 170 as in bench_load.py.
WHERE THE BYTES COME FROM: the strip (226 MB at TX = 32) is smaller than the MI355X's 256 MiB last-level cache, and a loop that reads
one buffer again and again may be served from it, which no strip of wsi.focus_map is (each is uploaded and read once).  So the calls
rotate over COPIES copies of the strip at different addresses (default 4); --copies 1 is the re-read buffer, for comparison.  The
ratios between the calls of one run are the yardstick either way.
usage: timeout 300 python scripts/bench_focus.py [TX] [--reps 20] [--warm 3] [--copies 4] [--out profiles/focus.txt]
       (the whole run takes a few seconds; the time limit keeps a hung device from holding a shared machine)"""
import argparse
import statistics

import harness
import torch

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import StainMap, tile_grid

ap = argparse.ArgumentParser()
ap.add_argument("tx", nargs="?", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--copies", type=int, default=4, help="copies of the strip the calls rotate over (1: one buffer, re-read)")
ap.add_argument("--out", default=None)
ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
a = ap.parse_args()
TX, tile, BG, CELL, THRES_BIN, SIDE, STRIP_ROW = a.tx, 1536, 170, 128, 10, 70000, 20 * 1536
report = harness.Report()
say = report.say

dev = torch.device("cuda:0")
strip = torch.from_numpy(harness.synthetic_strip(TX, tile)).to(dev)
strips = harness.Rotation(strip, a.copies)
next_strip = strips.next            # the pointer of the copy this call reads: the one read longest ago
H, W = strip.shape[:2]
assert STRIP_ROW + H <= SIDE
rows_h = harness.slide_rows(250000, 50000, float(W))[0]          # the focus pass takes whole rows of the slide: the slide is as wide as the strip
rows = torch.from_numpy(rows_h).to(dev)
M = len(rows_h)
on_strip = int(((rows_h[:, 3] > STRIP_ROW) & (rows_h[:, 1] < STRIP_ROW + H) & (rows_h[:, 2] > 0) & (rows_h[:, 0] < W)).sum())
say("%s: strip %d x %d, %.3f GB, at row %d of a %d x %d slide; %d rows, about %d of them on the strip; cell %d, bg_level %d; "
    "%d warm + %d timed rounds; the calls rotate over %d cop%s of the strip"
    % (torch.cuda.get_device_name(0), H, W, strip.numel() / 1e9, STRIP_ROW, SIDE, W, M, on_strip, CELL, BG, a.warm, a.reps, a.copies,
       "y (one buffer, re-read: it fits the last-level cache)" if a.copies == 1 else "ies"))
L, sp = _lib.lib(), _lib.stream_ptr()
params = StainMap.identity().params
gy, gx, _ = tile_grid(SIDE, W, CELL)
counts = torch.empty(TX, device=dev, dtype=torch.int32)
load_cells = torch.zeros(gy, gx, 3, device=dev, dtype=torch.int64)
cells = [torch.zeros(gy, gx, 3, device=dev, dtype=torch.int64) for _ in range(2)]            # cells only; both
boxes = [torch.zeros(M, 3, device=dev, dtype=torch.int64) for _ in range(2)]                 # boxes only; both
flags = torch.zeros(1, device=dev, dtype=torch.int32)


def focus(c, b):
    check(L.ay_focus_u8(next_strip(), H, W, W * 3, 1, STRIP_ROW, SIDE, W, STRIP_ROW + 1, STRIP_ROW + H - 1, BG, CELL, ptr(c),
                        ptr(rows) if b is not None else None, M if b is not None else 0, ptr(b), ptr(flags) if b is not None else None, sp),
          "ay_focus_u8")


calls = [("ay_tile_tissue_u8           ", lambda: check(L.ay_tile_tissue_u8(next_strip(), H, W, W * 3, 1, tile, tile, 1, TX, BG, ptr(counts), sp), "tissue")),
         ("ay_stain_load_u8 cells only ", lambda: check(L.ay_stain_load_u8(next_strip(), H, W, W * 3, 1, STRIP_ROW, 0, SIDE, W, BG, ptr(params), 1,
                                                                           THRES_BIN, CELL, ptr(load_cells), None, 0, None, None, sp), "load")),
         ("ay_focus_u8 cells only      ", lambda: focus(cells[0], None)),
         ("ay_focus_u8 boxes only      ", lambda: focus(None, boxes[0])),
         ("ay_focus_u8 cells+boxes     ", lambda: focus(cells[1], boxes[1]))]
ms = harness.time_calls([call for _, call in calls], a.warm, a.reps)
reads = strip.numel()
for k, (name, _) in enumerate(calls):
    rate = "" if "boxes only" in name else ", %.0f GB/s of reads" % (reads / statistics.median(ms[k]) / 1e6)
    say("%s: %s per strip%s" % (name, harness.fmt_round(ms[k]), rate))
med = [statistics.median(m) for m in ms]
say("focus cells only / ay_stain_load_u8 cells only = %.2f, focus cells only / ay_tile_tissue_u8 = %.2f, focus cells+boxes / cells only = %.2f (medians)"
    % (med[2] / med[1], med[2] / med[0], med[4] / med[2]))
say("repeat spread (max - min) / median: load cells only %.1f %%, focus cells only %.1f %%" % (100 * harness.spread(ms[1]), 100 * harness.spread(ms[2])))
# the passes counted the same pixels: the evaluated pixels are tissue, the two focus calls agree, the boxes two ways
n = a.warm + a.reps
tissue = int(counts.sum())
evaluated = int(cells[0][:, :, 0].sum()) // n
assert int(load_cells[:, :, 0].sum()) == tissue * n and 0 < evaluated <= tissue
assert torch.equal(cells[0], cells[1]) and torch.equal(boxes[0], boxes[1]) and int(flags.item()) == 0
s = cells[0].sum((0, 1)).tolist()
say("tissue pixels of the strip: %d of %d; evaluated: %d; variance of the Laplacian over the strip: %.1f; boxes with an evaluated pixel: %d; "
    "the passes agree" % (tissue, H * W, evaluated, s[2] / s[0] - (s[1] / s[0]) ** 2, int((boxes[0][:, 0] > 0).sum())))
report.write(a.out, append=a.append)
