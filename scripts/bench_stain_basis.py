"""Cost of the two passes of the stain basis estimate (THE BASIS RULE, include/amyloid_yolo.h) on the synthetic strip of
scripts/bench_stain.py and scripts/bench_load.py (harness.synthetic_strip): one resident strip of TX 1536-px tiles, one process, four
calls taken in turn inside one timed loop:
  ay_tile_tissue_u8             one tile row (the floor: a minimum and a compare per pixel)
  ay_stain_hist_u8              the yardstick: the same bytes, both stains unmixed in fp32, two LDS adds per tissue pixel
  ay_stain_moments_u8           pass 1: nine integer multiply-adds per selected pixel in registers, 11 atomics per workgroup
  ay_stain_direction_hist_u8    pass 2: two projections, one unsigned division and one LDS add per selected pixel
The plane of pass 2 is the one the host takes from pass 1 on this strip (wsi.basis_plane), as wsi.estimate_basis does.
CALL time: after WARM warm rounds, REPS rounds, two device events around each call; median (min .. max).  Calls are kernel launches
only, so this is launch overhead plus kernels.  GB/s of READS: 3 B per source pixel of the strip over the median.  bg_level 170 as in
bench_stain.py; beta 0.15.
WHERE THE BYTES COME FROM: the strip (226 MB at TX = 32) is smaller than the MI355X's 256 MiB last-level cache, and a loop that reads
one buffer again and again may be served from it, which no strip of wsi.estimate_basis is (each is uploaded and read once).  So the
calls rotate over COPIES copies of the strip at different addresses (default 4), as in bench_load.py; --copies 1 is the re-read buffer.
The ratios between the calls of one run are the yardstick either way.
--out keeps the lines tests/test_stain_basis_cpu.py wrote into the same file (they begin with "normalisation gap").
usage: timeout 300 python scripts/bench_stain_basis.py [TX] [--reps 20] [--warm 3] [--copies 4] [--out profiles/stain_basis.txt]
       (the whole run takes a few seconds; the time limit keeps a hung device from holding a shared machine)"""
import argparse
import statistics

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import StainMap

ap = argparse.ArgumentParser()
ap.add_argument("tx", nargs="?", type=int, default=32)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--copies", type=int, default=4, help="copies of the strip the calls rotate over (1: one buffer, re-read)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
TX, tile, BG, BETA_Q = a.tx, 1536, 170, 154
report = harness.Report()
say = report.say

dev = torch.device("cuda:0")
strip = torch.from_numpy(harness.synthetic_strip(TX, tile)).to(dev)
strips = harness.Rotation(strip, a.copies)
next_strip = strips.next            # the pointer of the copy this call reads: the one read longest ago
H, W = strip.shape[:2]
say("%s: strip %d x %d, %.3f GB; bg_level %d, beta_q %d; %d warm + %d timed rounds; the calls rotate over %d cop%s of the strip"
    % (torch.cuda.get_device_name(0), H, W, strip.numel() / 1e9, BG, BETA_Q, a.warm, a.reps, a.copies,
       "y (one buffer, re-read: it fits the last-level cache)" if a.copies == 1 else "ies"))
L, sp = _lib.lib(), _lib.stream_ptr()
params = StainMap.identity().params
odq = wsi._params_to_device(wsi.basis_tables(), dev)
counts = torch.empty(TX, device=dev, dtype=torch.int32)
hist = torch.zeros(1025, device=dev, dtype=torch.int64)
moments = torch.zeros(wsi.BASIS_MOMENT_WORDS, device=dev, dtype=torch.int64)
dirs = torch.zeros(wsi.BASIS_DIR_BINS + 2, device=dev, dtype=torch.int64)


def pass1(out):
    check(L.ay_stain_moments_u8(next_strip(), H, W, W * 3, 1, BG, BETA_Q, ptr(odq), ptr(out), sp), "ay_stain_moments_u8")


first = torch.zeros_like(moments)
pass1(first)
first = first.cpu().numpy()
eq1, eq2, eig = wsi.basis_plane(first)
say("pass 1 on the strip: %d tissue pixels, %d selected; plane eq1 %s, eq2 %s" % (first[0], first[1], eq1.tolist(), eq2.tolist()))
plane = [int(v) for v in eq1] + [int(v) for v in eq2]
calls = [("ay_tile_tissue_u8         ", lambda: check(L.ay_tile_tissue_u8(next_strip(), H, W, W * 3, 1, tile, tile, 1, TX, BG, ptr(counts), sp), "tissue")),
         ("ay_stain_hist_u8          ", lambda: check(L.ay_stain_hist_u8(next_strip(), H, W, W * 3, 1, BG, ptr(params), ptr(hist), sp), "hist")),
         ("ay_stain_moments_u8       ", lambda: pass1(moments)),
         ("ay_stain_direction_hist_u8", lambda: check(L.ay_stain_direction_hist_u8(next_strip(), H, W, W * 3, 1, BG, BETA_Q, *plane, ptr(odq), ptr(dirs), sp),
                                                      "ay_stain_direction_hist_u8"))]
ms = harness.time_calls([call for _, call in calls], a.warm, a.reps)
reads = strip.numel()
for k, (name, _) in enumerate(calls):
    say("%s: %s per strip, %.0f GB/s of reads" % (name, harness.fmt_round(ms[k]), reads / statistics.median(ms[k]) / 1e6))
med = [statistics.median(m) for m in ms]
say("moments / ay_stain_hist_u8 = %.2f, moments / ay_tile_tissue_u8 = %.2f, direction hist / ay_stain_hist_u8 = %.2f, "
    "direction hist / ay_tile_tissue_u8 = %.2f (medians)" % (med[2] / med[1], med[2] / med[0], med[3] / med[1], med[3] / med[0]))
say("repeat spread (max - min) / median: moments %.1f %%, direction hist %.1f %%" % (100 * harness.spread(ms[2]), 100 * harness.spread(ms[3])))
# the passes counted the same pixels
n = a.warm + a.reps
tissue = int(counts.sum())
m, d = moments.cpu().numpy(), dirs.cpu().numpy()
assert int(hist[1024]) == tissue * n and np.array_equal(m, first * n) and int(first[0]) == tissue
assert int(d[513]) == int(first[1]) * n == int(d[:513].sum())
say("tissue pixels of the strip: %d of %d; selected: %d; outside the half plane: %d; the passes agree" % (tissue, H * W, first[1], d[512] // n))
report.write(a.out, keep_prefix="normalisation gap")
