"""Time of one slide-level matching call (ay_slide_match, stats.match_slide) on a synthetic slide: about 250 k detection rows
against 50 k annotations of 8..47 px (the box sizes of the seam merge's 258 633-row slide), inputs, outputs and workspace resident
on the device.
CALL time: after WARM warm calls, REPS times, two device events around ONE call of the C entry point.  The call reads the grid
parameters back in its middle (a reduction over the targets, a pageable copy, a stream synchronisation) and issues five memsets, so
this is NOT a sum of kernel times and cannot be set against the seam merge's "0.95 ms of kernels"; the median of the REPS is
reported with min and max, for K = 1 and K = 3 thresholds, with and without a region of interest, and for cell sides other than the
one the data gives (the result is the same bytes, the work differs; a side is doubled until the grid has at most 2 T cells, so on
this slide nothing below 256 px can be asked for).
KERNEL time: the sum of the six kernels of a call from a rocprofv3 kernel trace of `--calls-only N` (N calls at K = 3, nothing
else), read back with `--kernel-stats DIR`; that figure is the one to hold against the seam merge's.
The wall time of stats.match_slide from host arrays (upload, allocation, call, read-back of the counts) is printed for information.
usage: rocprofv3 --kernel-trace --stats -d DIR -o slide --output-format csv -- python scripts/bench_slide_match.py --calls-only 20
       python scripts/bench_slide_match.py [--rows 250000] [--targets 50000] [--reps 9] [--kernel-stats DIR] [--out profiles/slide_match.txt]"""
import argparse
import ctypes as C
import time

import harness
import torch

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.stats import match_slide

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=250000)
ap.add_argument("--targets", type=int, default=50000)
ap.add_argument("--side", type=float, default=70000.0, help="side of the square slide in pixels")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--calls-only", type=int, default=0, help="issue that many calls at K = 3 and leave (for a kernel trace)")
ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --calls-only")
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say

L = _lib.lib()
dev = torch.device("cuda:0")
M, T = a.rows, a.targets
rows_h, targets_h = harness.slide_rows(M, T, a.side)
rows, targets = torch.from_numpy(rows_h).to(dev), torch.from_numpy(targets_h).to(dev)
KMAX = 3
tp = torch.empty(KMAX, M, device=dev, dtype=torch.uint8)
best_iou, best_target = torch.empty(M, device=dev), torch.empty(M, device=dev, dtype=torch.int32)
claim = torch.empty(KMAX, T, device=dev, dtype=torch.int32)
row_ign, tgt_ign = torch.empty(M, device=dev, dtype=torch.uint8), torch.empty(T, device=dev, dtype=torch.uint8)
stats = torch.empty(2 * KMAX + 2, device=dev, dtype=torch.int32)
ws = torch.empty(L.ay_slide_match_workspace_bytes(M, T, KMAX), device=dev, dtype=torch.uint8)


def call(thres, roi, cell_side):
    thr = (C.c_float * len(thres))(*thres)
    roi_c = None if roi is None else (C.c_float * 4)(*roi)
    check(L.ay_slide_match(ptr(rows), M, ptr(targets), T, thr, len(thres), roi_c, C.c_float(cell_side), ptr(tp), ptr(best_iou),
                           ptr(best_target), ptr(claim), ptr(row_ign), ptr(tgt_ign), ptr(stats), ptr(ws), ws.numel(), _lib.stream_ptr()),
          "ay_slide_match")


if a.calls_only:
    harness.calls_only(a.calls_only, lambda: call([0.3, 0.5, 0.75], None, 0.0))

say(f"# ay_slide_match on {torch.cuda.get_device_name(0)}: {M} rows against {T} targets of 8..47 px on a {a.side:.0f}-px square; "
    f"CALL time = {a.reps} x (two events around one call, after {a.warm} warm calls), median [min, max]; it holds the call's host read "
    f"of the grid and its memsets, and is no sum of kernel times")
half = (0.25 * a.side, 0.25 * a.side, 0.75 * a.side, 0.75 * a.side)
cases = [("K=1 (0.5)", [0.5], None, 0.0), ("K=3 (0.3, 0.5, 0.75)", [0.3, 0.5, 0.75], None, 0.0), ("K=3, roi = the middle quarter", [0.3, 0.5, 0.75], half, 0.0),
         ("K=3, cell side 1024", [0.3, 0.5, 0.75], None, 1024.0), ("K=3, cell side 8192", [0.3, 0.5, 0.75], None, 8192.0)]
ref_bytes = None
for name, thres, roi, side in cases:
    ms = harness.time_calls([lambda: call(thres, roi, side)], a.warm, a.reps)[0]
    st = stats.cpu().numpy()
    K = len(thres)
    say(f"call, {name:38s} {harness.fmt_square(ms)}   eligible / claimed per k: "
        f"{[(int(st[2 * k]), int(st[2 * k + 1])) for k in range(K)]}, oversize targets {int(st[2 * K + 1])}")
    if K == 3 and roi is None:   # the cell side must not show in the result
        b = tp.cpu().numpy().tobytes() + claim.cpu().numpy().tobytes() + best_target.cpu().numpy().tobytes() + best_iou.cpu().numpy().tobytes()
        ref_bytes = ref_bytes or b
        say(f"{'':44s} same bytes as at the data's own cell side: {b == ref_bytes}")
wall = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    match_slide(rows_h, targets_h, [0.3, 0.5, 0.75])
    torch.cuda.synchronize()
    wall.append((time.perf_counter() - t0) * 1e3)
say(f"stats.match_slide from host arrays, wall: {min(wall):.2f} ms (best of 3; upload of {rows_h.nbytes / 1e6:.1f} + {targets_h.nbytes / 1e6:.1f} MB, "
    f"allocation, call, counts back)")
if a.kernel_stats:
    ours, calls = harness.kernel_table(a.kernel_stats, ["slide_", "grid_"])   # (the reduction and the scan are ay_box_grid.h's)
    say(f"# KERNEL time per call at K=3, from a kernel trace of {calls} calls (mean per dispatch):")
    harness.say_kernel_table(say, ours, calls, "sum of the six kernels")
    say("# for scale: ay_seam_merge takes 0.95 ms of kernels on its 258 633 rows of such boxes (profiles/seam_*.txt)")
report.write(a.out)
