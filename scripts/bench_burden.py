"""Time of the slide-level burden calls (ay_burden_bin, ay_field_select) on the synthetic slide of scripts/bench_slide_match.py
(harness.slide_rows, the class modulo 2): about 250 k detection rows of 8..47-px boxes on a 70 000-px square, C = 2 classes, cell = 128 px (a 547 x 547 map), field = 8 cells, top_k =
5, inputs, outputs and workspace resident on the device.  The tissue plane is a disc of full cells (cell^2 pixels each) that covers
the middle of the slide, need_tissue = half a field.
CALL time: after WARM warm calls, REPS times, two device events around the call(s); both calls are kernel launches only, so this is
launch overhead plus kernels; min .. max (and the median) of the REPS are reported for ay_burden_bin, ay_field_select and the two
together.  The binning is also timed with every row in ONE cell: all atomics of a class on one word, the worst case of a dense slide.
KERNEL time: per kernel from a rocprofv3 kernel trace of `--calls-only N` (N times both calls, nothing else), read back with
`--kernel-stats DIR`; that figure is the one to hold against ay_slide_match's 0.254 ms and the seam merge's 0.95 ms of kernels.
usage: rocprofv3 --kernel-trace --stats -d DIR -o burden --output-format csv -- python scripts/bench_burden.py --calls-only 20
       python scripts/bench_burden.py [--rows 250000] [--reps 9] [--kernel-stats DIR] [--out profiles/burden.txt]"""
import argparse
import ctypes as C
import math
import statistics

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=250000)
ap.add_argument("--side", type=int, default=70000, help="side of the square slide in pixels")
ap.add_argument("--cell", type=int, default=128)
ap.add_argument("--field", type=int, default=8)
ap.add_argument("--top-k", type=int, default=5)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--calls-only", type=int, default=0, help="issue both calls that many times and leave (for a kernel trace)")
ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --calls-only")
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say

L = _lib.lib()
dev = torch.device("cuda:0")
M, NC, cell, F, K, side = a.rows, 2, a.cell, a.field, a.top_k, a.side
gy = gx = -(-side // cell)
rows_h = harness.slide_rows(M, 50000, side)[0]
rows_h[:, 6] %= 2                    # C = 2: the object's class modulo 2
one_cell_h = rows_h.copy()          # the same boxes, every centre moved into the cell in the middle of the map
centre = (rows_h[:, 0:2] + rows_h[:, 2:4]) / 2
target = (np.array([gx // 2, gy // 2], np.float32) + 0.5) * cell
one_cell_h[:, 0:2] += target - centre
one_cell_h[:, 2:4] += target - centre
rows, one_cell = torch.from_numpy(rows_h).to(dev), torch.from_numpy(one_cell_h).to(dev)
yy, xx = np.mgrid[0:gy, 0:gx]
tissue_h = (((yy - gy / 2) ** 2 + (xx - gx / 2) ** 2 < (0.45 * gx) ** 2) * cell * cell).astype(np.int32)
tissue = torch.from_numpy(tissue_h).to(dev)
need = max(1, math.ceil(0.5 * (F * cell) ** 2))
counts = torch.empty(NC, gy, gx, device=dev, dtype=torch.int32)
stats = torch.empty(NC + 3, device=dev, dtype=torch.int32)
fields = torch.empty(NC, K, 4, device=dev, dtype=torch.int32)
n_found = torch.empty(NC, device=dev, dtype=torch.int32)
ws = torch.empty(int(L.ay_field_select_workspace_bytes(NC, gy, gx, F)), device=dev, dtype=torch.uint8)


def bin_(r=rows):
    check(L.ay_burden_bin(ptr(r), M, NC, side, side, cell, C.c_float(0.5), ptr(counts), ptr(stats), _lib.stream_ptr()), "ay_burden_bin")


def select():
    check(L.ay_field_select(ptr(counts), NC, gy, gx, ptr(tissue), F, need, K, ptr(fields), ptr(n_found), ptr(ws), ws.numel(), _lib.stream_ptr()),
          "ay_field_select")


def both():
    bin_()
    select()


if a.calls_only:
    harness.calls_only(a.calls_only, both)


def timed(fn):
    ms = harness.time_calls([fn], a.warm, a.reps)[0]
    return f"{min(ms):8.3f} .. {max(ms):.3f} ms (median {statistics.median(ms):.3f})"


say(f"# ay_burden_bin / ay_field_select on {torch.cuda.get_device_name(0)}: {M} rows of 8..47-px boxes on a {side}-px square, C = {NC}, "
    f"cell = {cell} ({gy} x {gx} cells), field = {F}, top_k = {K}, need_tissue = {need}; CALL time = min .. max of {a.reps} x (two events "
    f"around the call, after {a.warm} warm calls): launch overhead and kernels")
say(f"ay_burden_bin (zero + one lane per row, wave-merged adds) {timed(bin_)}")
st = stats.cpu().numpy()
say(f"    counted per class {st[:NC].tolist()}, below {int(st[NC])}, flagged {int(st[NC + 1])}; fullest cell {int(counts.max())} rows")
say(f"ay_burden_bin, every row in ONE cell                      {timed(lambda: bin_(one_cell))}")
say(f"    fullest cell {int(counts.max())} rows")
bin_()
say(f"ay_field_select (row pass, column pass, selection)        {timed(select)}")
say(f"    n_found {n_found.cpu().tolist()}, picks (fy, fx, n, t) of class 0: {fields[0].cpu().tolist()}")
say(f"both calls                                                {timed(both)}")
if a.kernel_stats:
    ours, _ = harness.kernel_table(a.kernel_stats, ["burden_"])
    _, calls = harness.kernel_table(a.kernel_stats, ["burden_select"])     # one selection kernel per call of both
    say(f"# KERNEL time per call of both, from a kernel trace of {calls} calls (total per call; the column pass runs twice, the tissue plane first):")
    harness.say_kernel_table(say, ours, calls, "sum of the six launches")
    say("# for scale: ay_slide_match takes 0.254 ms and ay_seam_merge 0.95 ms of kernels on slides of this size (DESIGN.md section 8)")
report.write(a.out)
