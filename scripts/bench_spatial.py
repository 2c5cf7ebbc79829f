"""Time of one spatial-statistics call (ay_pair_counts, wsi.spatial_stats) on a synthetic slide: 200 k clustered detection rows of
two classes on a 70 000-px square (2 000 parents, offspring sigma 150 px, a quarter of the rows uniform), inputs, outputs and
workspace resident on the device.
CALL time: after WARM warm calls, REPS times, two device events around ONE call of the C entry point (seven kernel launches, nothing
else); the median of the REPS is reported with min and max, at r_max = 64, 256 and 1024 px with B = 16 radii and C = 2.
PAIR TESTS: the partners a call visits = for every counted row, the counted rows in the 3 x 3 grid cells around its own, counted
on the host from the grid the call states (S = R_max * 2^m quarter pixels, at most 2 max(n, 2048) cells); pair tests per second =
that number over the call time.  WITHIN: the partners that lie within r_max (the last column of `pairs` without the border rule),
each of which costs a bin search, an LDS add and an LDS minimum on top of the test.
WHAT BOUNDS IT: two more calls per r_max through the arguments alone -- the same radii on cells four times as wide (16 times the
partners visited, the same partners within: the cost of a visit that fails the radius test), and, at the call's own cells, ONE
radius r_max in place of the 16 (the same visits and the same partners within, every add on one bin per class: the cost of LDS
atomic conflicts).
In the same run ay_slide_match with those rows as both rows and targets, the sibling search on the same grid header (its call time
holds a host read and memsets; see scripts/bench_slide_match.py).
KERNEL time: the kernels of a call from a rocprofv3 kernel trace of `--calls-only N --r-max R`, read back with `--kernel-stats DIR`.
usage: rocprofv3 --kernel-trace --stats -d DIR -o spatial --output-format csv -- python scripts/bench_spatial.py --calls-only 20 --r-max 256
       python scripts/bench_spatial.py [--rows 200000] [--reps 9] [--kernel-stats DIR] [--out profiles/spatial.txt]"""
import argparse
import ctypes as C
import statistics
import time

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import spatial_stats

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--side", type=int, default=70000, help="side of the square slide in pixels")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--r-max", type=int, default=256, help="r_max in pixels of --calls-only")
ap.add_argument("--calls-only", type=int, default=0, help="issue that many calls at --r-max and leave (for a kernel trace)")
ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of --calls-only")
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say


def visits(rows_h, side, r_max_q, cell_side_q):
    """partners visited by a call: the grid as include/amyloid_yolo.h states it, the 3 x 3 cell sums on the host"""
    S = cell_side_q or r_max_q
    cap = 2 * max(len(rows_h), 2048)
    while not cell_side_q and (-(-4 * side // S)) ** 2 > cap:
        S *= 2
    g = -(-4 * side // S)
    c = (rows_h[:, 0:2] + rows_h[:, 2:4]) * np.float32(0.5)
    q = np.floor(np.clip(c * np.float32(4), 0, 4 * side - 1)).astype(np.int64) // S
    cnt = np.zeros((g + 2, g + 2), np.int64)
    np.add.at(cnt, (q[:, 1] + 1, q[:, 0] + 1), 1)
    box = sum(cnt[1 + dy:g + 1 + dy, 1 + dx:g + 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    return int((box * cnt[1:-1, 1:-1]).sum() - len(rows_h)), S, g


L = _lib.lib()
dev = torch.device("cuda:0")
M, side, NC, B = a.rows, a.side, 2, 16
rows_h = harness.clustered_rows(M, side)
rows = torch.from_numpy(rows_h).to(dev)
pairs = torch.empty(NC, NC, B, device=dev, dtype=torch.int64)
centres = torch.empty(NC, B, device=dev, dtype=torch.int32)
nn, bd = torch.empty(M, NC, 2, device=dev, dtype=torch.int32), torch.empty(M, device=dev, dtype=torch.int32)
stats = torch.empty(2 * NC + 3, device=dev, dtype=torch.int32)
I32P = C.POINTER(C.c_int32)


def call(radii_q, border, cell_side_q, ws):
    rq = np.ascontiguousarray(radii_q, np.int32)
    check(L.ay_pair_counts(ptr(rows), M, NC, side, side, C.c_float(0.0), rq.ctypes.data_as(I32P), len(rq), None, border, cell_side_q, ptr(pairs),
                           ptr(centres), ptr(nn), ptr(bd), ptr(stats), ptr(ws), ws.numel(), _lib.stream_ptr()), "ay_pair_counts")


def workspace(r_max_q, cell_side_q):
    return torch.empty(int(L.ay_pair_counts_workspace_bytes(M, side, side, r_max_q, cell_side_q)), device=dev, dtype=torch.uint8)


def radii(r_max_px):
    return [4 * r_max_px * (k + 1) // B for k in range(B)]


if a.calls_only:
    ws = workspace(4 * a.r_max, 0)
    harness.calls_only(a.calls_only, lambda: call(radii(a.r_max), 1, 0, ws))

say(f"# ay_pair_counts on {torch.cuda.get_device_name(0)}: {M} clustered rows, C = {NC}, B = {B}, on a {side}-px square; CALL time = {a.reps} x "
    f"(two events around one call, after {a.warm} warm calls), median [min, max]; a call is seven kernel launches")
for r_max in (64, 256, 1024):
    rq = radii(r_max)
    for name, rr, cs in ((f"r_max {r_max:4d} px", rq, 0), ("  cells 4 x as wide", rq, None), ("  one radius (B = 1)", rq[-1:], 0)):
        n_vis, S, g = visits(rows_h, side, rq[-1], 0)
        if cs is None:
            cs = 4 * S
            n_vis, S, g = visits(rows_h, side, rq[-1], cs)
        ws = workspace(rq[-1], cs)
        call(rr, 0, cs, ws)
        within = int(pairs.view(-1)[:NC * NC * len(rr)].view(NC, NC, len(rr))[:, :, -1].sum().item())
        ms = harness.time_calls([lambda: call(rr, 1, cs, ws)], a.warm, a.reps)[0]
        med = statistics.median(ms)
        say(f"call, {name:20s} {harness.fmt_square(ms)}   cells {S / 4:g} px ({g} x {g}), partners visited {n_vis:.4g} "
            f"({n_vis / (med * 1e-3):.3g} pair tests/s), within r_max {within:.4g} ({within / (med * 1e-3):.3g} /s)")

# the sibling search on the same grid header: every row against every row as a target
targets = torch.cat([rows[:, 6:7], rows[:, 0:4]], 1).contiguous()
tp = torch.empty(1, M, device=dev, dtype=torch.uint8)
best_iou, best_target = torch.empty(M, device=dev), torch.empty(M, device=dev, dtype=torch.int32)
claim = torch.empty(1, M, device=dev, dtype=torch.int32)
row_ign, tgt_ign = torch.empty(M, device=dev, dtype=torch.uint8), torch.empty(M, device=dev, dtype=torch.uint8)
mstats = torch.empty(4, device=dev, dtype=torch.int32)
mws = torch.empty(L.ay_slide_match_workspace_bytes(M, M, 1), device=dev, dtype=torch.uint8)
thr = (C.c_float * 1)(0.5)


def match():
    check(L.ay_slide_match(ptr(rows), M, ptr(targets), M, thr, 1, None, C.c_float(0.0), ptr(tp), ptr(best_iou), ptr(best_target), ptr(claim),
                           ptr(row_ign), ptr(tgt_ign), ptr(mstats), ptr(mws), mws.numel(), _lib.stream_ptr()), "ay_slide_match")


ms = harness.time_calls([match], a.warm, a.reps)[0]
say(f"call, ay_slide_match, the rows as rows and targets, K = 1: {harness.fmt_square(ms)}   (holds a host read and memsets)")
wall = []
for _ in range(3):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    spatial_stats(rows_h, (side, side), [r / 4 for r in radii(256)], NC)
    wall.append((time.perf_counter() - t0) * 1e3)
say(f"wsi.spatial_stats from host rows at r_max 256 px, wall: {min(wall):.2f} ms (best of 3; upload of {rows_h.nbytes / 1e6:.1f} MB, allocation, "
    f"call, one read-back of {(M * (2 * NC + 2) * 4) / 1e6:.1f} MB, K / L / g / G on the host)")
if a.kernel_stats:
    ours, calls = harness.kernel_table(a.kernel_stats, ["pair_", "grid_"])
    say(f"# KERNEL time per call at r_max {a.r_max} px, from a kernel trace of {calls} calls (mean per dispatch):")
    harness.say_kernel_table(say, ours, calls, "sum of the seven kernels")
report.write(a.out)
