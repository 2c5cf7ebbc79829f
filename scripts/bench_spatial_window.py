"""What the tissue-shaped window costs: ay_pair_counts_window against ay_pair_counts in the same process, on the slide of
scripts/bench_spatial.py (harness.clustered_rows: 200 k clustered detection rows of two classes on a 70 000-px square, B = 16 radii),
inputs, outputs, mask and workspace resident on the device.
MASK: a tissue-like blob (an ellipse with a wavy outline and 40 round holes, about half of the slide) on cells of 128 px (547 x 547
cells, what quantify_region's default cell gives) and of 16 px (4 375 x 4 375 = 19.1 M cells, the finest the call takes).
CALL time: after WARM warm calls of both, REPS times and ALTERNATING between the two calls, two device events around CALLS calls of
one entry point (kernel launches only); the time per call; median [min, max] over the REPS, and the ratio of the medians.
KERNEL time: each kernel apart, from a rocprofv3 kernel trace of `--calls-only N --r-max R --mask-cell C`, read back with
`--kernel-stats DIR` (once per traced configuration).
usage: rocprofv3 --kernel-trace --stats -d DIR -o w --output-format csv -- python scripts/bench_spatial_window.py --calls-only 20 --r-max 256 --mask-cell 128
       python scripts/bench_spatial_window.py [--reps 9] [--kernel-stats DIR:LABEL ...] [--out profiles/spatial_window.txt]"""
import argparse
import ctypes as C
import statistics

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--side", type=int, default=70000, help="side of the square slide in pixels")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--calls", type=int, default=20, help="calls between the two events of one repetition")
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--r-max", type=int, default=256, help="r_max in pixels of --calls-only")
ap.add_argument("--mask-cell", type=int, default=128, help="mask cell in pixels of --calls-only; 0: the plain call")
ap.add_argument("--calls-only", type=int, default=0, help="issue that many calls at --r-max / --mask-cell and leave (for a kernel trace)")
ap.add_argument("--kernel-stats", action="append", default=[], help="DIR:LABEL of a rocprofv3 --kernel-trace --stats run of --calls-only")
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say


def blob_mask(side, cell, seed=3, holes=40):
    """uint8 [G, G]: an ellipse with a wavy outline around the slide's middle, less `holes` round holes; the same shape at every cell"""
    G = -(-side // cell)
    rng = np.random.default_rng(seed)
    c = (np.arange(G, dtype=np.float32) + 0.5) * (cell / side)                      # cell centres in 0 .. 1
    y, x = c[:, None], c[None, :]
    ang = np.arctan2(y - 0.5, x - 0.5)
    rad = 1.0 + 0.12 * np.sin(3 * ang + rng.uniform(0, 6)) + 0.08 * np.sin(7 * ang + rng.uniform(0, 6))
    m = ((y - 0.5) / 0.40) ** 2 + ((x - 0.5) / 0.44) ** 2 <= rad ** 2
    for _ in range(holes):
        hy, hx, hr = rng.uniform(0.15, 0.85), rng.uniform(0.15, 0.85), rng.uniform(0.01, 0.04)
        m &= (y - hy) ** 2 + (x - hx) ** 2 > hr ** 2
    return np.ascontiguousarray(m, np.uint8)


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
masks = {}


def mask_of(cell):
    if cell not in masks:
        masks[cell] = torch.from_numpy(blob_mask(side, cell)).to(dev)
    return masks[cell]


def radii(r_max_px):
    return np.ascontiguousarray([4 * r_max_px * (k + 1) // B for k in range(B)], np.int32)


def caller(r_max_px, cell):
    """-> a function that issues one call: the plain one for cell == 0, else the window call on the mask of that cell"""
    rq = radii(r_max_px)
    if cell:
        ws = torch.empty(int(L.ay_pair_counts_window_workspace_bytes(M, side, side, int(rq[-1]), 0, cell)), device=dev, dtype=torch.uint8)
        mask = mask_of(cell)
        return lambda: check(L.ay_pair_counts_window(ptr(rows), M, NC, side, side, C.c_float(0.0), rq.ctypes.data_as(I32P), B, None, 1, 0, ptr(mask), cell,
                                                     ptr(pairs), ptr(centres), ptr(nn), ptr(bd), ptr(stats), ptr(ws), ws.numel(), _lib.stream_ptr()),
                             "ay_pair_counts_window")
    ws = torch.empty(int(L.ay_pair_counts_workspace_bytes(M, side, side, int(rq[-1]), 0)), device=dev, dtype=torch.uint8)
    return lambda: check(L.ay_pair_counts(ptr(rows), M, NC, side, side, C.c_float(0.0), rq.ctypes.data_as(I32P), B, None, 1, 0, ptr(pairs), ptr(centres),
                                          ptr(nn), ptr(bd), ptr(stats), ptr(ws), ws.numel(), _lib.stream_ptr()), "ay_pair_counts")


if a.calls_only:
    harness.calls_only(a.calls_only, caller(a.r_max, a.mask_cell))

say(f"# ay_pair_counts_window against ay_pair_counts on {torch.cuda.get_device_name(0)}: {M} clustered rows, C = {NC}, B = {B}, on a {side}-px square; "
    f"CALL time = {a.reps} x (two events around {a.calls} calls, per call), the calls alternating, after {a.warm} warm calls of each; median [min, max]")
for cell in (128, 16):
    m = mask_of(cell)
    say(f"# mask on {cell}-px cells: {m.shape[0]} x {m.shape[1]} = {m.numel()} cells, {float(m.float().mean()):.3f} IN; "
        f"window workspace {int(L.ay_pair_counts_window_workspace_bytes(M, side, side, 1024, 0, cell)) / 2 ** 20:.1f} MiB against "
        f"{int(L.ay_pair_counts_workspace_bytes(M, side, side, 1024, 0)) / 2 ** 20:.1f} MiB")
for r_max, cells in ((256, (128, 16)), (1024, (128, 16))):
    fns = [caller(r_max, 0)] + [caller(r_max, c) for c in cells]
    harness.time_calls(fns, a.warm, 0)                                  # WARM warm calls of each
    res = harness.time_calls(fns, 0, a.reps, per=a.calls)               # REPS times CALLS calls of each, taking turns
    caller(r_max, 0)()
    plain_centres = centres.cpu().numpy().copy()
    say(f"call, r_max {r_max:4d} px, plain              {harness.fmt_square(res[0])}   eligible centres at r_max {plain_centres[:, -1].sum()}")
    for c, r in zip(cells, res[1:]):
        caller(r_max, c)()
        n_in, n_el = int(stats[NC:2 * NC].sum().item()), int(centres[:, -1].sum().item())
        say(f"call, r_max {r_max:4d} px, mask on {c:3d}-px cells {harness.fmt_square(r)}   {statistics.median(r) / statistics.median(res[0]):.3f} x the plain call; "
            f"rows in IN cells {n_in}, eligible centres at r_max {n_el}")
for item in a.kernel_stats:
    d, label = item.split(":", 1)
    ours, calls = harness.kernel_table(d, ["pair_", "grid_"])
    say(f"# KERNEL time per call, {label}, from a kernel trace of {calls} calls (mean per dispatch):")
    harness.say_kernel_table(say, ours, calls, "sum of the kernels")
report.write(a.out)
