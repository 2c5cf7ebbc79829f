"""What the tissue-shaped window costs: ay_pair_counts_window against ay_pair_counts in the same process, on the slide of
scripts/bench_spatial.py (200 k clustered detection rows of two classes on a 70 000-px square, B = 16 radii), inputs, outputs, mask
and workspace resident on the device.
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
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
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

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def synthetic_slide(M, side, seed=0):
    """the rows of scripts/bench_spatial.py"""
    rng = np.random.default_rng(seed)
    parents = rng.uniform(0, side, (2000, 2))
    xy = parents[rng.integers(0, 2000, M)] + rng.normal(0, 150.0, (M, 2))
    loose = rng.uniform(size=M) < 0.25
    xy[loose] = rng.uniform(0, side, (int(loose.sum()), 2))
    wh = rng.uniform(8, 60, (M, 2))
    return np.concatenate([xy - wh / 2, xy + wh / 2, rng.uniform(0.5, 1, (M, 2)), rng.integers(0, 2, (M, 1))], 1).astype(np.float32)


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
rows_h = synthetic_slide(M, side)
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


def timed_alternating(fns):
    """ms per call of every function: REPS repetitions of CALLS calls each, the functions taking turns"""
    for f in fns:
        for _ in range(a.warm):
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(a.reps):
        for k, f in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.calls)
    return [(statistics.median(m), min(m), max(m)) for m in ms]


if a.calls_only:
    f = caller(a.r_max, a.mask_cell)
    for _ in range(a.calls_only):
        f()
    torch.cuda.synchronize()
    sys.exit(0)

say(f"# ay_pair_counts_window against ay_pair_counts on {torch.cuda.get_device_name(0)}: {M} clustered rows, C = {NC}, B = {B}, on a {side}-px square; "
    f"CALL time = {a.reps} x (two events around {a.calls} calls, per call), the calls alternating, after {a.warm} warm calls of each; median [min, max]")
for cell in (128, 16):
    m = mask_of(cell)
    say(f"# mask on {cell}-px cells: {m.shape[0]} x {m.shape[1]} = {m.numel()} cells, {float(m.float().mean()):.3f} IN; "
        f"window workspace {int(L.ay_pair_counts_window_workspace_bytes(M, side, side, 1024, 0, cell)) / 2 ** 20:.1f} MiB against "
        f"{int(L.ay_pair_counts_workspace_bytes(M, side, side, 1024, 0)) / 2 ** 20:.1f} MiB")
for r_max, cells in ((256, (128, 16)), (1024, (128, 16))):
    res = timed_alternating([caller(r_max, 0)] + [caller(r_max, c) for c in cells])
    caller(r_max, 0)()
    plain_centres = centres.cpu().numpy().copy()
    say(f"call, r_max {r_max:4d} px, plain              {res[0][0]:8.3f} ms  [{res[0][1]:.3f}, {res[0][2]:.3f}]   eligible centres at r_max {plain_centres[:, -1].sum()}")
    for c, r in zip(cells, res[1:]):
        caller(r_max, c)()
        n_in, n_el = int(stats[NC:2 * NC].sum().item()), int(centres[:, -1].sum().item())
        say(f"call, r_max {r_max:4d} px, mask on {c:3d}-px cells {r[0]:8.3f} ms  [{r[1]:.3f}, {r[2]:.3f}]   {r[0] / res[0][0]:.3f} x the plain call; rows in IN cells "
            f"{n_in}, eligible centres at r_max {n_el}")
for item in a.kernel_stats:
    import csv
    import glob
    d, label = item.split(":", 1)
    table = list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*_kernel_stats.csv"), recursive=True)[0])))
    ours = [r for r in table if "pair_" in r["Name"] or "grid_" in r["Name"]]
    calls = max(int(r["Calls"]) for r in ours)
    say(f"# KERNEL time per call, {label}, from a kernel trace of {calls} calls (mean per dispatch):")
    for r in sorted(ours, key=lambda r: -float(r["TotalDurationNs"])):
        say(f"  {r['Name'].split('(')[0][:60]:60s} {float(r['TotalDurationNs']) / calls / 1e3:8.1f} us")
    say(f"  {'sum of the kernels':60s} {sum(float(r['TotalDurationNs']) for r in ours) / calls / 1e3:8.1f} us")
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
