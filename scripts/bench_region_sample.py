"""Cost of cutting training windows out of a slide (ay_augment_ingest_window_u8, wsi.SlideSampler) next to the tile augmentation it
extends, at the training shape: B windows of TILE^2 uint8 -> B x 3 x S^2 fp32, every operation on (the default ranges).
In one process, alternating inside every repeat:
  (a) ay_augment_ingest_u8 on B resident tiles -- this tree, and with --parent_lib the library of the parent commit on the same batch
  (b) ay_augment_ingest_window_u8, context 0, the same tiles as blocks (bit-identical output, checked)
  (c) ay_augment_ingest_window_u8, context 1, the same records on windows of a resident RASTER^2 raster (block = the raster)
each timed between two device events around CALLS launches after a warm call, REPS times: median [min, max].  The spread of (a)
over the repeats, and between the two libraries, is what a difference has to exceed to mean anything.
  (d) the host side of a SlideSampler batch on a host raster of the same size: planning (draws, footprints, labels), the staging
      copy of footprint ∩ block into the pinned buffer, the bytes staged, and the upload of that buffer; wall clock, --host_reps
      batches after two warm ones.  It depends on the box's CPUs and on who else uses them.
--step_ms: the training step at the same B and size (bench.py --mode train --train_batch B --train_size S, same box, same visit)
that (d) is held against: one batch staged ahead hides the host side only if it is shorter than the step.
usage: python scripts/bench_region_sample.py [--batch 32] [--tile 1536] [--size 1024] [--raster 8192] [--parent_lib PATH]
                                             [--step_ms MS] [--out profiles/region_sample.txt]"""
import argparse
import ctypes as C
import os
import statistics
import time

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib, augment as ag
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import SlideSampler

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--tile", type=int, default=1536)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--raster", type=int, default=8192)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--host_reps", type=int, default=6)
ap.add_argument("--parent_lib", default=None)
ap.add_argument("--step_ms", type=float, default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say

L = _lib.lib()
dev = torch.device("cuda:0")
B, T, S, R = a.batch, a.tile, a.size, a.raster
sp = _lib.stream_ptr
base = harness.synthetic_tiles(T)
tiles = torch.from_numpy(np.ascontiguousarray(np.stack([base[i % 4] for i in range(B)]))).to(dev)
table = ag.sample_params(np.random.default_rng(0), [(T, T)] * B)
up = lambda recs: torch.from_numpy(recs.view(np.uint8).reshape(-1).copy()).to(dev)
d_tile = up(table.dev)
d_win0 = up(ag.make_window_table(table, [(T, T)] * B, [(0, 0)] * B, context=False).dev)
# the raster: the four synthetic tiles repeated over R x R, on the host (for d) and resident (for c)
n = -(-R // T)
raster_host = np.ascontiguousarray(np.concatenate([np.concatenate([base[(i + j) % 4] for j in range(n)], 1) for i in range(n)], 0)[:R, :R])
raster = torch.from_numpy(raster_host).to(dev)
rng = np.random.default_rng(1)
origins = [(int(rng.integers(0, R - T + 1)), int(rng.integers(0, R - T + 1))) for _ in range(B)]
d_win1 = up(ag.make_window_table(table, [(R, R)] * B, origins, context=True, src_offsets=[0] * B).dev)
out, out_b = torch.empty(B, 3, S, S, device=dev), torch.empty(B, 3, S, S, device=dev)

runs = {"(a) ay_augment_ingest_u8, this tree": lambda: check(L.ay_augment_ingest_u8(ptr(tiles), tiles.numel(), ptr(d_tile), B, S, ptr(out), sp()))}
if a.parent_lib:
    P = C.CDLL(os.path.abspath(a.parent_lib))
    P.ay_augment_ingest_u8.restype = C.c_int
    P.ay_augment_ingest_u8.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    out_p = torch.empty(B, 3, S, S, device=dev)
    runs["(a) ay_augment_ingest_u8, parent commit"] = lambda: check(P.ay_augment_ingest_u8(ptr(tiles), tiles.numel(), ptr(d_tile), B, S, ptr(out_p), sp()))
runs["(b) window kernel, context 0, same tiles"] = lambda: check(L.ay_augment_ingest_window_u8(ptr(tiles), tiles.numel(), ptr(d_win0), B, S, ptr(out_b), sp()))
runs["(c) window kernel, context 1, resident raster"] = lambda: check(L.ay_augment_ingest_window_u8(ptr(raster), raster.numel(), ptr(d_win1), B, S, ptr(out_b), sp()))

say(f"# region sampling on {torch.cuda.get_device_name(0)}: B={B}, {T}^2 windows -> {S}^2 fp32, default ranges; raster {R}^2; "
    f"{a.reps} x ({a.calls} calls between two events after a warm call), median [min, max]")
times = dict(zip(runs, harness.time_calls(list(runs.values()), 0, a.reps, per=a.calls, lead=1)))     # all of them alternate inside every repeat
med = {k: statistics.median(v) for k, v in times.items()}
ref = med["(a) ay_augment_ingest_u8, this tree"]
for name, v in times.items():
    say(f"{name:48s} {harness.fmt_square(v, us=True)}   {med[name] / ref:.3f} x (a)")
list(runs.values())[0]()
runs["(b) window kernel, context 0, same tiles"]()
torch.cuda.synchronize()
say(f"(b) == (a), bitwise: {torch.equal(out, out_b)}")
if a.parent_lib:
    say(f"(a) parent == (a) this tree, bitwise: {torch.equal(out, out_p)}")

# (d) the host side of a batch
targets = np.array([[0, x, y, x + 60, y + 60] for x in range(100, R - 100, 400) for y in range(100, R - 100, 400)], np.float64)
s = SlideSampler([(raster_host, targets)], tile=T, img_size=S, batch_size=B, batches=1, seed=0,
                 tile_mask=np.ones((n, n), bool))
from concurrent.futures import ThreadPoolExecutor
pool = ThreadPoolExecutor(max_workers=4)     # the sampler's staging pool has as many threads
pinned = resident = None
t_plan, t_stage, t_up, nbytes = [], [], [], []
rep = 0
while len(nbytes) < a.host_reps:
    t0 = time.perf_counter()
    plan = s.plan_batch()
    wt = s.window_table(plan)
    t1 = time.perf_counter()
    need = s.staged_bytes(plan)
    grown = pinned is None or pinned.numel() < need
    if grown:
        pinned = torch.empty(need * 5 // 4, dtype=torch.uint8).pin_memory()
        resident = torch.empty(pinned.numel(), dtype=torch.uint8, device=dev)
    t2 = time.perf_counter()
    s.stage(plan, wt, pinned.numpy(), pool)
    t3 = time.perf_counter()
    torch.cuda.synchronize()
    t4 = time.perf_counter()
    resident[:need].copy_(pinned[:need], non_blocking=True)
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    rep += 1
    if rep > 2 and not grown:        # two warm batches; a batch that had to grow the buffers touches fresh pages
        t_plan.append(1e3 * (t1 - t0)); t_stage.append(1e3 * (t3 - t2)); t_up.append(1e3 * (t5 - t4)); nbytes.append(need)
    assert rep < 4 * a.host_reps + 8
m = statistics.median
say(f"(d) host raster {R}^2, per batch of {B} ({a.host_reps} batches after 2 warm ones, medians): plan {m(t_plan):.1f} ms, staging copy "
    f"{m(t_stage):.1f} ms [{min(t_stage):.1f}, {max(t_stage):.1f}] for {m(nbytes) / 1e6:.0f} MB (footprint ∩ block; the windows alone are "
    f"{B * T * T * 3 / 1e6:.0f} MB) = {m(nbytes) / m(t_stage) / 1e6:.1f} GB/s, upload {m(t_up):.1f} ms")
host = m(t_plan) + m(t_stage)
if a.step_ms:
    say(f"host side {host:.1f} ms (plan + staging) against the {a.step_ms:.1f} ms training step at B={B}, {S}^2: "
        f"{'hidden behind the step by staging one batch ahead' if host < a.step_ms else 'NOT hidden: the host side is longer than the step'}; "
        f"(c) is {100 * med['(c) window kernel, context 1, resident raster'] / a.step_ms:.2f} % of the step")
report.write(a.out)
