"""Cost of the stain normalisation (THE STAIN RULE, include/amyloid_yolo.h) on the synthetic slide of scripts/bench_wsi.py: TY x TX
1536-px tiles in host memory, one process, three comparisons, each alternating its two sides inside one timed loop:
  1. CUT      ay_ingest_region_tiles_stain_u8 (views = {0}) against ay_ingest_region_tiles_list_u8 on one resident strip of TX tiles,
              1536 -> 1024: time per tile and GB/s of STORES (12 B per output pixel; the plain cut is bound by them).
  2. STATS    ay_stain_hist_u8 against ay_tile_tissue_u8 (one tile row) on the same strip: GB/s of READS (3 B per source pixel).
  3. DETECT   wsi.detect_region with and without stain= over the whole slide (upload, cut, model, NMS), wall clock.
CALL time: after WARM warm calls of both sides, REPS times, two device events around the call; median (min .. max).  Calls are
kernel launches only, so this is launch overhead plus kernel.  The synthetic tiles have a noisy background of U{180..255}: bg_level 170.
usage: python scripts/bench_stain.py [TY TX] [--reps 20] [--warm 3] [--detect-reps 3] [--out profiles/stain.txt]"""
import argparse
import ctypes as C
import statistics
import tempfile
import time

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib, cfg_gen, parse_config, synth
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.models import Darknet
from amyloid_yolo_paper_amd.wsi import StainMap, detect_region, stain_stats

ap = argparse.ArgumentParser()
ap.add_argument("grid", nargs="*", type=int, default=[2, 32])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warm", type=int, default=3)
ap.add_argument("--detect-reps", type=int, default=3)
ap.add_argument("--out", default=None)
a = ap.parse_args()
TY, TX = a.grid
tile, S, BG = 1536, 1024, 170
report = harness.Report()
say = report.say

dev = torch.device("cuda:0")
row = harness.synthetic_strip(TX, tile)
raster = np.concatenate([np.roll(row, 97 * j, 1) for j in range(TY)], 0)
say("raster %s, %.3f GB; tile %d -> %d; %d warm + %d timed calls per side" % (raster.shape, raster.nbytes / 1e9, tile, S, a.warm, a.reps))

stats = stain_stats(raster, bg_level=BG)
q = stats.strength()
stain = StainMap(stats, (1.3 * q[0], 0.7 * q[1]))
say("stain_stats (probe_stride 16): %d tissue pixels, strength %s, gains of the map %s" % (stats.n_tissue, q, stain.gains))
L, sp = _lib.lib(), _lib.stream_ptr()
strip = torch.from_numpy(raster[:tile]).to(dev)
H, W = strip.shape[:2]
origins = torch.tensor([(i * tile, 0) for i in range(TX)], dtype=torch.int32, device=dev)
out = torch.empty(TX, 3, S, S, device=dev)
ids = (C.c_int * 1)(0)
params = stain.params

# ---- 1. the cut ----
plain = lambda: check(L.ay_ingest_region_tiles_list_u8(ptr(strip), H, W, W * 3, 1, tile, ptr(origins), TX, S, ptr(out), sp), "list")
mapped = lambda: check(L.ay_ingest_region_tiles_stain_u8(ptr(strip), H, W, W * 3, 1, tile, ptr(origins), TX, ids, 1, ptr(params), S, ptr(out), sp), "stain")
t_plain, t_stain = harness.time_calls([plain, mapped], a.warm, a.reps)
stores = out.numel() * 4
for name, ms in (("plain list cut", t_plain), ("stain cut     ", t_stain)):
    m = statistics.median(ms)
    say("CUT    %s: %s per call of %d tiles = %.1f us per tile, %.0f GB/s of stores" % (name, harness.fmt_round(ms), TX, m * 1e3 / TX, stores / m / 1e6))
say("CUT    stain / plain = %.2f (medians)" % (statistics.median(t_stain) / statistics.median(t_plain)))

# ---- 2. the statistics ----
counts = torch.empty(TX, device=dev, dtype=torch.int32)
hist = torch.zeros(1025, device=dev, dtype=torch.int64)
tissue = lambda: check(L.ay_tile_tissue_u8(ptr(strip), H, W, W * 3, 1, tile, tile, 1, TX, BG, ptr(counts), sp), "tissue")
histo = lambda: check(L.ay_stain_hist_u8(ptr(strip), H, W, W * 3, 1, BG, ptr(params), ptr(hist), sp), "hist")
t_tissue, t_hist = harness.time_calls([tissue, histo], a.warm, a.reps)
reads = strip.numel()
for name, ms in (("ay_tile_tissue_u8", t_tissue), ("ay_stain_hist_u8 ", t_hist)):
    say("STATS  %s: %s per strip, %.0f GB/s of reads" % (name, harness.fmt_round(ms), reads / statistics.median(ms) / 1e6))
assert int(hist[1024]) == int(counts.sum()) * (a.warm + a.reps)       # the histogram accumulates; both count the same tissue
say("STATS  tissue pixels of the strip: %d of %d" % (int(counts.sum()), H * W))

# ---- 3. detect_region ----
cfg = cfg_gen.write_cfg(3, tempfile.mkdtemp())
m = Darknet(cfg, precision="bf16")
sd = m.state_dict()   # the calibrated synthetic weights of bench.py
for i, p in synth.synth_params(parse_config.parse_model_config(cfg), seed=7).items():
    for k, name in (("weight", f"conv_{i}.weight"), ("bias", f"conv_{i}.bias"), ("gamma", f"batch_norm_{i}.weight"),
                    ("beta", f"batch_norm_{i}.bias"), ("mean", f"batch_norm_{i}.running_mean"), ("var", f"batch_norm_{i}.running_var")):
        if k in p:
            sd[f"module_list.{i}.{name}"].copy_(torch.from_numpy(p[k]))
m = m.to(dev).eval()
wall = {None: [], stain: []}
rows = {}
for rep in range(1 + a.detect_reps):       # the first round warms both
    for st in (None, stain):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = detect_region(m, raster, tile, S, conf_thres=0.5, nms_thres=0.4, batch_size=TX, stain=st)
        torch.cuda.synchronize()
        if rep:
            wall[st].append(time.perf_counter() - t0)
        rows[st] = sum(len(d) for _, _, d in res)
for name, st in (("without stain", None), ("with stain   ", stain)):
    s = statistics.median(wall[st])
    say("DETECT %s: %.3f s (%.3f .. %.3f), %.1f tiles/s, %d rows" % (name, s, min(wall[st]), max(wall[st]), TY * TX / s, rows[st]))
say("DETECT with / without = %.3f (medians)" % (statistics.median(wall[stain]) / statistics.median(wall[None])))
report.write(a.out)
