"""Throughput of the WSI -> tile -> detection stream (§8f N4): a synthetic slide of TY x TX 1536-px tiles in host memory,
streamed strip by strip (pinned upload on a copy stream, device-side tiling + /255 + resize to 1024), model + merge-NMS.
usage: python scripts/bench_wsi.py [TY TX] [--overlap N] [--max-det D] [--reps R] [--blank F] [--min-tissue M] [--bg-level L]
[--probe-stride D] [--views V] [--min-views K] ; prints tiles/s including the PCIe upload (this is NOT bench.py's `value`).
--overlap N: tiles that share N pixels (more tiles over the same slide) + the slide-level seam merge.
--blank F: the last round(F * TX) tile columns and the last round(F * TY) tile rows of the slide are painted 255 (glass).
--min-tissue M (> 0): only tiles with that fraction of tissue pixels are read (wsi.tissue_mask on a --probe-stride probe, inside the
timed call); the script prints how many tiles are wanted and the bytes staged.  The synthetic tiles have a noisy background of
U{180..255} per channel, so runs on them use --bg-level 170 (the default 220 is for scanned glass), and a synthetic tile that drew
no blob is rightly unwanted.
--views V (1, 2, 4 or 8; default 1 = off): every tile runs in the first V dihedral views (wsi.detect_region(views=range(V)): 4 = the
flips, 8 = all); --min-views K keeps the detections at least K views agree on.  The report then counts images (tiles x V) as well,
and how many tiles leave the NMS LDS paths (more than 1 024 / 4 096 candidates, now that a tile holds V times the rows)."""
import sys, time
import harness
import numpy as np, torch
from amyloid_yolo_paper_amd import cfg_gen, synth
from amyloid_yolo_paper_amd.models import Darknet
from amyloid_yolo_paper_amd.wsi import RegionTileStream, detect_region
import tempfile

argv = sys.argv[1:]
opts = {"--overlap": 0, "--reps": 2, "--max-det": 4096, "--blank": 0.0, "--min-tissue": 0.0, "--bg-level": 220, "--probe-stride": 16, "--views": 1,
        "--min-views": 1}
for o in opts:
    if o in argv:
        k = argv.index(o)
        opts[o] = type(opts[o])(argv[k + 1])
        del argv[k:k + 2]
OVERLAP, REPS = opts["--overlap"], opts["--reps"]
TY, TX = (int(argv[0]), int(argv[1])) if len(argv) > 1 else (8, 32)
tile, S = 1536, 1024
dev = torch.device("cuda:0")
from amyloid_yolo_paper_amd import parse_config
cfg = cfg_gen.write_cfg(3, tempfile.mkdtemp())
m = Darknet(cfg, precision="bf16")
sd = m.state_dict()   # the calibrated synthetic weights of bench.py (random-init nets put every box at conf ~0.5: NMS-bound nonsense)
for i, p in synth.synth_params(parse_config.parse_model_config(cfg), seed=7).items():
    for k, name in (("weight", f"conv_{i}.weight"), ("bias", f"conv_{i}.bias"), ("gamma", f"batch_norm_{i}.weight"),
                    ("beta", f"batch_norm_{i}.bias"), ("mean", f"batch_norm_{i}.running_mean"), ("var", f"batch_norm_{i}.running_var")):
        if k in p:
            sd[f"module_list.{i}.{name}"].copy_(torch.from_numpy(p[k]))
m = m.to(dev).eval()
row = harness.synthetic_strip(TX, tile)
raster = np.concatenate([np.roll(row, 97 * j, 1) for j in range(TY)], 0)
if opts["--blank"] > 0:
    raster[:, (TX - round(opts["--blank"] * TX)) * tile:] = 255
    raster[(TY - round(opts["--blank"] * TY)) * tile:] = 255
print("raster", raster.shape, "%.2f GB" % (raster.nbytes / 1e9), flush=True)
if OVERLAP:   # the grid over the same slide with overlapping tiles
    from amyloid_yolo_paper_amd.wsi import tile_grid
    GY, GX, _ = tile_grid(raster.shape[0], raster.shape[1], tile, OVERLAP)
    kw = dict(overlap=OVERLAP)
    det_kw = dict(overlap=OVERLAP, max_det=opts["--max-det"])   # the synthetic tiles are dense: some overlapping tile passes 1 024 rows
else:
    GY, GX, kw, det_kw = TY, TX, {}, {}
if opts["--min-tissue"] > 0:   # the mask the timed call will compute, for the report and the ingest-only loop
    from amyloid_yolo_paper_amd.wsi import tissue_mask
    t0 = time.perf_counter()
    mask = tissue_mask(raster, tile, 1, OVERLAP, opts["--min-tissue"], opts["--bg-level"], opts["--probe-stride"])
    t1 = time.perf_counter()
    kw = dict(kw, tile_mask=mask)
    det_kw = dict(det_kw, min_tissue=opts["--min-tissue"], bg_level=opts["--bg-level"], probe_stride=opts["--probe-stride"])
    probe = RegionTileStream(raster, tile, S, **kw)
    print("tissue mask: %d of %d tiles wanted in %d of %d strips, %.3f GB of %.3f GB staged, probe %.3f s (first call)"
          % (mask.sum(), mask.size, len(probe), GY, probe._staged_bytes() / 1e9, raster.nbytes / 1e9, t1 - t0), flush=True)
    del probe
VIEWS = tuple(range(opts["--views"]))
if VIEWS != (0,) or opts["--min-views"] != 1:
    assert len(VIEWS) in (1, 2, 4, 8)
    kw = dict(kw, views=VIEWS)
    det_kw = dict(det_kw, views=VIEWS, min_views=opts["--min-views"], max_det=opts["--max-det"])
    from amyloid_yolo_paper_amd import utils
    cands, real_nms = [], utils.nms_device
    def counting_nms(pred, *a, **k):     # cand_count of every NMS call, read after the timed region
        out = real_nms(pred, *a, **k)
        cands.append(out[3].clone())
        return out
    utils.nms_device = counting_nms
for rep in range(REPS):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    n = 0
    for tiles, cs in RegionTileStream(raster, tile, S, **kw):
        n += tiles.shape[0]
    torch.cuda.synchronize(); t1 = time.perf_counter()
    print("ingest only: %.0f tiles/s (%d tiles, %.3f s, %.1f GB/s of slide)" % (n / (t1 - t0), n, t1 - t0, raster.nbytes / (t1 - t0) / 1e9), flush=True)
for rep in range(REPS):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    res = detect_region(m, raster, tile, S, conf_thres=0.5, nms_thres=0.4, batch_size=GX, **det_kw)
    torch.cuda.synchronize(); t1 = time.perf_counter()
    print("detect_region%s: %.0f tiles/s, %.3f s, %.2f GB/s of slide (%d tiles, %d with detections, %d rows)"
          % ("(overlap=%d)" % OVERLAP if OVERLAP else "", GY * GX / (t1 - t0), t1 - t0, raster.nbytes / (t1 - t0) / 1e9, GY * GX, len(res),
             sum(len(d) for _, _, d in res)), flush=True)
    if VIEWS != (0,) or opts["--min-views"] != 1:
        c = torch.cat(cands).cpu().numpy(); del cands[:]
        print("  views %d, min_views %d: %d images, %.0f images/s; candidates per tile median %d max %d; tiles beyond 1024: %d, beyond 4096: %d of %d"
              % (len(VIEWS), opts["--min-views"], len(c) * len(VIEWS), len(c) * len(VIEWS) / (t1 - t0), np.median(c), c.max(),
                 (c > 1024).sum(), (c > 4096).sum(), len(c)), flush=True)
