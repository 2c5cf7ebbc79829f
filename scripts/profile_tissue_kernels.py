"""Kernel timings of the tissue path on one strip of the scripts/bench_wsi.py slide (1536 rows x 32 tiles of 1536 px, 226 MB, resident
on the device): ay_tile_tissue_u8 (16-byte loads, byte loads, shrink 2, abutting and overlapping grid), ay_ingest_region_tiles_step_u8,
ay_ingest_region_tiles_u8 (the step entry at step == tile) and ay_ingest_region_tiles_list_u8 on the full grid (one kernel,
region_tiles_cut_u8_kernel<V, Origins>, in a trace); 3 repeats x (1 warm call + 10 calls between two events) each.
usage: python scripts/profile_tissue_kernels.py
       rocprofv3 --kernel-trace --stats -d DIR -o tk --output-format csv -- python scripts/profile_tissue_kernels.py
       python scripts/profile_tissue_kernels.py --trace DIR     (per kernel, the dispatch durations of DIR's kernel trace; no GPU)"""
import sys
if "--trace" in sys.argv:
    import csv, glob, collections
    files = glob.glob(sys.argv[sys.argv.index("--trace") + 1] + "/**/*kernel_trace.csv", recursive=True)
    d = collections.defaultdict(list)
    for f in files:
        for r in csv.DictReader(open(f)):
            n = r.get("Kernel_Name", "")
            if any(k in n for k in ("tile_tissue", "region_tiles", "zero_i32")):
                d[n.split("(")[0]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    for n, v in sorted(d.items()):
        v = sorted(v)
        print("%-70s n=%3d  min %8.1f  median %8.1f  max %8.1f us" % (n[:70], len(v), v[0], v[len(v) // 2], v[-1]))
    sys.exit(0)
import harness
import numpy as np, torch
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
L = _lib.lib()
dev = torch.device("cuda:0")
tile, S, TX = 1536, 1024, 32
row = np.ascontiguousarray(harness.synthetic_strip(TX, tile))
W = row.shape[1]
strip = torch.from_numpy(row).to(dev)
off = torch.empty(row.size + 16, dtype=torch.uint8, device=dev); off[1:1 + row.size] = strip.reshape(-1)
out = torch.empty(TX, 3, S, S, device=dev)
out2 = torch.empty(TX, 3, S, S, device=dev)
counts = torch.empty(64, dtype=torch.int32, device=dev)
origins = torch.tensor([(i * tile, 0) for i in range(TX)], dtype=torch.int32, device=dev)
sp = _lib.stream_ptr
runs = {
 "tissue wide step=tile (32 tiles)": lambda: check(L.ay_tile_tissue_u8(ptr(strip), tile, W, W * 3, 1, tile, tile, 1, TX, 170, ptr(counts), sp())),
 "tissue wide step=1408 (35 tiles)": lambda: check(L.ay_tile_tissue_u8(ptr(strip), tile, W, W * 3, 1, tile, 1408, 1, 35, 170, ptr(counts), sp())),
 "tissue bytewise base+1": lambda: check(L.ay_tile_tissue_u8(ptr(off[1:]), tile, W, W * 3, 1, tile, tile, 1, TX, 170, ptr(counts), sp())),
 "tissue wide shrink=2 (16 tiles of 1536 on 768 rows)": lambda: check(L.ay_tile_tissue_u8(ptr(strip), tile, W, W * 3, 2, tile, tile, 1, 16, 170, ptr(counts), sp())),
 "step ingest step=tile": lambda: check(L.ay_ingest_region_tiles_step_u8(ptr(strip), tile, W, W * 3, 1, tile, tile, 1, TX, S, ptr(out), sp())),
 "grid ingest (the entry without a step)": lambda: check(L.ay_ingest_region_tiles_u8(ptr(strip), tile, W, W * 3, 1, tile, 1, TX, S, ptr(out), sp())),
 "list ingest full grid": lambda: check(L.ay_ingest_region_tiles_list_u8(ptr(strip), tile, W, W * 3, 1, tile, ptr(origins), TX, S, ptr(out2), sp())),
}
times = harness.time_calls(list(runs.values()), 0, 3, per=10, lead=1)
for rep in range(3):
    for name, ms in zip(runs, times):
        print("rep %d  %-52s %8.1f us per call (events, 10 calls)" % (rep, name, ms[rep] * 1e3), flush=True)
print("list == step:", torch.equal(out, out2), " counts[:4]", counts[:4].tolist(), " source bytes", row.size)
