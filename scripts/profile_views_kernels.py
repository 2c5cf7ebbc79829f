"""Kernel timings of the dihedral-views path.  (1) On one strip of the scripts/bench_wsi.py slide (1536 rows x 32 tiles of 1536 px,
226 MB, resident on the device): ay_ingest_region_tiles_list_u8 on 8 tiles against ay_ingest_region_tiles_views_u8 on the same tiles
at V = 1, 4, 8, and the transposed views alone (region_tiles_cut_u8_kernel<V, ay::ListOrigins> and region_tiles_views_u8_kernel<V> in a
trace).  (2) At B = 8 tiles x 8 views of 1024^2 (64 512 rows per view, 3 classes, about 230
candidates per view): ay_unview_rows, the merge-NMS of the concatenated rows, ay_view_votes and ay_view_select.  3 repeats x (1 warm
call + 10 calls between two events) each.
usage: python scripts/profile_views_kernels.py
       rocprofv3 --kernel-trace --stats -d DIR -o vk --output-format csv -- python scripts/profile_views_kernels.py
       python scripts/profile_views_kernels.py --trace DIR     (per kernel, the dispatch durations of DIR's kernel trace; no GPU)"""
import sys
if "--trace" in sys.argv:
    import csv, glob, collections
    files = glob.glob(sys.argv[sys.argv.index("--trace") + 1] + "/**/*kernel_trace.csv", recursive=True)
    d = collections.defaultdict(list)
    for f in files:
        for r in csv.DictReader(open(f)):
            n = r.get("Kernel_Name", "")
            if any(k in n for k in ("region_tiles", "unview_rows", "view_votes", "view_select", "zero_i32", "nms_")):
                d[n.split("(")[0]].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
    for n, v in sorted(d.items()):
        v = sorted(v)
        print("%-70s n=%3d  min %8.1f  median %8.1f  max %8.1f us" % (n[:70], len(v), v[0], v[len(v) // 2], v[-1]))
    sys.exit(0)
import harness
import ctypes as C
import numpy as np, torch
from amyloid_yolo_paper_amd import _lib, utils, views
from amyloid_yolo_paper_amd._lib import check, ptr
L = _lib.lib()
dev = torch.device("cuda:0")
tile, S, TX, NT = 1536, 1024, 32, 8
row = np.ascontiguousarray(harness.synthetic_strip(TX, tile))
W = row.shape[1]
strip = torch.from_numpy(row).to(dev)
origins = torch.tensor([(i * tile * 4, 0) for i in range(NT)], dtype=torch.int32, device=dev)   # 8 tiles spread over the strip
out = torch.empty(NT * 8, 3, S, S, device=dev)
ref = torch.empty(NT, 3, S, S, device=dev)
sp = _lib.stream_ptr
def ingest(ids):
    arr = (C.c_int * len(ids))(*ids)
    return lambda: check(L.ay_ingest_region_tiles_views_u8(ptr(strip), tile, W, W * 3, 1, tile, ptr(origins), NT, arr, len(ids), S, ptr(out), sp()))
# the post-processing: rows as a decode would leave them, candidates in clusters shared by the views
N, K, V, MAXD = 64512, 8, 8, 1024
rng = np.random.default_rng(0)
pred0 = torch.zeros(NT * V, N, K, device=dev)
pred0[..., 0:2] = torch.rand(NT * V, N, 2, device=dev) * S
pred0[..., 2:4] = torch.rand(NT * V, N, 2, device=dev) * 40 + 8
pred0[..., 4] = torch.rand(NT * V, N, device=dev) * 0.45
pred0[..., 5:] = torch.rand(NT * V, N, 3, device=dev)
obj = rng.uniform(40, S - 40, (NT, 230, 2)).astype(np.float32)
for b in range(NT):
    for j in range(V):
        r = torch.from_numpy(rng.choice(N, 230, replace=False)).to(dev)
        box = torch.from_numpy(np.concatenate([obj[b] + rng.uniform(-2, 2, (230, 2)), np.full((230, 2), 30.0)], 1).astype(np.float32)).to(dev)
        pred0[b * V + j, r, 0:4] = box          # every view reports every object, in its own frame after the unview: undo it here
        pred0[b * V + j, r, 4] = 0.9
pred = pred0.clone()
cat = pred.view(NT, V * N, K)
state = {}
def nms():
    pred.copy_(pred0)
    state["r"] = utils.nms_device(cat, 0.5, 0.4, MAXD)
def votes():
    state["v"] = views.view_votes_device(cat, V, 0.5, 0.4, state["r"][0], state["r"][2])
def select():
    rows, keep, count, _ = state["r"]
    views.view_select_device(rows, keep, count, state["v"], 1)      # min_views 1 keeps everything: the same work every call
runs = {
 "list ingest, 8 tiles": lambda: check(L.ay_ingest_region_tiles_list_u8(ptr(strip), tile, W, W * 3, 1, tile, ptr(origins), NT, S, ptr(ref), sp())),
 "views ingest V=1 (0)": ingest((0,)),
 "views ingest V=4 (0,1,2,3)": ingest((0, 1, 2, 3)),
 "views ingest V=4 (4,5,6,7) transposed": ingest((4, 5, 6, 7)),
 "views ingest V=8": ingest(range(8)),
 "copy of the rows (the reset in front of the NMS)": lambda: pred.copy_(pred0),
 "unview_rows 64 images x 64512 rows": lambda: views.unview_rows_device(pred, (1, 2, 3, 4, 5, 6, 7, 0), S),
 "copy + nms_merge 8 x 516096 rows": nms,
 "view_votes": votes,
 "view_select": select,
}
times = harness.time_calls(list(runs.values()), 0, 3, per=10, lead=1)
for rep in range(3):
    for name, ms in zip(runs, times):
        print("rep %d  %-60s %8.1f us per call (events, 10 calls)" % (rep, name[:60], ms[rep] * 1e3), flush=True)
ingest((0,))(); torch.cuda.synchronize()
print("views (0,) == list:", torch.equal(out[:NT], ref), " count", state["r"][2].tolist(), " cand", state["r"][3].tolist(),
      " votes popcount histogram", np.bincount([bin(v).count("1") for v in state["v"].cpu().numpy().ravel()], minlength=9).tolist())
