"""Cost of the fused training augmentation (ay_augment_ingest_u8) next to the plain ingest it extends, at the training shape:
B tiles of TILE^2 uint8 -> B x 3 x S^2 fp32, all resident on the device.  In one process, on the same batch:
  ay_ingest_tiles_u8 (the existing kernel) | ay_augment_ingest_u8 with identity records | ay_augment_ingest_u8 with full random records
each timed between two device events around CALLS launches after a warm call, REPS times; the median of the REPS is reported with
min and max, and the rate the pass's traffic (output bytes + every source byte once: an upper bound on the reads) amounts to.
Then, for information (it depends on the box's CPUs): images/s a DataLoader with --n_cpu workers delivers from PNG tiles in the host
fp32 form and in the raw uint8 form of ListDataset.
usage: python scripts/bench_augment.py [--batch 32] [--tile 1536] [--size 1024] [--out profiles/augment_ingest.txt] [--step_ms 69.0]
       rocprofv3 --kernel-trace --stats -d DIR -o aug --output-format csv -- python scripts/bench_augment.py --no_loader
--step_ms: the training step (bench.py --mode train, same box) the 1.5 % bar refers to; without it only the times are printed."""
import argparse
import os
import statistics
import tempfile
import time

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib, augment as ag
from amyloid_yolo_paper_amd._lib import check, ptr

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--tile", type=int, default=1536)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--step_ms", type=float, default=None)
ap.add_argument("--no_loader", action="store_true")
ap.add_argument("--loader_tiles", type=int, default=64)
ap.add_argument("--n_cpu", type=int, default=8)
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say

L = _lib.lib()
dev = torch.device("cuda:0")
B, T, S = a.batch, a.tile, a.size
base = harness.synthetic_tiles(T)
tiles = torch.from_numpy(np.ascontiguousarray(np.stack([base[i % 4] for i in range(B)]))).to(dev)
sizes = [(T, T)] * B
tables = {"identity": ag.identity_params(sizes), "full": ag.sample_params(np.random.default_rng(0), sizes)}
dtab = {k: torch.from_numpy(v.dev.view(np.uint8).reshape(-1).copy()).to(dev) for k, v in tables.items()}
out = torch.empty(B, 3, S, S, device=dev)
out_id = torch.empty(B, 3, S, S, device=dev)
sp = _lib.stream_ptr
runs = {
    "ay_ingest_tiles_u8": lambda: check(L.ay_ingest_tiles_u8(ptr(tiles), B, T, T, S, 0.0, ptr(out), sp())),
    "ay_augment_ingest_u8 identity": lambda: check(L.ay_augment_ingest_u8(ptr(tiles), tiles.numel(), ptr(dtab["identity"]), B, S, ptr(out_id), sp())),
    "ay_augment_ingest_u8 full": lambda: check(L.ay_augment_ingest_u8(ptr(tiles), tiles.numel(), ptr(dtab["full"]), B, S, ptr(out_id), sp())),
}
traffic = B * 3 * S * S * 4 + tiles.numel()
say(f"# augment ingest on {torch.cuda.get_device_name(0)}: B={B}, {T}^2 uint8 -> {S}^2 fp32; output {B * 3 * S * S * 4 / 1e6:.0f} MB + source "
    f"{tiles.numel() / 1e6:.0f} MB; {a.reps} x ({a.calls} calls between two events after a warm call), median [min, max]")
times = dict(zip(runs, harness.time_calls(list(runs.values()), 0, a.reps, per=a.calls, lead=1)))     # the three alternate inside every repeat
med = {}
for name, v in times.items():
    med[name] = statistics.median(v)
    say(f"{name:32s} {harness.fmt_square(v, us=True)}   {traffic / med[name] / 1e9:.2f} TB/s of output + source")
runs["ay_ingest_tiles_u8"]()
runs["ay_augment_ingest_u8 identity"]()
torch.cuda.synchronize()
say(f"identity records == ay_ingest_tiles_u8, bitwise: {torch.equal(out, out_id)}")
if a.step_ms:
    share = med["ay_augment_ingest_u8 full"] / a.step_ms
    say(f"full augmentation = {100 * share:.2f} % of the {a.step_ms:.1f} ms training step (bar 1.5 %): {'met' if share <= 0.015 else 'MISSED'}")

if not a.no_loader:
    from PIL import Image
    from torch.utils.data import DataLoader
    from amyloid_yolo_paper_amd.datasets import ListDataset
    with tempfile.TemporaryDirectory() as d:
        os.makedirs(os.path.join(d, "images"))
        os.makedirs(os.path.join(d, "labels"))
        paths = []
        for i in range(a.loader_tiles):
            p = os.path.join(d, "images", f"t{i}.png")
            Image.fromarray(base[i % 4]).save(p, compress_level=1)
            with open(os.path.join(d, "labels", f"t{i}.txt"), "w") as fh:
                fh.write("0 0.5 0.5 0.1 0.1\n")
            paths.append(p)
        with open(os.path.join(d, "train.txt"), "w") as fh:
            fh.write("\n".join(paths) + "\n")
        for raw in (False, True):
            ds = ListDataset(os.path.join(d, "train.txt"), img_size=S, multiscale=False, raw_u8=raw)
            loader = DataLoader(ds, batch_size=8, shuffle=False, num_workers=a.n_cpu, pin_memory=True, collate_fn=ds.collate_fn)
            n, t0 = 0, None
            for epoch in range(2):            # the first pass starts the workers and warms the page cache
                if epoch == 1:
                    t0 = time.time()
                for batch in loader:
                    n += len(batch[0]) if epoch == 1 else 0
            dt = time.time() - t0
            say(f"loader, {a.n_cpu} workers, {T}^2 PNG tiles, {'raw uint8 form' if raw else 'host fp32 form '}: {n / dt:7.1f} images/s "
                f"({n} images in {dt:.2f} s; for information, depends on the box's CPUs)")
report.write(a.out)
