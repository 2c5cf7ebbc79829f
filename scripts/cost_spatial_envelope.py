"""What the random-labelling envelope costs: ONE ay_pair_counts_relabel call with S labellings (a) against S plain ay_pair_counts
calls on rows whose class column is swapped from the same label table (b) -- what a user could do before the relabel call existed --
in the same process, on the slide of scripts/bench_spatial.py (harness.clustered_rows: 200 k clustered detection rows of two classes
on a 70 000-px square, B = 16 radii); rows (for (b): all S copies with their class columns already swapped), table, outputs and
workspace resident on the device.
HOST time: wsi.relabel_table for the S - 1 simulations (NumPy, one stable argsort of uint64 keys per simulation), wall clock.
CALL time: after WARM warm rounds, REPS times and ALTERNATING: two device events around (a) one relabel call, (b) the S plain calls;
median [min, max] over the REPS, and the ratio of the medians.  Before the timing the S blocks of (a) are compared with the S results
of (b), byte for byte.
Also (a) and (b) at a realistic 5 000 rows (a square of the same density).
usage: python scripts/cost_spatial_envelope.py [--reps 7] [--sims 100] [--out profiles/spatial_envelope.txt]"""
import argparse
import ctypes as C
import statistics
import time

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd._lib import check, ptr

ap = argparse.ArgumentParser()
ap.add_argument("--rows", type=int, default=200000)
ap.add_argument("--side", type=int, default=70000, help="side of the square slide in pixels")
ap.add_argument("--sims", type=int, default=100, help="S: the labellings of one call, the observed one included")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--out", default=None)
a = ap.parse_args()

report = harness.Report()
say = report.say
L = _lib.lib()
dev = torch.device("cuda:0")
NC, B, S = 2, 16, a.sims
I32P = C.POINTER(C.c_int32)


def radii(r_max_px):
    return np.ascontiguousarray([4 * r_max_px * (k + 1) // B for k in range(B)], np.int32)


class Case:
    """M rows on a square of `side` px: the table, the S relabelled copies of the rows, the outputs of both calls"""

    def __init__(self, M, side):
        self.M, self.side = M, side
        rows_h = harness.clustered_rows(M, side)
        labels = rows_h[:, 6].astype(np.int64)                          # (every row of the generator is counted at min_conf 0)
        t0 = time.perf_counter()
        table = wsi.relabel_table(labels, NC, S - 1, 0)
        self.table_s = time.perf_counter() - t0
        self.stride = (S + 63) & ~63
        padded = np.full((M, self.stride), 255, np.uint8)
        padded[:, :S] = table
        self.labels = torch.from_numpy(padded).to(dev)
        self.rows = torch.from_numpy(rows_h).to(dev)
        self.copies = []
        for s in range(S):                                              # (b)'s inputs, made outside the timed region
            r = rows_h.copy()
            r[:, 6] = table[:, s]
            self.copies.append(torch.from_numpy(r).to(dev))
        self.sim_pairs = torch.empty(S, NC, NC, B, device=dev, dtype=torch.int64)
        self.sim_centres = torch.empty(S, NC, B, device=dev, dtype=torch.int32)
        self.sim_inside = torch.empty(S, NC, device=dev, dtype=torch.int32)
        self.pairs = torch.empty(S, NC, NC, B, device=dev, dtype=torch.int64)      # (b) keeps every result, as a user would
        self.centres = torch.empty(S, NC, B, device=dev, dtype=torch.int32)
        self.stats_b = torch.empty(S, 2 * NC + 3, device=dev, dtype=torch.int32)
        self.nn, self.bd = torch.empty(M, NC, 2, device=dev, dtype=torch.int32), torch.empty(M, device=dev, dtype=torch.int32)
        self.stats = torch.empty(2 * NC + 3, device=dev, dtype=torch.int32)

    def callers(self, r_max_px):
        """-> (a, b): one relabel call; the S plain calls"""
        M, side, rq = self.M, self.side, radii(r_max_px)
        need_a = int(L.ay_pair_counts_relabel_workspace_bytes(M, NC, B, side, side, int(rq[-1]), 0, 0, S))
        need_b = int(L.ay_pair_counts_workspace_bytes(M, side, side, int(rq[-1]), 0))
        ws_a, ws_b = (torch.empty(n, device=dev, dtype=torch.uint8) for n in (need_a, need_b))

        def relabel():
            check(L.ay_pair_counts_relabel(ptr(self.rows), M, NC, side, side, C.c_float(0.0), rq.ctypes.data_as(I32P), B, None, 1, 0, None, 0,
                                           ptr(self.labels), S, self.stride, ptr(self.sim_pairs), ptr(self.sim_centres), ptr(self.sim_inside),
                                           ptr(self.bd), ptr(self.stats), ptr(ws_a), need_a, _lib.stream_ptr()), "ay_pair_counts_relabel")

        def plain():
            for s in range(S):
                check(L.ay_pair_counts(ptr(self.copies[s]), M, NC, side, side, C.c_float(0.0), rq.ctypes.data_as(I32P), B, None, 1, 0, ptr(self.pairs[s]),
                                       ptr(self.centres[s]), ptr(self.nn), ptr(self.bd), ptr(self.stats_b[s]), ptr(ws_b), need_b, _lib.stream_ptr()),
                      "ay_pair_counts")

        return relabel, plain

    def measure(self, r_max_px):
        fa, fb = self.callers(r_max_px)
        fa(), fb()
        torch.cuda.synchronize()
        same = torch.equal(self.sim_pairs, self.pairs) and torch.equal(self.sim_centres, self.centres) and \
            torch.equal(self.sim_inside, self.stats_b[:, NC:2 * NC])
        n_pairs = int(self.sim_pairs[0, :, :, -1].sum().item())
        res = harness.time_calls([fa, fb], a.warm, a.reps)
        ma, mb = statistics.median(res[0]), statistics.median(res[1])
        say(f"{self.M:7d} rows, r_max {r_max_px:4d} px: (a) one relabel call, S = {S}  {harness.fmt_square(res[0])}")
        say(f"{self.M:7d} rows, r_max {r_max_px:4d} px: (b) {S} plain calls          {harness.fmt_square(res[1])}   (b) / (a) = {mb / ma:.2f}; "
            f"{mb / S:.3f} ms a plain call; the S blocks of (a) {'equal' if same else 'DIFFER FROM'} the S results of (b); "
            f"{n_pairs} ordered pairs within r_max of an eligible centre")
        return same


say(f"# ay_pair_counts_relabel (a) against S plain ay_pair_counts calls (b) on {torch.cuda.get_device_name(0)}: C = {NC}, B = {B}, S = {S} labellings "
    f"(the observed one and {S - 1} simulations); CALL time = {a.reps} x (two events around (a), then around (b)), after {a.warm} warm rounds; "
    "median [min, max]")
ok = True
for M, side in ((a.rows, a.side), (5000, int(round(a.side * (5000 / a.rows) ** 0.5)))):
    case = Case(M, side)
    say(f"# {M} rows on a {side}-px square: host relabel_table for {S - 1} simulations {case.table_s * 1e3:.1f} ms (NumPy, wall clock); "
        f"table {case.labels.numel() / 2 ** 20:.1f} MiB on the device (stride {case.stride})")
    for r_max in (256, 1024):
        ok = case.measure(r_max) and ok
    del case
report.write(a.out)
if not ok:
    raise SystemExit("the relabel call and the plain calls disagree")
