"""What the measuring scripts of this directory share, and nothing that only one of them needs: the report (say / --out), the
event-timing protocol and its formatters, the synthetic strip and the rotation over its copies, the two generators of detection
rows, the reader of a rocprofv3 kernel table and the --calls-only mode.  The scripts import it (`python scripts/bench_x.py` puts
this directory on the path); the package does not.  Importing it puts the repository root on the path, so the scripts import the
package after it.  torch and the package are imported where they are used: kernel_stats.py and the --trace modes need neither."""
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np


# ---- report -------------------------------------------------------------------------------------------------------------------------
class Report:
    """the lines of a run: say() prints a line and keeps it, write() puts the kept lines into the --out file"""

    def __init__(self):
        self.lines = []

    def say(self, s):
        print(s, flush=True)
        self.lines.append(s)

    def write(self, path, append=False, keep_prefix=None):
        """Replace `path` by the lines (append=True: add them to it); the parent directory is created; path None: nothing.
        keep_prefix: the lines of the file so far that begin with it stay, behind the new ones (another writer owns them)."""
        if not path:
            return
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        kept = []
        if keep_prefix is not None and os.path.exists(path):
            kept = [ln for ln in open(path).read().splitlines() if ln.startswith(keep_prefix)]
        with open(path, "a" if append else "w") as f:
            f.write("\n".join(self.lines + kept) + "\n")


# ---- timing -------------------------------------------------------------------------------------------------------------------------
def time_calls(calls, warm, reps, per=1, lead=0, Event=None):
    """The timing protocol of every script here.  warm + reps rounds; in every round each of `calls` is taken in turn: two device
    events around `per` invocations of it, then a wait for the second event.  The first `warm` rounds are dropped.
    lead: that many invocations outside the events in front of every event pair (the "warm call" of the scripts that time `per`
    launches at once), waited for before the first event is recorded.
    -> one list per call of `reps` times in milliseconds per invocation (the time between the events over `per`).
    Event: the event type, torch.cuda.Event unless a test passes its own; there is no fallback without a device."""
    if Event is None:
        import torch
        Event = torch.cuda.Event

    def pair(call, n):
        e0, e1 = Event(enable_timing=True), Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    ms = [[] for _ in calls]
    for i in range(warm + reps):
        for k, call in enumerate(calls):
            if lead:
                pair(call, lead)
            t = pair(call, per)
            if i >= warm:
                ms[k].append(t)
    return ms


def fmt_round(ms):
    """median (min .. max)"""
    return "%.3f ms (%.3f .. %.3f)" % (statistics.median(ms), min(ms), max(ms))


def fmt_square(ms, us=False):
    """median [min, max], in milliseconds to 1 us or (us=True) in microseconds to 0.1 us"""
    k, d, unit = (1e3, 1, "us") if us else (1, 3, "ms")
    return "%8.*f %s  [%.*f, %.*f]" % (d, statistics.median(ms) * k, unit, d, min(ms) * k, d, max(ms) * k)


def spread(ms):
    """(max - min) / median"""
    return (max(ms) - min(ms)) / statistics.median(ms)


def calls_only(n, fn):
    """the --calls-only mode, for a kernel trace: n calls, a device synchronisation, and the process leaves"""
    import torch
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    sys.exit(0)


# ---- the synthetic strip ------------------------------------------------------------------------------------------------------------
def synthetic_tiles(tile=1536):
    """uint8 [4, tile, tile, 3]: the four synthetic tiles every strip, batch and raster of the scripts is made of"""
    from amyloid_yolo_paper_amd import synth
    return (synth.synth_tiles(4, tile, start=0) * 255).astype(np.uint8).transpose(0, 2, 3, 1)


def synthetic_strip(tx, tile=1536):
    """uint8 [tile, tx * tile, 3]: one tile row, the four synthetic tiles in turn"""
    base = synthetic_tiles(tile)
    return np.concatenate([base[i % 4] for i in range(tx)], 1)


class Rotation:
    """`copies` copies of a device tensor at different addresses (the tensor itself is one of them).  A loop that reads one buffer
    again and again may be served from the 256 MiB last-level cache; calls that take next() read the copy read longest ago."""

    def __init__(self, tensor, copies):
        self.copies = [tensor] + [tensor.clone() for _ in range(copies - 1)]
        self.turn = 0

    def next(self):
        """the pointer of the copy this call reads"""
        from amyloid_yolo_paper_amd._lib import ptr
        self.turn += 1
        return ptr(self.copies[self.turn % len(self.copies)])


# ---- detection rows -----------------------------------------------------------------------------------------------------------------
def slide_rows(M, T, side, seed=0):
    """-> (rows [M, 7], targets [T, 5]), float32.  T annotations of 8..47 px anywhere on a `side`-px square; four rows in five are
    jittered sightings of an annotation (several per annotation), the rest boxes of the same sizes anywhere; three classes, scores
    in (0.5, 1).  rows: x1 y1 x2 y2 conf score class; targets: class x1 y1 x2 y2."""
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, side, (T, 2))
    tb = np.concatenate([xy, xy + rng.uniform(8, 47, (T, 2))], 1)
    cls = rng.integers(0, 3, T)
    g = rng.integers(0, T, M)
    box = tb[g] + rng.normal(0, 3.0, (M, 4))
    anywhere = rng.uniform(size=M) < 0.2
    p = rng.uniform(0, side, (M, 2))
    box[anywhere] = np.concatenate([p, p + rng.uniform(8, 47, (M, 2))], 1)[anywhere]
    rows = np.concatenate([box, rng.uniform(0.5, 1, (M, 2)), cls[g][:, None]], 1).astype(np.float32)
    return rows, np.concatenate([cls[:, None], tb], 1).astype(np.float32)


def clustered_rows(M, side, seed=0):
    """-> rows [M, 7], float32: boxes of 8..60 px of two classes around 2 000 parents on a `side`-px square (offspring sigma 150 px),
    a quarter of the rows anywhere"""
    rng = np.random.default_rng(seed)
    parents = rng.uniform(0, side, (2000, 2))
    xy = parents[rng.integers(0, 2000, M)] + rng.normal(0, 150.0, (M, 2))
    loose = rng.uniform(size=M) < 0.25
    xy[loose] = rng.uniform(0, side, (int(loose.sum()), 2))
    wh = rng.uniform(8, 60, (M, 2))
    return np.concatenate([xy - wh / 2, xy + wh / 2, rng.uniform(0.5, 1, (M, 2)), rng.integers(0, 2, (M, 1))], 1).astype(np.float32)


# ---- the kernel table of a trace ----------------------------------------------------------------------------------------------------
def kernel_table(directory, substrings):
    """-> (rows, calls): the rows (dicts, in the file's order) of the *_kernel_stats.csv under the directory of a
    `rocprofv3 --kernel-trace --stats` run whose kernel name holds one of `substrings`, and the largest `Calls` among them"""
    files = glob.glob(os.path.join(directory, "**", "*_kernel_stats.csv"), recursive=True)
    if not files:
        raise FileNotFoundError(f"no *_kernel_stats.csv under {directory}: not the directory of a rocprofv3 --kernel-trace --stats run")
    with open(files[0]) as f:
        rows = [r for r in csv.DictReader(f) if any(s in r["Name"] for s in substrings)]
    return rows, max((int(r["Calls"]) for r in rows), default=0)


def say_kernel_table(say, rows, calls, sum_label):
    """the "us per call" lines: every row's total time over `calls`, the longest first, and their sum under `sum_label`"""
    for r in sorted(rows, key=lambda r: -float(r["TotalDurationNs"])):
        say(f"  {r['Name'].split('(')[0][:60]:60s} {float(r['TotalDurationNs']) / calls / 1e3:8.1f} us")
    say(f"  {sum_label:60s} {sum(float(r['TotalDurationNs']) for r in rows) / calls / 1e3:8.1f} us")
