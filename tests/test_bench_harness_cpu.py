"""CPU: scripts/harness.py, what the measuring scripts under scripts/ share.  The generators and the strip are pinned as SHA-256
digests that were taken from the functions of the commit before the harness (synthetic_slide of bench_slide_match.py, slide_rows of
bench_load.py and bench_focus.py, synthetic_rows of bench_burden.py, synthetic_slide of bench_spatial.py and bench_spatial_window.py,
the strip expression of bench_stain.py): their text was cut out of those files and run on its own, never the new code.  The timing
protocol runs on a fake event type; the formatters on timing lines of profiles/; the kernel table on a stored rocprofv3 table.
profiles/burden.txt holds no `median [min, max]` line (bench_burden.py prints `min .. max ms (median)`, a form of its own that stays
in that script), so the bracket form is checked on profiles/spatial.txt and profiles/augment_ingest.txt."""
import csv
import glob
import hashlib
import os
import re
import runpy
import shutil
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(REPO, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)
import harness  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
# (M, T, side) -> digests of the rows, of the targets and of the rows with the class modulo 2 (bench_burden.py's), None where no
# script of the parent made them.  side 70 000: bench_slide_match / bench_load / bench_burden; 49 152 = 32 * 1536: bench_focus.
SLIDE = {
    (1000, 200, 70000.0): ("7d11065d94db0177fb3e05d9bb7ea7a0917b930064a9234c2094c9fc35859143",
                           "53f42a49110573484dfe868afda4bf0e250760b7022291f0bd8d46f112ba188e",
                           "88b1cc3a9c4e1ec697289bcdc98e688a3cefdf51da2d23456ce8d48be8adfa2f"),
    (250000, 50000, 70000.0): ("bb1f03d2636f5ea27f903c1a9d33fca99c5d4fef3783cd86bde1f761c2791b55",
                               "2f2b66f6265405edff0ec3ec6e62e83ae4f8c84b3b8b65da810de565455a2baa",
                               "13c7041ceae5b82bf88a4244d314c4bda9d705f19faf656810f43aa6ec1a7316"),
    (1000, 200, 49152.0): ("b39be6ec5265eb8693c5fa527892668410f5cdd71ab87647bd31213adb747408", None, None),
    (250000, 50000, 49152.0): ("c419af243b40cb6bf9a72f0edeede2f21e4b49ce357fc05de09a0a6d23e5b47f", None, None),
}
CLUSTERED = {1000: "caa75b3b67fc59145dd0dd86be443701002f9c8190e407671e089f627fc4b277",
             200000: "8f0d4a69ead5cea9abc70a0d19c98074114566398520b9cc334f87cf19565d65"}
STRIP = {1: "1055a29a9da97800d1b3159e471efd8a746cf913f3231e51afcf8e2488592c53",
         5: "147b2908bedaced0cad8e99fb964863eab126aec9d2401d27ee4a4b179dfbf70"}


@pytest.mark.parametrize("key", list(SLIDE), ids=lambda k: "M%d_T%d_side%d" % k)
def test_slide_rows_are_the_draws_of_the_parent_scripts(key):
    M, T, side = key
    want_rows, want_targets, want_mod2 = SLIDE[key]
    rows, targets = harness.slide_rows(M, T, side)
    assert rows.shape == (M, 7) and targets.shape == (T, 5) and rows.dtype == targets.dtype == np.float32
    assert digest(rows) == want_rows
    assert digest(harness.slide_rows(M, T, int(side))[0]) == want_rows          # bench_burden.py passes an integer side
    if want_targets:
        assert digest(targets) == want_targets
    if want_mod2:
        rows[:, 6] %= 2                                                         # what bench_burden.py does to column 6
        assert digest(rows) == want_mod2 and set(np.unique(rows[:, 6])) <= {0.0, 1.0}


@pytest.mark.parametrize("M", list(CLUSTERED))
def test_clustered_rows_are_the_draws_of_the_parent_scripts(M):
    rows = harness.clustered_rows(M, 70000)
    assert rows.shape == (M, 7) and rows.dtype == np.float32 and digest(rows) == CLUSTERED[M]


@pytest.mark.parametrize("tx", list(STRIP))
def test_synthetic_strip(tx):
    strip = harness.synthetic_strip(tx)
    assert strip.shape == (1536, tx * 1536, 3) and strip.dtype == np.uint8 and digest(strip) == STRIP[tx]


# ---- timing -------------------------------------------------------------------------------------------------------------------------
def fake_events():
    """-> (log, Event): an event type that writes what happens to it into log; a pair's time is 1 ms per call between the events"""
    log = []

    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing
            log.append(("new", self))

        def record(self):
            self.at = len(log)
            log.append(("record", self))

        def synchronize(self):
            log.append(("wait", self))

        def elapsed_time(self, other):
            return float(sum(1 for what, _ in log[self.at:other.at] if what == "call"))

    return log, Event


def pairs_of(log):
    """the event pairs of a log in order: [(names of the calls between the two records, waited for the second event)]"""
    out, i = [], 0
    kinds = [what for what, _ in log]
    while "record" in kinds[i:]:
        i = kinds.index("record", i)
        j = kinds.index("record", i + 1)
        assert all(k == "call" for k in kinds[i + 1:j]) and log[i][1] is not log[j][1]
        out.append(([name for _, name in log[i + 1:j]], log[j + 1] == ("wait", log[j][1])))
        i = j + 1
    return out


@pytest.mark.parametrize("warm, reps, per", [(3, 20, 1), (0, 9, 10), (2, 4, 5), (3, 0, 1)])
def test_time_calls_takes_the_calls_in_turn_and_drops_the_warm_rounds(warm, reps, per):
    log, Event = fake_events()
    names = ["a", "b", "c"]
    calls = [lambda n=n: log.append(("call", n)) for n in names]
    ms = harness.time_calls(calls, warm, reps, per=per, Event=Event)
    pairs = pairs_of(log)
    # every round takes a, b, c in turn; `per` invocations of one call sit between one pair of events; the second event is waited for
    assert pairs == [([n] * per, True) for _ in range(warm + reps) for n in names]
    assert [what for what, _ in log].count("call") == (warm + reps) * per * len(names)
    # exactly `warm` rounds are dropped, and the time is per invocation
    assert len(ms) == len(names) and all(m == [1.0] * reps for m in ms)


def test_time_calls_counts_only_the_timed_rounds():
    """the time of a pair grows with the round, so the kept values say which rounds were kept"""
    log, Event = fake_events()
    rounds = []

    def call():
        for _ in range(len(rounds)):           # as many log entries as rounds so far: round r takes r + 1 "ms"
            log.append(("call", "x"))

    def count():
        rounds.append(1)

    ms = harness.time_calls([count, call], 2, 3, Event=Event)
    assert ms[1] == [3.0, 4.0, 5.0] and ms[0] == [0.0, 0.0, 0.0]


def test_time_calls_single_call_and_lead():
    log, Event = fake_events()
    f = lambda: log.append(("call", "f"))      # noqa: E731
    assert harness.time_calls([f], 1, 2, Event=Event) == [[1.0, 1.0]]
    del log[:]
    ms = harness.time_calls([f], 0, 2, per=10, lead=1, Event=Event)
    # one invocation outside the timed pair, waited for, in front of every timed pair of ten
    assert pairs_of(log) == [(["f"], True), (["f"] * 10, True)] * 2 and ms == [[1.0, 1.0]]


def test_time_calls_defaults_to_the_device_event():
    import inspect
    import torch
    assert inspect.signature(harness.time_calls).parameters["Event"].default is None
    if not torch.cuda.is_available():          # no fallback: without a device the scripts fail as they did
        with pytest.raises(Exception):
            harness.time_calls([lambda: None], 0, 1)


def timing_line(path, pattern):
    """the first line of profiles/<path> that matches, and its three numbers in the order median, min, max"""
    for line in open(os.path.join(REPO, "profiles", path)):
        m = re.search(pattern, line)
        if m:
            return line, [float(v) for v in m.groups()]
    raise AssertionError(path)


def test_formatters_reproduce_stored_timing_lines():
    num = r"(\d+\.\d+)"
    line, v = timing_line("focus.txt", rf"{num} ms \({num} \.\. {num}\)")
    assert line.startswith("ay_tile_tissue_u8           : 0.089 ms (0.086 .. 0.090) per strip")
    assert "ay_tile_tissue_u8           : %s per strip" % harness.fmt_round(v) == line[:line.index(" per strip") + 10]
    line, v = timing_line("spatial.txt", rf"{num} ms  \[{num}, {num}\]")
    assert line.startswith("call, r_max   64 px           0.155 ms  [0.152, 0.161]   cells")
    assert f"call, {'r_max   64 px':20s} {harness.fmt_square(v)}   cells" == line[:line.index("cells") + 5]
    line, v = timing_line("augment_ingest.txt", rf"{num} us  \[{num}, {num}\]")
    assert line.startswith("ay_ingest_tiles_u8                  133.5 us  [132.6, 140.8]   4.71 TB/s")
    assert f"{'ay_ingest_tiles_u8':32s} {harness.fmt_square([t / 1e3 for t in v], us=True)}   4.71 TB/s" == line[:line.index("TB/s") + 4]
    # profiles/burden.txt: bench_burden.py's own form, from the same three numbers
    line, (lo, hi, med) = timing_line("burden.txt", rf"{num} \.\. {num} ms \(median {num}\)")
    assert harness.fmt_round([med, lo, hi]) == "0.032 ms (0.031 .. 0.036)" and harness.fmt_square([med, lo, hi]) == "   0.032 ms  [0.031, 0.036]"
    assert abs(harness.spread([0.079, 0.077, 0.084]) - (0.084 - 0.077) / 0.079) < 1e-12


# ---- kernel table -------------------------------------------------------------------------------------------------------------------
STORED = os.path.join(REPO, "profiles", "r04_bench_b64_kernel_stats_v5.csv")


def test_kernel_table_selects_by_substring(tmp_path):
    run = tmp_path / "trace" / "run"
    run.mkdir(parents=True)
    shutil.copy(STORED, run / "x_kernel_stats.csv")
    rows, calls = harness.kernel_table(str(tmp_path / "trace"), ["conv3x3_m16"])
    with open(STORED) as f:
        want = [r for r in csv.DictReader(f) if "conv3x3_m16" in r["Name"]]
    assert len(want) == 2 and rows == want and calls == max(int(r["Calls"]) for r in want) == 154
    both, calls_both = harness.kernel_table(str(tmp_path / "trace"), ["conv3x3_m16", "nms_"])
    assert [r for r in both if "conv3x3_m16" in r["Name"]] == want and len(both) > len(want) and calls_both >= calls
    said = []
    harness.say_kernel_table(said.append, rows, calls, "sum of the two")
    total = sum(float(r["TotalDurationNs"]) for r in want)
    assert len(said) == 3 and said[-1] == f"  {'sum of the two':60s} {total / 154 / 1e3:8.1f} us"
    assert said[0] == f"  {'void ay::conv3x3_m16_ring_kernel<true, ay::Bf16>':60s} {77831752 / 154 / 1e3:8.1f} us"
    assert [float(s.split()[-2]) for s in said[:2]] == sorted((float(s.split()[-2]) for s in said[:2]), reverse=True)
    every, _ = harness.kernel_table(str(tmp_path / "trace"), [""])          # what kernel_stats.py reads: every row, the file's order
    with open(STORED) as f:
        assert every == list(csv.DictReader(f))


def test_kernel_table_names_a_directory_without_a_table(tmp_path):
    with pytest.raises(FileNotFoundError, match=re.escape(str(tmp_path))):
        harness.kernel_table(str(tmp_path), ["conv"])


# ---- report -------------------------------------------------------------------------------------------------------------------------
GAP = "normalisation gap, mean |byte difference| to slide A over the tissue: raw slide B 16.2000"       # tests/test_stain_basis_cpu.py's


def test_report_replace_append_and_keep_prefix(tmp_path, capsys):
    path = tmp_path / "not" / "there" / "yet" / "out.txt"
    r = harness.Report()
    r.say("first")
    r.say("second")
    assert capsys.readouterr().out == "first\nsecond\n" and r.lines == ["first", "second"]
    r.write(None)                                                   # no --out: nothing is written
    assert not path.parent.exists()
    r.write(str(path))                                              # the parent directory is created
    assert path.read_text() == "first\nsecond\n"
    r.write(str(path))                                              # replace
    assert path.read_text() == "first\nsecond\n"
    r.write(str(path), append=True)                                 # append
    assert path.read_text() == "first\nsecond\nfirst\nsecond\n"
    path.write_text("an old line\n" + GAP + "\nanother old line\n" + GAP.replace("raw slide B 16.2000", "H_DAB map 13.5444") + "\n")
    r.write(str(path), keep_prefix="normalisation gap")             # the other writer's lines stay, behind the new ones
    assert path.read_text() == "first\nsecond\n" + GAP + "\n" + GAP.replace("raw slide B 16.2000", "H_DAB map 13.5444") + "\n"
    fresh = tmp_path / "fresh.txt"
    r.write(str(fresh), keep_prefix="normalisation gap")            # nothing to keep yet
    assert fresh.read_text() == "first\nsecond\n"


def test_the_gap_line_is_the_one_the_stain_basis_test_writes():
    src = open(os.path.join(REPO, "tests", "test_stain_basis_cpu.py")).read()
    assert 'f"normalisation gap, mean |byte difference| to slide A over the tissue: {name} {v:.4f}"' in src
    assert 'keep_prefix="normalisation gap"' in open(os.path.join(SCRIPTS, "bench_stain_basis.py")).read()


# ---- rehearsal ----------------------------------------------------------------------------------------------------------------------
PORTED = sorted(glob.glob(os.path.join(SCRIPTS, "bench_*.py")) + glob.glob(os.path.join(SCRIPTS, "profile_*_kernels.py"))
                + [os.path.join(SCRIPTS, "kernel_stats.py"), os.path.join(SCRIPTS, "time_wgrad.py")])


def test_every_script_compiles_and_uses_the_harness():
    assert len(PORTED) == 17
    shared = ("Event(enable_timing", "def say", "_kernel_stats.csv", "def next_strip", "rng.uniform(8, 47", "rng.normal(0, 150.0")
    for path in sorted(glob.glob(os.path.join(SCRIPTS, "*.py"))):
        src = open(path).read()
        compile(src, path, "exec")
        if path.endswith("harness.py"):
            assert all(s in src for s in shared if s != "def next_strip")       # the rotation's method is Rotation.next
            continue
        for gone in shared:                                                     # in harness.py and nowhere else
            assert gone not in src, (path, gone)
        if path in PORTED:
            assert "import harness" in src and "sys.path.insert" not in src, path


@pytest.mark.parametrize("name", [os.path.basename(p) for p in PORTED if "argparse" in open(p).read()])
def test_help_needs_no_device(name, monkeypatch, capsys):
    """`python scripts/<name> --help` ends with status 0 before anything touches the device (run here inside this process)"""
    monkeypatch.setattr(sys, "argv", [os.path.join(SCRIPTS, name), "--help"])
    with pytest.raises(SystemExit) as e:
        runpy.run_path(os.path.join(SCRIPTS, name), run_name="__main__")
    assert e.value.code == 0 and "usage:" in capsys.readouterr().out
