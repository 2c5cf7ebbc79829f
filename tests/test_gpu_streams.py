"""GPU (-m gpu): the two properties of the persistent convolution launches that every real batch and bench.py rely on, held to
an independent reference.  Every comparison in this file is equality.

A. ITEMS DEALT BY THE COUNTER.  A ring launch deals a workgroup its first D items statically and takes the others from its XCD's
   atomic counter (ItemDealer::fetch).  The exact tests of test_gpu_conv_exact.py run fewer items than workgroups, so the map from a
   dealt id to an image and a tile, and the look-ahead loader of a dealt item's first stage, were only ever compared with
   themselves (forward against reversed, run against rerun).  Here each base case of tests/streams_reference.py runs at the
   item-count conditions dyn / uneven / few of test_gpu_traversal.py, forward and reversed, against the exact reference of a
   PERIODIC batch (image i = base[i % 7]); any two base images differ in at least 90 % of every tile (tests/test_streams_cpu.py),
   so a tile computed from another image's pixels fails.
B. COUNTER SETS.  ay_conv_deal_probe around every launch: only the launchers that call launch_ring(..., dynamic = true, ...) take a
   set (the RING forms of conv_fwd_16, the m16 entry, the stride-2 data gradient; expected deltas written from the code), and every
   set is zero again when the launch is over -- also after 70 launches on one stream, which wrap the rotation of 64 sets.
C-E. TWO STREAMS IN FLIGHT, two host threads, more streams than own counter sets (a child process: the table never shrinks).
F-G. bench.py's two protocols at model level -- the forward into alternating out_slots with the merge-NMS on a side stream behind
   events, and two model instances on two streams -- against the serial result of each input, and a graph replayed on another
   stream than its capture stream while a second instance runs eagerly beside it.

No test here tries to make a race happen, and none can prove that launches of two streams overlapped: the launch counts are
fixed, nothing spins or repeats until failure.  What the tests pin is that the results and the counter sets are right when the
hardware is free to overlap them."""
import ctypes as C
import os
import subprocess
import sys
import threading

import pytest
import torch

import conv_exact_reference as R
import golden_cases as gc
import streams_reference as SR
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr

pytestmark = pytest.mark.gpu
DTYPES = ["bf16", "f16"]
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def streams(dev):
    """three distinct side streams for the whole module: a stream that has dealt dynamically owns counter sets for the life of the
    process and only 16 streams can, so the tests share these instead of making their own"""
    out = []
    for _ in range(8):
        s = torch.cuda.Stream(device=dev)
        if all(s.cuda_stream != t.cuda_stream for t in out) and s.cuda_stream != torch.cuda.current_stream().cuda_stream:
            out.append(s)
        if len(out) == 3:
            break
    assert len(out) == 3
    return out


def probe(stream=None):
    """(slot, launches, nonzero_words) of ay_conv_deal_probe for a torch stream (default: the current one); synchronises the device"""
    sp = _lib.stream_ptr() if stream is None else C.c_void_p(stream.cuda_stream)
    slot, launches, nonzero = C.c_int32(-2), C.c_uint32(0), C.c_int32(-1)
    check(_lib.lib().ay_conv_deal_probe(sp, C.byref(slot), C.byref(launches), C.byref(nonzero)), "ay_conv_deal_probe")
    return slot.value, launches.value, nonzero.value


# ------------------------------------------------------------------------------------------- A (+ B around each launch)
@pytest.mark.parametrize("cond", ["dyn", "uneven", "few"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(SR.BASE_CASES))
def test_counter_dealt_items_equal_the_reference(dev, name, dtype, cond):
    """every value of a periodic batch equals the exact reference, forward and reversed; each launch takes one counter set and
    leaves all sets zero.  dyn: more than half of the items come from the counter, from the launch geometry (the form of
    test_dgrad_s2_across_items)"""
    L = _lib.lib()
    B, n_items, wgs = SR.geometry(name, cond)
    D = SR.BASE_CASES[name][5]
    print(f"{name} {cond}: batch {B}, {n_items} items, {wgs} workgroups, {max(n_items - D * wgs, 0)} items from the counter")
    if cond == "dyn":
        assert n_items >= 8 * wgs and n_items - D * wgs > n_items // 2, "most items are dealt by the counter"
    p = SR.Prepared(dev, name, 7, dtype, B)
    try:
        for rev in (0, 1):
            L.ay_conv_set_traversal(rev)
            assert L.ay_conv_get_traversal() == rev
            before = probe()
            out = p.launch()
            after = probe()
            p.verify(out, f"{cond} {'reversed' if rev else 'forward'}")
            assert after[1] - before[1] == 1, ("a dynamic launch takes one counter set", before, after)
            assert after[0] >= 0 and after[2] == 0, ("counter sets are zero after the launch", after)
    finally:
        L.ay_conv_set_traversal(0)


# ------------------------------------------------------------------------------------------- B: the other entry points
def _resblock_only(dev, dtype):
    """ay_resblock_fwd_* alone (run_resblock of test_gpu_conv_exact also runs the two ay_conv_fwd calls it replaces)"""
    import test_gpu_conv_exact as X
    case = R.RESBLOCK_CASES[0]
    Cc, H, W, B, leaky1, leaky2 = case
    r = R.resblock_reference(case, dtype)
    xb = X.blocked(dtype, r["x"], dev)
    p1, p2 = X.packed_filters(dtype, r["w1"], Cc // 2, dev), X.packed_filters(dtype, r["w2"], Cc, dev)
    s1, t1, s2, t2 = (r[k].to(dev) for k in ("scale1", "shift1", "scale2", "shift2"))
    out = X.Guarded((B, Cc // 16, H, W, 16), dtype, dev)
    check(getattr(_lib.lib(), f"ay_resblock_fwd_{dtype}")(ptr(xb), ptr(p1), ptr(s1), ptr(t1), int(leaky1), ptr(p2), ptr(s2), ptr(t2), int(leaky2),
                                                          ptr(out.t), B, Cc, H, W, _lib.stream_ptr()), "resblock")
    got = X.unblocked(dtype, out.t, Cc)
    assert out.intact()
    R.assert_same_numbers(got, r["out"], f"resblock {dtype}")


def _x(fn, *args):
    def run(dev):
        import test_gpu_conv_exact as X
        getattr(X, fn)(dev, *args)
    return run


# name: (one exact case of the entry point, counter sets it takes).  The deltas are read off the launchers: launch_dgrad_s2 calls
# launch_ring(.., true, ..); launch_ring1x1 (the route-folding and the 256-channel 1x1) calls launch_ring(.., false, ..); the fused
# block, both stems and the register-staged conv_bf16_kernel (fp32 heads, cin % 64 != 0) never reach launch_ring
OTHER_ENTRIES = {
    "dgrad-s2": (_x("run_dgrad_s2", R.DGRAD_S2_CASES[0]), 1),
    "conv1x1-cat": (_x("run_cat", R.CAT_CASES[0], "bf16"), 0),
    "resblock": (lambda dev: _resblock_only(dev, "bf16"), 0),
    "stem-s2-fused": (_x("run_stem_fused", R.STEM_FUSED_CASES[0], "bf16"), 0),
    "stem-conv": (_x("run_stem_conv", R.STEM_CONV_CASES[0], "bf16"), 0),
    "ring1x1-bn256": (_x("run_conv", (512, 256, 1, 1, 13, 40, True, False, False, 2), "bf16"), 0),
    "f32-head": (_x("run_conv", (256, 24, 1, 1, 13, 40, False, False, True, 2), "bf16"), 0),
    "conv1x1-cin48": (_x("run_conv", (48, 96, 1, 1, 40, 13, True, False, False, 2), "bf16"), 0),
}


@pytest.mark.parametrize("entry", list(OTHER_ENTRIES))
def test_only_dynamic_launches_take_a_counter_set(dev, entry):
    run, delta = OTHER_ENTRIES[entry]
    before = probe()
    run(dev)
    after = probe()
    assert after[1] - before[1] == delta, (entry, before, after)
    assert after[2] == 0, (entry, after)


def test_rotation_of_64_counter_sets_wraps(dev):
    """70 launches on one stream: the last six re-use the sets of the first six, which came back zeroed"""
    name, dtype = "m16-res", "bf16"
    B, _, _ = SR.geometry(name, "few")
    p = SR.Prepared(dev, name, 7, dtype, B)
    before = probe()
    for _ in range(70):
        out = p.launch()
    after = probe()
    p.verify(out, "launch 70")
    assert after[1] - before[1] == 70, (before, after)
    assert after[2] == 0, after


# ------------------------------------------------------------------------------------------- C: two streams
@pytest.mark.parametrize("size", ["few", "dyn"])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["m16-res", "ring3x3"])
def test_two_streams_in_flight(dev, streams, name, dtype, size):
    """Three launches on each of two streams, issued alternately without host synchronisation: the P = 7 operands on one stream,
    the P = 5 operands (other images, other filters) on the other, an output of its own per launch.  few: both launches fit on the
    device together; dyn: tails and ramps can overlap.  All six outputs exact, two different slots, three sets taken by each, all
    sets zero.  The test cannot prove that the launches overlapped; it pins the result when they may."""
    B, _, _ = SR.geometry(name, size)
    pa, pb = SR.Prepared(dev, name, 7, dtype, B), SR.Prepared(dev, name, 5, dtype, B)
    sa, sb = streams[0], streams[1]
    before = [probe(sa), probe(sb)]
    outs = []
    for k in range(3):
        for s, p in ((sa, pa), (sb, pb)):
            with torch.cuda.stream(s):
                outs.append((p, p.launch(), k))
    torch.cuda.synchronize()
    for p, out, k in outs:
        p.verify(out, f"{size} launch {k}")
    after = [probe(sa), probe(sb)]
    assert after[0][0] >= 0 and after[1][0] >= 0 and after[0][0] != after[1][0], after
    assert [a[1] - b[1] for a, b in zip(after, before)] == [3, 3], (before, after)
    assert after[1][2] == 0, after


# ------------------------------------------------------------------------------------------- D: two host threads
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["m16-res", "ring3x3"])
def test_two_host_threads(dev, streams, name, dtype):
    """the same at few size from two Python threads (ctypes releases the GIL; the current stream and the traversal direction are
    per thread): one thread launches reversed, the other forward; outputs exact, each thread reads back its own direction, the
    main thread's is still forward"""
    L = _lib.lib()
    B, _, _ = SR.geometry(name, "few")
    ps = [SR.Prepared(dev, name, 7, dtype, B), SR.Prepared(dev, name, 5, dtype, B)]
    before = [probe(streams[0]), probe(streams[1])]
    result = [None, None]
    gate = threading.Barrier(2, timeout=60)

    def work(i):
        try:
            torch.cuda.set_device(dev)
            L.ay_conv_set_traversal(1 - i)
            gate.wait()
            with torch.cuda.stream(streams[i]):
                outs = [ps[i].launch() for _ in range(3)]
            result[i] = (outs, L.ay_conv_get_traversal())
        except BaseException as exc:      # reported by the main thread
            result[i] = exc

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
        assert not t.is_alive()
    torch.cuda.synchronize()
    for i in range(2):
        assert not isinstance(result[i], BaseException), result[i]
        outs, direction = result[i]
        assert direction == 1 - i, "a thread reads back the direction it set"
        for k, out in enumerate(outs):
            ps[i].verify(out, f"thread {i} launch {k}")
    assert L.ay_conv_get_traversal() == 0, "the main thread's direction is untouched"
    after = [probe(streams[0]), probe(streams[1])]
    assert [a[1] - b[1] for a, b in zip(after, before)] == [3, 3], (before, after)
    assert after[0][0] != after[1][0] and min(after[0][0], after[1][0]) >= 0 and after[1][2] == 0, after


# ------------------------------------------------------------------------------------------- E: 18 streams
def test_more_streams_than_the_table_holds(dev):
    """a fresh process (tests/streams_child.py): 16 streams own counter sets, the 17th and 18th deal statically; all outputs exact"""
    r = subprocess.run([sys.executable, os.path.join(HERE, "streams_child.py"), "m16-res", "bf16"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("stream ")]
    assert len(lines) == 18, r.stdout
    for i, f in enumerate(lines):
        assert f[:2] == ["stream", str(i)] and f[2] == "slot" and f[4] == "launches" and f[6] == "exact", f
        slot, launches, exact = int(f[3]), int(f[5]), int(f[7])
        assert exact == 1, (f, r.stderr[-4000:])
        assert (slot, launches) == ((i, 1) if i < 16 else (-1, 0)), f
    assert [ln for ln in r.stdout.splitlines() if ln.startswith("nonzero ")] == ["nonzero 0"], r.stdout


# ------------------------------------------------------------------------------------------- F, G: model level
S_MODEL, B_MODEL, STARTS = 96, 2, (2, 3, 4)      # c3_s96_b2 of golden_cases.MODEL_CASES (start 2), pinned by test_gpu_parity.py
CONF, NMS, MAX_DET = 0.5, 0.4, 512
_second_instance = {}


def _two_models(cfg_dir, dev, precision):
    """build_models twice: the instance the other modules share, and a second one of the same weights (kept for this module)"""
    import test_gpu_parity as TP
    m1 = TP.build_models(3, cfg_dir, dev, precision)[0]
    if precision not in _second_instance:
        kept = TP._models.pop((3, precision))
        try:
            _second_instance[precision] = TP.build_models(3, cfg_dir, dev, precision)[0]
        finally:
            TP._models[(3, precision)] = kept
    return m1, _second_instance[precision]


def _inputs(dev):
    return [torch.from_numpy(gc.model_inputs(S_MODEL, B_MODEL, s)).to(dev) for s in STARTS]


def _serial(m, xs):
    """the serial result of each input on this instance: forward_device + nms_device, cloned"""
    from amyloid_yolo_paper_amd.utils import nms_device
    refs = []
    for x in xs:
        out = m.forward_device(x, out_slot=0)
        fwd = out.clone()
        refs.append((fwd, [t.clone() for t in nms_device(out, CONF, NMS, MAX_DET, 11)]))
    torch.cuda.synchronize()
    assert sum(int(r[1][2].sum()) for r in refs) > 0, "the inputs have detections"
    return refs


def _same_step(got, ref, what):
    rows, keep, count, cand = got
    r_rows, r_keep, r_count, r_cand = ref
    assert torch.equal(count, r_count) and torch.equal(cand, r_cand), (what, count.tolist(), r_count.tolist(), cand.tolist(), r_cand.tolist())
    for b in range(count.numel()):
        n = int(r_count[b])
        assert n <= MAX_DET
        assert torch.equal(rows[b, :n], r_rows[b, :n]), (what, "rows of image", b)
        assert torch.equal(keep[b, :n], r_keep[b, :n]), (what, "kept indices of image", b)


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_headline_step_of_the_benchmark(tmp_cfg_dir, dev, streams, precision):
    """bench.py's step as written there: the forward on the main stream into out_slot = k & 1, the merge-NMS on a side stream
    behind a `ready` event with slot k & 1, the main stream waiting for the slot's `done` event before it re-uses the slot; eight
    steps cycling three inputs without host synchronisation, every step equal to its input's serial result"""
    from amyloid_yolo_paper_amd.utils import nms_device
    m, _ = _two_models(tmp_cfg_dir, dev, precision)
    xs = _inputs(dev)
    refs = _serial(m, xs)
    main, side = torch.cuda.current_stream(), streams[0]
    slot_free, got = [None, None], []
    for k in range(8):
        slot = k & 1
        if slot_free[slot] is not None:
            main.wait_event(slot_free[slot])
        out = m.forward_device(xs[k % 3], out_slot=slot)
        ready = torch.cuda.Event()
        ready.record(main)
        side.wait_event(ready)
        with torch.cuda.stream(side):
            res = nms_device(out, CONF, NMS, MAX_DET, 8 + slot)
            got.append([t.clone() for t in res])
            done = torch.cuda.Event()
            done.record(side)
        slot_free[slot] = done
    torch.cuda.synchronize()
    for k, g in enumerate(got):
        _same_step(g, refs[k % 3][1], f"{precision} step {k}")
    assert probe()[2] == 0


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_two_instances_on_two_streams(tmp_cfg_dir, dev, streams, precision):
    """the two-batches-in-flight leg of bench.py --full: two instances (own arenas), each on a stream of its own running forward
    and merge-NMS back to back, eight alternating steps, each instance cycling the inputs from a different start"""
    from amyloid_yolo_paper_amd.utils import nms_device
    m1, m2 = _two_models(tmp_cfg_dir, dev, precision)
    xs = _inputs(dev)
    refs = {id(m1): _serial(m1, xs), id(m2): _serial(m2, xs)}
    arena = lambda m: m._plan(B_MODEL, S_MODEL, m._prepare(dev), dev).workspace.data_ptr()
    assert m1 is not m2 and arena(m1) != arena(m2)
    pipes = [(m1, streams[1], 8, 0), (m2, streams[2], 10, 1)]
    got = []
    for k in range(8):
        m, s, slot, start = pipes[k & 1]
        i = (start + k // 2) % 3
        with torch.cuda.stream(s):
            out = m.forward_device(xs[i], out_slot=0)
            got.append((m, i, [t.clone() for t in nms_device(out, CONF, NMS, MAX_DET, slot)]))
    torch.cuda.synchronize()
    for k, (m, i, g) in enumerate(got):
        _same_step(g, refs[id(m)][i][1], f"{precision} step {k} (instance {k & 1}, input {i})")
    assert probe()[2] == 0


def test_graph_replayed_off_its_capture_stream_beside_eager_work(tmp_cfg_dir, dev, streams):
    """The graph rule of include/amyloid_yolo.h: a captured forward keeps the counter sets of its CAPTURE stream, so it may be
    replayed on another stream as long as nothing of the library runs on the capture stream.  One capture of instance 1 on a side
    stream, two replays on the main stream while a third stream runs eager steps of instance 2; nothing runs on the capture
    stream.  Both results equal their serial references, all counter sets zero afterwards."""
    from amyloid_yolo_paper_amd import utils as ay
    m1, m2 = _two_models(tmp_cfg_dir, dev, "bf16")
    xs = _inputs(dev)
    ref1, ref2 = _serial(m1, xs), _serial(m2, xs)
    static_x = torch.zeros_like(xs[0])
    capture, eager = streams[0], streams[2]
    capture.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=capture):
        out = m1.forward_device(static_x, out_slot=0)
    torch.cuda.synchronize()
    got1, got2 = [], []
    for rep in range(2):
        static_x.copy_(xs[rep])
        ay.graph_replay(g)
        got1.append(out.clone())
        with torch.cuda.stream(eager):
            o2 = m2.forward_device(xs[rep + 1], out_slot=0)
            got2.append([t.clone() for t in ay.nms_device(o2, CONF, NMS, MAX_DET, 10)])
    torch.cuda.synchronize()
    for rep in range(2):
        assert torch.equal(got1[rep], ref1[rep][0]), f"replay {rep} differs from the serial forward"
        _same_step(got2[rep], ref2[rep + 1][1], f"eager step {rep} beside the replay")
    assert probe()[2] == 0


def test_counter_sets_are_zero_at_the_end(dev):
    """the last test of the module: no launch of it left a word of a counter set behind"""
    assert probe()[2] == 0
