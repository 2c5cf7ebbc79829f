"""Plaque segmentation (-m gpu): ay_box_segments_u8, wsi.segment_boxes, wsi.quantify_region(segment=True).  Every comparison is exact:
integers, or bytes.  Yardstick: tests/segment_reference.py (THE SEGMENT RULE restated in NumPy with a plain flood fill, on
load_reference's pixel classes).  Guard words of -7 sit behind `out`; `out` is never zeroed first: a call writes every word of the rows it
owns and no other."""
import numpy as np
import pytest
import torch

import load_reference as lr
import segment_reference as sr
import stain_reference as sref
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import StainMap, plaque_morphometry, quantify_region, segment_boxes
from test_gpu_load import PLACEMENTS, hand_rows
from test_gpu_seam import BATCH, CONF, NMS, S, TILE, build_model, region_raster
from test_gpu_stain import placed

pytestmark = pytest.mark.gpu

GUARD = 16
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


IDENTITY = StainMap.identity()        # kept alive: its params tensor is what the calls read


def fresh(dev, M):
    """M rows of 20 words and GUARD words behind them, all -7: what a call does not own keeps it"""
    return torch.full((M * sr.COLS + GUARD,), -7, device=dev, dtype=torch.int32)


def device_segments(dev, r, shrink, rows, margin, min_area=1, origin=(0, 0), slide=None, own=None, base=0, pad=0, out=None, flags=None,
                    j=sr.THRES_BIN, core=sr.CORE_BIN):
    """one call on the region r at `origin` of the slide -> (words int64 [M, 20], flags); `out` / `flags`: tensors to go on writing into"""
    H, W = r.shape[0] // shrink, r.shape[1] // shrink
    slide = slide or (H, W)
    own = own or (0, slide[0])
    M = len(rows)
    out = fresh(dev, M) if out is None else out
    flags = torch.tensor([0, -7], device=dev, dtype=torch.int32) if flags is None else flags
    buf, stride = placed(dev, r, base, pad)
    d_rows = torch.from_numpy(np.ascontiguousarray(rows)).to(dev)
    check(_lib.lib().ay_box_segments_u8(ptr(buf), r.shape[0], r.shape[1], stride, shrink, origin[0], origin[1], slide[0], slide[1], own[0],
                                        own[1], sr.BG, ptr(IDENTITY.params), 1, j, core, margin, min_area,
                                        ptr(d_rows), M, ptr(out), ptr(flags), _lib.stream_ptr()),
          "ay_box_segments_u8")
    got = out.cpu().numpy().astype(np.int64)
    assert (got[M * sr.COLS:] == -7).all() and flags[1].item() == -7          # the guard words
    return got[:M * sr.COLS].reshape(M, sr.COLS), int(flags[0].item())


def reference(r, shrink, rows, margin, min_area=1):
    out, flags = sr.segment(r, shrink, sr.BG, sref.tables(), 1, sr.THRES_BIN, sr.CORE_BIN, margin, min_area, rows)
    return out, int(flags[0])


def test_the_colours_have_the_bins_the_tests_rely_on():
    px = np.asarray([[sr.POSITIVE, sr.CORE, sr.NEGATIVE, sr.GLASS]], np.uint8)
    t, q = lr.classes(px, 1, sr.BG, sref.tables(), 1)
    assert t.tolist() == [[True, True, True, False]] and q[0, :3].tolist() == [44, 69, 0]


# ---- 1. painted shapes through the C ABI ------------------------------------------------------------------------------------------------
SIZE_ROWS = np.asarray([sr.row(20 + 3 * i, 30 + k, 20 + 3 * i + w, 30 + k + h) for i, w in enumerate((1, 31, 32, 33, 63, 64, 65, 255))
                        for k, h in enumerate((1, 2, 255))], np.float32)


@pytest.fixture(scope="module")
def painted():
    """per shrink: [(name, raster, rows, margin, min_area, want, want_flags)], the reference computed once"""
    worst, worst_rows = sr.worst_slide()
    hand, hand_core, hand_rows_, _ = sr.hand_slide()
    cases = {}
    for shrink in (1, 2):
        blobs, _ = sr.blob_raster(300, 300, 11, shrink)
        cases[shrink] = []
        for name, r, rows, margin, min_area in (("worst", sr.paint(worst, None, None, shrink), worst_rows, sr.WORST_MARGIN, 1),
                                                ("sizes", blobs, SIZE_ROWS, 0, 1),
                                                ("hand", sr.paint(hand, hand_core, None, shrink), hand_rows_, sr.HAND_MARGIN, 1),
                                                ("hand, min_area 10", sr.paint(hand, hand_core, None, shrink), hand_rows_, sr.HAND_MARGIN, 10),
                                                ("hand, margin 0", sr.paint(hand, hand_core, None, shrink), hand_rows_, 0, 1)):
            cases[shrink].append((name, r, rows, margin, min_area) + reference(r, shrink, rows, margin, min_area))
    return cases


@pytest.mark.parametrize("shrink", [1, 2])
def test_painted_shapes_against_the_reference(dev, painted, shrink):
    """the smallest and the worst windows: widths 1, 31 .. 33, 63 .. 65, 255 and heights 1, 2, 255 on blobs; 255 x 255 full (area 65 025,
    perimeter 1 020), checkerboard (ONE component of 32 513), every other pixel (16 384 components, the first candidate wins), a
    one-pixel spiral, a serpentine, a comb, a diagonal, two equal blobs; a 256-wide window (LARGE); the margin cases and the corner
    boxes of the CPU file.  Four placements: both load paths.  Two runs give the same bytes; AY_SEG_INTERNAL never appears."""
    for name, r, rows, margin, min_area, want, want_flags in painted[shrink]:
        if name == "worst":
            got = dict(zip(sr.WORST, want.tolist()))
            assert got["full"][5:11] == [65025, 1, 65025, 0, 65025 * 44, 1020] and got["checkerboard"][5:8] == [32513, 1, 32513]
            assert got["every other"][5:8] == [16384, 28 * 28, 1] and got["spiral"][5:8] == got["serpentine"][5:8] == [32767, 1, 32767]
            assert want[-1, 0] == sr.LARGE and want_flags == sr.LARGE
        if name == "sizes":
            assert sorted(set(want[:, 3])) == [1, 31, 32, 33, 63, 64, 65, 255] and sorted(set(want[:, 4])) == [1, 2, 255]
            assert (want[:, 7] > 0).sum() >= 12 and (want[:, 0] == 0).all()
        for base, pad in PLACEMENTS:
            runs = [device_segments(dev, r, shrink, rows, margin, min_area, base=base, pad=pad) for _ in range(2)]
            assert runs[0][0].tobytes() == runs[1][0].tobytes(), (name, base, pad)
            got, flags = runs[0]
            assert not (got[:, 0] & sr.INTERNAL).any() and not flags & sr.INTERNAL, name
            bad = np.flatnonzero((got != want).any(1))
            assert len(bad) == 0, (name, base, pad, bad[:5], got[bad[:2]], want[bad[:2]])
            assert flags == want_flags, name


# ---- 2. random boxes against the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shrink", [1, 2])
def test_random_boxes_on_one_region_and_on_uneven_owned_ranges(dev, shrink):
    r, rows, short = sr.random_case(shrink, hand_rows(300, 260))
    H, W, M, margin = 300, 260, len(rows), sr.RANDOM_MARGIN
    want, want_flags = reference(r, shrink, rows, margin)
    sr.assert_random_counts(want, np.asarray([want_flags]))            # the inputs show what they are meant to, on the reference alone
    got, flags = device_segments(dev, r, shrink, rows, margin, base=5, pad=7)
    assert got.tobytes() == want.tobytes() and flags == want_flags and not flags & sr.INTERNAL
    # uneven owned ranges on overlapping regions that just hold their windows; the outputs are written piece by piece
    _, _, win, owner = sr.windows(rows, H, W, margin)
    out, fl = fresh(dev, M), torch.tensor([0, -7], device=dev, dtype=torch.int32)
    bounds = [0, 100, 101, 250, H]
    for a, b in zip(bounds[:-1], bounds[1:]):
        mine = (owner >= a) & (owner < b) & (want[:, 0] == 0)
        lo, hi = (a, max(int((win[mine, 1] + win[mine, 3]).max()), a + 1)) if mine.any() else (a, a + 1)
        got, flags = device_segments(dev, r[lo * shrink:hi * shrink], shrink, rows, margin, origin=(lo, 0), slide=(H, W), own=(a, b), out=out, flags=fl)
        theirs = (owner < a) | (owner >= b)
        assert (got[theirs & (owner >= b)] == -7).all()               # rows of a later call: untouched so far
    assert got.tobytes() == want.tobytes() and flags == want_flags
    # a region deliberately short, and one that starts at column 30: NOT_RESIDENT where the reference says so, the rest as before
    for region, origin in ((r[:short * shrink], (0, 0)), (np.ascontiguousarray(r[40 * shrink:, 30 * shrink:230 * shrink]), (40, 30))):
        t, q = lr.classes(region, shrink, sr.BG, sref.tables(), 1)
        ref, ref_f = np.full((M, sr.COLS), -1, np.int64), np.zeros(1, np.int64)
        sr.add_classes(t, q, origin[0], origin[1], H, W, (0, H), sr.THRES_BIN, sr.CORE_BIN, margin, 1, rows, ref, ref_f)
        assert (ref[:, 0] == sr.NOT_RESIDENT).sum() >= 1 and ((ref[:, 0] == 0) & (ref[:, 7] > 0)).sum() >= 20
        got, flags = device_segments(dev, region, shrink, rows, margin, origin=origin, slide=(H, W))
        assert got.tobytes() == ref.tobytes() and flags == int(ref_f[0])
    # other thresholds and min_area: the positive colour is core too; nothing is positive
    for j, core, min_area in ((44, 44, 5), (70, 512, 1)):
        ref, ref_f = sr.segment(r, shrink, sr.BG, sref.tables(), 1, j, core, margin, min_area, rows)
        got, flags = device_segments(dev, r, shrink, rows, margin, min_area, j=j, core=core)
        assert got.tobytes() == ref.tobytes() and flags == int(ref_f[0]), (j, core, min_area)
    assert (ref[:, 5] == 0).all()                                     # bin 70: nothing is positive


# ---- 3. a captured HIP graph ----------------------------------------------------------------------------------------------------------
def test_hip_graph_of_one_call_replays_on_other_rows(dev):
    """one call captured on one stream (no side branches) and replayed onto other rows: launches only"""
    r, _ = sr.blob_raster(200, 180, 21)
    H, W, M, margin = 200, 180, 90, 8
    inputs = [lr.random_boxes(M, H, W, 80 + k) for k in range(3)]
    rd = torch.from_numpy(r).to(dev)
    rows = torch.from_numpy(inputs[0]).to(dev)
    params = IDENTITY.params
    out = torch.full((M, sr.COLS), -7, device=dev, dtype=torch.int32)
    flags = torch.zeros(1, device=dev, dtype=torch.int32)

    def step():
        check(_lib.lib().ay_box_segments_u8(ptr(rd), H, W, W * 3, 1, 0, 0, H, W, 0, H, sr.BG, ptr(params), 1, sr.THRES_BIN, sr.CORE_BIN, margin, 1,
                                            ptr(rows), M, ptr(out), ptr(flags), _lib.stream_ptr()), "ay_box_segments_u8")

    step()                                                            # eager once (loads the code objects)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    for k in (1, 2, 0, 1):
        out.fill_(-7)
        flags.zero_()
        rows.copy_(torch.from_numpy(inputs[k]))
        g.replay()
        torch.cuda.synchronize()
        want, want_f = reference(r, 1, inputs[k], margin)
        assert ((want[:, 0] == 0) & (want[:, 7] > 0)).sum() >= 30
        np.testing.assert_array_equal(out.cpu().numpy(), want)
        assert int(flags.item()) == want_f


# ---- 4. bad arguments through the C ABI -----------------------------------------------------------------------------------------------
def test_bad_arguments_return_minus_one_and_leave_the_outputs_alone(dev):
    L, params, sp = _lib.lib(), IDENTITY.params, _lib.stream_ptr()
    rd = torch.full((32, 32, 3), 90, dtype=torch.uint8, device=dev)
    rows = torch.tensor([[8, 8, 24, 24, 1, 1, 0]], dtype=torch.float32, device=dev)
    out = torch.full((sr.COLS + 1,), 77, dtype=torch.int32, device=dev)
    flags = torch.full((1,), 77, dtype=torch.int32, device=dev)
    good = dict(region=ptr(rd), h=32, w=32, stride=96, shrink=1, oy=0, ox=0, sh=32, sw=32, own0=0, own1=32, bg=220, params=ptr(params), stain=1,
                j=10, core=64, margin=4, min_area=1, rows=ptr(rows), n=1, out=ptr(out), flags=ptr(flags))
    call = lambda **kw: L.ay_box_segments_u8(*{**good, **kw}.values(), sp)
    for bad in (dict(region=None), dict(params=None), dict(h=0), dict(w=0), dict(stride=95), dict(shrink=0), dict(shrink=3), dict(bg=-1),
                dict(bg=257), dict(stain=-1), dict(stain=2), dict(j=-1), dict(j=513, core=513), dict(core=513), dict(j=11, core=10),
                dict(margin=-1), dict(margin=128), dict(min_area=0), dict(min_area=-5), dict(oy=-1), dict(ox=-1), dict(oy=1), dict(ox=1),
                dict(sh=31, own1=31), dict(sw=31), dict(sh=0, own1=0), dict(sw=(1 << 24) + 1), dict(sh=(1 << 24) + 1), dict(shrink=2, sh=15, own1=15),
                dict(own0=-1), dict(own0=5, own1=4), dict(own1=33), dict(n=-1), dict(rows=None), dict(out=None), dict(flags=None)):
        assert call(**bad) == -1, bad
        assert _lib.lib().ay_last_error()
    torch.cuda.synchronize()
    assert (out == 77).all() and (flags == 77).all()
    assert call(n=0) == 0 and call(n=0, rows=None, out=None, flags=None) == 0 and call(own0=5, own1=32) == 0       # nothing owned
    torch.cuda.synchronize()
    assert (out == 77).all() and (flags == 77).all()
    # the good call is good: every pixel is tissue of bin q, one component fills the 24 x 24 window
    t, q = lr.classes(np.full((1, 1, 3), 90, np.uint8), 1, 220, sref.tables(), 1)
    assert t.all() and q[0, 0] >= 10
    core = 576 if q[0, 0] >= 64 else 0
    assert call() == 0
    assert out.tolist() == [0, 4, 4, 24, 24, 576, 1, 576, core, 576 * int(q[0, 0]), 96, 576 * 23 // 2, 576 * 23 // 2, 4, 4, 28, 28, 15, 256, 0, 77]
    assert flags.item() == 77
    assert call(shrink=2, sh=16, sw=16, own1=16, margin=127) == 0      # the halved image: one 16 x 16 window, touching all four sides
    assert out.tolist()[:8] == [0, 0, 0, 16, 16, 256, 1, 256] and out[17].item() == 15 and out[18].item() == 64 and out[20].item() == 77


# ---- 5. wsi.segment_boxes ---------------------------------------------------------------------------------------------------------------
def test_segment_boxes_through_the_stream(dev):
    raster = region_raster()
    H, W = raster.shape[:2]
    assert H > 255
    rows = np.concatenate([hand_rows(H, W), lr.random_boxes(150, H, W, 5)])
    want, want_f = sr.segment(raster, 1, 220, sref.tables(), 1, 10, 64, 8, 1, rows)
    assert ((want[:, 0] == 0) & (want[:, 7] > 0)).sum() >= 10 and want_f[0] == sr.NONFINITE | sr.EMPTY | sr.LARGE
    got = {strip: segment_boxes(raster, rows, core_thres=1.0, strip=strip) for strip in (255, 300, 2048)}
    for strip, g in got.items():
        assert g["segments"].dtype == np.int32 and g["segments"].shape == (len(rows), 20)
        assert np.array_equal(g["segments"], want) and g["flags"] == int(want_f[0]), strip
        assert g["thres"] == 10 / 64 and g["core_thres"] == 1.0 and g["strips"][1] == len(sr.strip_plan(H, strip)) and g["strips"][0] >= 1
        assert sorted(g) == ["core_thres", "flags", "segments", "strips", "thres"]
    assert got[255]["strips"][1] == H - 254 and got[2048]["strips"] == (1, 1)
    # rows on the device; a non-contiguous view of a wider raster, other arguments
    on_dev = segment_boxes(raster, torch.from_numpy(rows).to(dev), core_thres=1.0, strip=300)
    assert np.array_equal(on_dev["segments"], want)
    wide = np.concatenate([raster, 255 - raster], 1)
    view = wide[:, 5:5 + W]
    assert not view.flags["C_CONTIGUOUS"]
    ref, ref_f = sr.segment(np.ascontiguousarray(view), 1, 200, sref.tables(), 0, lr.thres_bin(0.4), 512, 3, 4, rows)
    g = segment_boxes(view, rows, margin=3, bg_level=200, thres=0.4, stain=0, min_area=4, strip=256)
    assert np.array_equal(g["segments"], ref) and g["flags"] == int(ref_f[0]) and g["core_thres"] == 8.0 and ((ref[:, 0] == 0) & (ref[:, 7] > 0)).sum() >= 5
    # shrink 2 on a tall raster: windows across the strip cuts; detections confined to the top upload one strip
    tall, tie = sr.blob_raster(700, 60, 9, 2)
    step = 300 - 254
    near_top = np.asarray([sr.row(5, 20, 25, 35), sr.row(30, 2, 50, 30), sr.row(10, 10, 14, 14)], np.float32)
    rows2 = np.concatenate([tie, near_top, lr.random_boxes(90, 700, 60, 6, cuts=tuple(range(step, 700 - 254, step)))])
    ref, ref_f = sr.segment(tall, 2, sr.BG, sref.tables(), 1, sr.THRES_BIN, sr.CORE_BIN, 8, 1, rows2)
    _, _, win, owner = sr.windows(rows2, 700, 60, 8)
    plan = sr.strip_plan(700, 300)
    crossing = sum(1 for y, h in zip(win[:, 1], win[:, 3]) if h and any(y < p[2] < y + h for p in plan[1:]))
    assert crossing >= 10 and ((ref[:, 0] == 0) & (ref[:, 7] > 0)).sum() >= 40
    for strip in (255, 300, 2048):
        g = segment_boxes(tall, rows2, shrink=2, core_thres=1.0, strip=strip)
        assert np.array_equal(g["segments"], ref) and g["flags"] == int(ref_f[0]), strip
    assert g["strips"] == (1, 1) and segment_boxes(tall, rows2, shrink=2, strip=300)["strips"][1] == len(plan) > 1
    top = rows2[(win[:, 1] + win[:, 3] <= step) & (win[:, 3] > 0)]
    assert len(top) >= 3
    g = segment_boxes(tall, top, shrink=2, core_thres=1.0, strip=300)
    assert g["strips"] == (1, len(plan)) and np.array_equal(g["segments"], ref[(win[:, 1] + win[:, 3] <= step) & (win[:, 3] > 0)])
    assert segment_boxes(tall, np.zeros((0, 7), np.float32), shrink=2)["segments"].shape == (0, 20)


# ---- 6. quantify_region(segment=True) ---------------------------------------------------------------------------------------------------
def test_quantify_region_with_segment(tmp_cfg_dir, dev):
    model = build_model(3, tmp_cfg_dir, dev, "bf16")
    raster = region_raster()
    H, W = raster.shape[:2]
    kw = dict(cell=32, field=3, top_k=4, tile=TILE, img_size=S, conf_thres=CONF, nms_thres=NMS, batch_size=BATCH)
    base = quantify_region(model, raster, **kw)
    assert sorted(base) == sorted(["rows", "counts", "tissue", "fields", "n_found", "totals", "below", "flagged", "flags"])
    got = quantify_region(model, raster, dab_thres=0.15, segment=True, core_thres=1.0, seg_margin=6, **kw)
    assert sorted(got) == sorted(list(base) + ["segments", "segment_flags", "plaque", "class_area_px"])
    assert torch.equal(got["rows"], base["rows"]) and np.array_equal(got["fields"], base["fields"]) and len(got["rows"]) >= 12
    assert all(np.array_equal(got[k], base[k]) for k in ("tissue", "n_found", "totals")) and torch.equal(got["counts"], base["counts"])
    rows = got["rows"].cpu().numpy()
    sg = segment_boxes(raster, got["rows"], margin=6, thres=0.15, core_thres=1.0)
    want, want_f = sr.segment(raster, 1, 220, sref.tables(), 1, 10, 64, 6, 1, rows)
    assert np.array_equal(got["segments"], sg["segments"]) and np.array_equal(sg["segments"], want) and got["segment_flags"] == sg["flags"] == int(want_f[0])
    pm = plaque_morphometry(sg["segments"], None, (H, W))
    assert sorted(got["plaque"]) == sorted(pm) and all(np.array_equal(got["plaque"][k], pm[k], equal_nan=True) for k in pm)
    assert ((want[:, 0] == 0) & (want[:, 7] > 0)).sum() >= 3
    conf = float(np.sort(rows[:, 4])[len(rows) // 2])                 # a bound that drops about half of the rows; exact in fp32
    above = quantify_region(model, raster, dab_thres=0.15, segment=True, core_thres=1.0, seg_margin=6, min_conf=conf, **kw)
    assert np.array_equal(above["segments"], got["segments"])        # min_conf selects rows for the quartiles, never for the pass
    for res, bound in ((got, 0.0), (above, conf)):
        quart = np.full((3, 3), NAN)                                  # the host recomputation
        for c in range(3):
            a = [float(w[7]) for w, r in zip(want, rows) if w[0] == 0 and w[7] > 0 and r[4] >= bound and r[6] == c]
            if a:
                quart[c] = np.percentile(np.asarray(a), [25, 50, 75])
        assert res["class_area_px"].shape == (3, 3) and res["class_area_px"].dtype == np.float64
        np.testing.assert_array_equal(res["class_area_px"], quart)
    # with load and mpp as well: the keys of both, the areas in microns
    both = quantify_region(model, raster, dab_thres=0.15, load=True, segment=True, mpp=0.5, **kw)
    assert {"box_load", "segments", "plaque", "class_area_px", "density_per_mm2"} <= set(both) and "area_um2" in both["plaque"]
    np.testing.assert_array_equal(both["plaque"]["area_um2"], both["plaque"]["area_px"] * 0.25)
