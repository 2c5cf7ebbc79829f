"""Stain basis estimation (-m gpu): ay_stain_moments_u8, ay_stain_direction_hist_u8, wsi.estimate_basis, the remix map on the device
and the estimated basis downstream.  Every comparison is exact: integer words, bytes, or the float64 host results that
tests/stain_basis_reference.py (THE BASIS RULE restated in NumPy and Python integers) gives bit for bit on the same words.

Yardsticks: tests/stain_basis_reference.py for both passes, the plane and the vectors; tests/stain_reference.py with the reference's
remix tables for the mapped raster and the cut; tests/load_reference.py for the load on the estimated basis."""
import functools

import numpy as np
import pytest
import torch

import load_reference as lref
import stain_basis_reference as br
import stain_reference as sref
from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.wsi import RegionTileStream, StainBasis, StainMap, estimate_basis, normalize_region, stain_load, stain_stats, tile_grid
from test_gpu_seam import OVERLAP, S, TILE, region_raster
from test_gpu_stain import placed
from test_gpu_tissue import dark_and_bright

pytestmark = pytest.mark.gpu

GUARD = 16
PLACEMENTS = ((0, 0), (0, 7), (5, 0), (5, 7))
HAND_PLANE = ((700, -650, 300), (-600, 250, 760))              # negative components: p1 <= 0 and p2 < 0 both occur
TRUE_A, TRUE_B = ((0.60, 0.74, 0.30), (0.35, 0.60, 0.72)), ((0.55, 0.76, 0.34), (0.20, 0.50, 0.84))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def params(dev):
    p = wsi._params_to_device(wsi.basis_tables(), dev)
    assert bytes(p.cpu().numpy()) == br.odq().astype(np.int32).tobytes()
    return p


def moments_call(params, buf, stride, shape, shrink, bg, bq, out):
    return _lib.lib().ay_stain_moments_u8(ptr(buf), shape[0], shape[1], stride, shrink, bg, bq, ptr(params), ptr(out), _lib.stream_ptr())


def hist_call(params, buf, stride, shape, shrink, bg, bq, plane, out):
    return _lib.lib().ay_stain_direction_hist_u8(ptr(buf), shape[0], shape[1], stride, shrink, bg, bq, *plane[0], *plane[1], ptr(params),
                                                 ptr(out), _lib.stream_ptr())


def guarded(dev, words):
    out = torch.full((words + GUARD,), -7, device=dev, dtype=torch.int64)
    out[:words] = 0                                              # the caller zeroes what is added to
    return out


def rasters(H, W):
    one = np.empty((H, W, 3), np.uint8)
    one[:] = (150, 90, 60)                                       # every add collides: one bin, one set of moments
    prim = np.random.default_rng(H).integers(0, 2, size=(H, W, 3)).astype(np.uint8) * 255      # saturated primaries: odq at its maximum
    return {"random": dark_and_bright(H + W, H, W), "one colour": one, "primaries": prim}


def planes_of(m):
    """the planes a histogram is taken on: the hand-made one, and the reference's own where the moments have one"""
    try:
        eq1, eq2, _ = br.plane(m)
        return [HAND_PLANE, (tuple(int(v) for v in eq1), tuple(int(v) for v in eq2))]
    except ValueError:
        return [HAND_PLANE]


# ---- 1. the two kernels against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(97, 131), (200, 304)], ids=str)
def test_both_passes_word_for_word(dev, params, shape):
    both_halves = False
    for name, r in rasters(*shape).items():
        other = np.ascontiguousarray(r[::-1, ::-1] // 2 + 40)                       # the "next strip": other pixels
        bufs = [(placed(dev, r, base, pad), placed(dev, other, base, pad)) for base, pad in PLACEMENTS]
        for shrink in (1, 2):
            for bg in (0, 170, 256):
                for bq in (0, 154, 2466):
                    want, want2 = br.moments(r, shrink, bg, bq), br.moments(other, shrink, bg, bq)
                    if bg == 256 and bq == 0:
                        assert want[0] == want[1] == (shape[0] // shrink) * (shape[1] // shrink)
                    if bg == 0:
                        assert want[0] == 0 and want[1] == 0
                    planes = planes_of(want)
                    hists = [(br.direction_hist(r, shrink, bg, bq, *p), br.direction_hist(other, shrink, bg, bq, *p)) for p in planes]
                    for h, _ in hists:
                        assert h[:513].sum() == h[513] == want[1]
                    if name == "random" and bg == 256 and bq == 0:   # the hand-made plane: outside and the lower half are filled
                        assert hists[0][0][512] > 0 and (hists[0][0][:256] > 0).any() and (hists[0][0][256:512] > 0).any()
                        both_halves = True
                    for ((buf, stride), (buf2, stride2)), place in zip(bufs, PLACEMENTS):
                        runs = []
                        for _ in range(2):
                            out = guarded(dev, 11)
                            assert moments_call(params, buf, stride, r.shape, shrink, bg, bq, out) == 0
                            runs.append(out.cpu().numpy())
                        assert runs[0].tobytes() == runs[1].tobytes()                 # two runs, the same bytes
                        assert np.array_equal(runs[0][:11], want) and (runs[0][11:] == -7).all(), (name, shrink, bg, bq, place)
                        assert moments_call(params, buf2, stride2, r.shape, shrink, bg, bq, out) == 0      # a second call adds
                        got = out.cpu().numpy()
                        assert np.array_equal(got[:11], want + want2) and (got[11:] == -7).all(), (name, shrink, bg, bq, place)
                        for plane, (h, h2) in zip(planes, hists):
                            runs = []
                            for _ in range(2):
                                out = guarded(dev, 514)
                                assert hist_call(params, buf, stride, r.shape, shrink, bg, bq, plane, out) == 0
                                runs.append(out.cpu().numpy())
                            assert runs[0].tobytes() == runs[1].tobytes()
                            assert np.array_equal(runs[0][:514], h) and (runs[0][514:] == -7).all(), (name, shrink, bg, bq, place, plane)
                            assert runs[0][:513].sum() == runs[0][513] == want[1]     # bins + outside == selected == the moments' n_sel
                            assert hist_call(params, buf2, stride2, r.shape, shrink, bg, bq, plane, out) == 0
                            got = out.cpu().numpy()
                            assert np.array_equal(got[:514], h + h2) and (got[514:] == -7).all(), (name, shrink, bg, bq, place, plane)
    assert both_halves
    # 3 * 304 and 3 * 131 + 7 are multiples of 16: base 0 with those strides took the 16-byte loads, everything else the byte loads
    assert (3 * 304) % 16 == 0 and (3 * 131 + 7) % 16 == 0


def test_rows_longer_than_a_work_unit(dev, params):
    """a work unit holds 2048 48-byte items of 16 rows: rows of 120 000 bytes are walked in two units, 20 rows in two bands"""
    r = dark_and_bright(23, 20, 40000)
    assert 2048 * 48 < 3 * r.shape[1] < 2 * 2048 * 48 and 2048 * 48 < 3 * 2 * (r.shape[1] // 2)
    for shrink in (1, 2):
        want = br.moments(r, shrink, 170, 154)
        assert 2 <= want[1] < want[0] < (20 // shrink) * (40000 // shrink)
        plane = planes_of(want)[1]
        h = br.direction_hist(r, shrink, 170, 154, *plane)
        for base, pad in ((0, 0), (5, 7)):                        # 120 000 is a multiple of 16: the 16-byte loads
            buf, stride = placed(dev, r, base, pad)
            out = guarded(dev, 11)
            assert moments_call(params, buf, stride, r.shape, shrink, 170, 154, out) == 0
            assert np.array_equal(out.cpu().numpy()[:11], want), (shrink, base, pad)
            out = guarded(dev, 514)
            assert hist_call(params, buf, stride, r.shape, shrink, 170, 154, plane, out) == 0
            assert np.array_equal(out.cpu().numpy()[:514], h), (shrink, base, pad)


def test_moments_beyond_32_bits(dev, params):
    """an all-black raster: every P word is 262 144 * 6 081 156 > 2^40 -- no 32-bit sum across items or in memory survives it"""
    r = np.zeros((32, 8192, 3), np.uint8)
    n = 32 * 8192
    want = np.array([n, n] + [n * 2466] * 3 + [n * 2466 * 2466] * 6, np.int64)
    assert want[5] == 262144 * 6081156 > 2 ** 40 and np.array_equal(want, br.moments(r, 1, 220, 154))
    buf, stride = placed(dev, r, 0, 0)
    out = guarded(dev, 11)
    assert moments_call(params, buf, stride, r.shape, 1, 220, 154, out) == 0
    assert np.array_equal(out.cpu().numpy()[:11], want)
    plane = ((591, 591, 591), (724, -724, 0))                     # p2 == 0 for a grey pixel: bin 256
    out = guarded(dev, 514)
    assert hist_call(params, buf, stride, r.shape, 1, 220, 154, plane, out) == 0
    got = out.cpu().numpy()
    assert got[256] == n == got[513] and got[:513].sum() == n and np.array_equal(got[:514], br.direction_hist(r, 1, 220, 154, *plane))


def test_refusals_leave_the_outputs_untouched(dev, params):
    L, sp = _lib.lib(), _lib.stream_ptr()
    rd = torch.zeros(8, 8, 3, dtype=torch.uint8, device=dev)
    m = torch.full((16,), -7, dtype=torch.int64, device=dev)
    h = torch.full((520,), -7, dtype=torch.int64, device=dev)
    ok = ((700, 650, 300), (-600, 250, 760))
    mom = lambda stride=24, shrink=1, bg=220, bq=154, p=params, out=m: L.ay_stain_moments_u8(
        ptr(rd), 8, 8, stride, shrink, bg, bq, None if p is None else ptr(p), out if isinstance(out, int) else ptr(out), sp)
    his = lambda stride=24, shrink=1, bg=220, bq=154, plane=ok, p=params, out=h: L.ay_stain_direction_hist_u8(
        ptr(rd), 8, 8, stride, shrink, bg, bq, *plane[0], *plane[1], None if p is None else ptr(p), out if isinstance(out, int) else ptr(out), sp)
    for call in (mom, his):
        assert call(bq=2467) == -1 and call(bq=-1) == -1 and call(bg=257) == -1 and call(shrink=3) == -1 and call(stride=23) == -1
        assert call(p=None) == -1
    assert mom(out=m.data_ptr() + 4) == -1 and his(out=h.data_ptr() + 4) == -1                # not 8-byte aligned
    for bad in (((1025, 0, 0), ok[1]), (ok[0], (0, 0, -1025)), ((0, -1025, 0), ok[1])):
        assert his(plane=bad) == -1
    assert b"1024" in L.ay_last_error()
    assert L.ay_stain_moments_u8(ptr(rd), 1, 8, 24, 2, 220, 154, ptr(params), ptr(m), sp) == 0           # no halved image: AY_OK
    assert L.ay_stain_direction_hist_u8(ptr(rd), 1, 8, 24, 2, 220, 154, *ok[0], *ok[1], ptr(params), ptr(h), sp) == 0
    torch.cuda.synchronize()
    assert (m == -7).all() and (h == -7).all()
    assert his(plane=((1024, -1024, 1024), (-1024, 1024, -1024))) == 0 and mom(bq=2466) == 0 and mom(bq=0, bg=0) == 0   # the edges pass


# ---- 2. wsi.estimate_basis ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slide(vectors=TRUE_A, strength=(1.0, 1.0)):
    s = br.synthetic_slide(256, 384, vectors[0], vectors[1], 0.20, 5, strength)
    s.setflags(write=False)
    return s


def check_estimate(got, want):
    assert got.moments.dtype == np.int64 and np.array_equal(got.moments, want["moments"])
    assert got.hist.shape == (512,) and np.array_equal(got.hist, want["hist"][:512])
    assert (got.n_tissue, got.n_selected, got.outside) == (want["moments"][0], want["moments"][1], want["hist"][512])
    assert np.array_equal(got.plane[0], want["plane"][0]) and np.array_equal(got.plane[1], want["plane"][1])
    assert got.plane[0].dtype == np.int32 and got.eigenvalues == tuple(want["eigenvalues"])
    assert isinstance(got.basis, StainBasis) and np.array_equal(got.basis.M, want["M"]) and np.array_equal(got.vectors, want["vectors"])
    assert got.fell_back == want["fell_back"] and got.angle_to_prior == pytest.approx(want["angle_to_prior"], rel=1e-9)


@pytest.mark.parametrize("shrink", [1, 2])
@pytest.mark.parametrize("stride", [1, 16])
def test_estimate_basis_is_the_reference_on_the_same_view(dev, monkeypatch, stride, shrink):
    r = slide()
    view = r if stride == 1 else r[0:shrink * (256 // shrink):shrink * stride, 0:shrink * (384 // shrink):shrink * stride]
    want = br.estimate(view, shrink if stride == 1 else 1)
    assert want["moments"][1] >= (20 if stride == 16 else 1000)
    host = estimate_basis(r, shrink=shrink, probe_stride=stride)
    check_estimate(host, want)
    assert (host.alpha, host.beta) == (1.0, 154 / 1024)
    check_estimate(estimate_basis(torch.from_numpy(np.array(r)).to(dev), shrink=shrink, probe_stride=stride), want)
    if stride == 16 and shrink == 1:
        check_estimate(estimate_basis(r), want)                                       # the defaults
    for strip in (7, 40):                                                             # the result does not depend on the strips
        monkeypatch.setattr(wsi.basis, "BASIS_STRIP", strip)
        check_estimate(estimate_basis(r, shrink=shrink, probe_stride=stride), want)
        check_estimate(estimate_basis(torch.from_numpy(np.array(r)).to(dev), shrink=shrink, probe_stride=stride), want)
    monkeypatch.undo()
    other = br.estimate(view, shrink if stride == 1 else 1, beta=0.3, alpha=0.1, M=sref.basis(sref.DAB, sref.HEMATOXYLIN), max_angle=None)
    got = estimate_basis(r, shrink=shrink, probe_stride=stride, beta=0.3, alpha=0.1, prior=StainBasis(sref.DAB, sref.HEMATOXYLIN),
                         max_angle=None)
    check_estimate(got, other)
    assert (got.alpha, got.beta) == (0.1, 307 / 1024)


def test_estimate_basis_refuses_a_slide_without_a_plane(dev):
    one = np.empty((40, 56, 3), np.uint8)
    one[:] = (150, 90, 60)
    for r in (np.full((40, 56, 3), 240, np.uint8), one):
        with pytest.raises(ValueError):
            estimate_basis(r, probe_stride=1)
    with pytest.raises(ValueError):
        estimate_basis(torch.zeros(8, 8, 3, dtype=torch.uint8))                      # a tensor raster lives on the device


# ---- 3. the remix map on the device, and the estimated basis downstream -------------------------------------------------------------------
def reference_stats(r, M, basis):
    h = sref.hist(r, 1, 220, sref.tables(M=M))
    return h, wsi.StainStats(h[:1024].reshape(2, 512), int(h[1024]), basis)


def remix_case(source, target):
    """source and target rasters -> (the product's remix map from its own estimates and statistics, the reference's tables)"""
    es, et = estimate_basis(source, probe_stride=1), estimate_basis(target, probe_stride=1)
    rs, rt = br.estimate(source), br.estimate(target)
    assert np.array_equal(es.basis.M, rs["M"]) and np.array_equal(et.basis.M, rt["M"]) and es.basis != et.basis
    ss, st = stain_stats(source, probe_stride=1, basis=es.basis), stain_stats(target, probe_stride=1, basis=et.basis)
    hs, _ = reference_stats(source, rs["M"], es.basis)
    ht, _ = reference_stats(target, rt["M"], et.basis)
    assert np.array_equal(ss.hist.ravel(), hs[:1024]) and np.array_equal(st.hist.ravel(), ht[:1024])
    g = sref.gains(sref.strength(hs[:1024].reshape(2, 512), int(hs[1024]), 99.0), sref.strength(ht[:1024].reshape(2, 512), int(ht[1024]), 99.0))
    m = StainMap(ss, st, remix=True)
    assert m.gains == g and m.basis == es.basis and m.target_basis == et.basis
    return m, br.remix_tables(rs["M"], g, rt["M"])


def test_normalize_region_with_a_remix_map(dev):
    B, A = slide(TRUE_B, (0.8, 1.25)), slide()
    m, t = remix_case(B, A)
    assert bytes(m.params.cpu().numpy()) == b"".join(t[k].tobytes() for k in ("od", "D", "A", "T"))
    for shrink in (1, 2):
        want = sref.to_u8(sref.map_pixels(sref.image(B, shrink), t))
        assert np.array_equal(normalize_region(B, m, shrink=shrink), want)
    same = sref.to_u8(sref.map_pixels(B, sref.tables(m.gains, br.estimate(B)["M"])))      # the same gains without the remix: other bytes
    assert (same != sref.to_u8(sref.map_pixels(B, t))).mean() > 0.05
    gap = lambda img: float(np.abs(img.astype(np.int64) - A.astype(np.int64))[32:224, 48:336].mean())
    print(f"mean |byte difference| to slide A: raw {gap(B):.3f}, remix map {gap(normalize_region(B, m)):.3f}")
    assert gap(normalize_region(B, m)) < gap(B)


def test_stream_with_a_remix_map(dev):
    raster = region_raster()
    source, target = StainBasis(*TRUE_A), StainBasis(*TRUE_B)                          # given bases: the cut is what is tested here
    h, stats = reference_stats(raster, sref.basis(*TRUE_A), source)
    g = sref.gains(sref.strength(h[:1024].reshape(2, 512), int(h[1024]), 99.0), (1.2, 0.9))
    m = StainMap(stats, (1.2, 0.9), remix=True, target_basis=target)
    t = br.remix_tables(sref.basis(*TRUE_A), g, sref.basis(*TRUE_B))
    assert m.gains == g and bytes(m.params.cpu().numpy()) == b"".join(t[k].tobytes() for k in ("od", "D", "A", "T"))
    ty, tx, step = tile_grid(raster.shape[0], raster.shape[1], TILE, OVERLAP)
    mask = np.random.default_rng(3).random((ty, tx)) < 0.6
    assert 0 < mask.sum() < mask.size
    idx = np.flatnonzero(mask.ravel())
    want = sref.cut(raster, 1, TILE, [(int(k) % tx * step, int(k) // tx * step) for k in idx], (0,), S, t)
    got, coords = [], []
    for tiles, cs in RegionTileStream(raster, TILE, S, 1, overlap=OVERLAP, tile_mask=mask, stain=m):
        got.append(tiles.cpu())
        coords += cs
    assert coords == [(int(k) // tx, int(k) % tx) for k in idx]
    assert torch.cat(got).numpy().tobytes() == want.tobytes()


def test_stain_load_on_the_estimated_basis(dev):
    r = slide(TRUE_B)
    est, ref = estimate_basis(r, probe_stride=1), br.estimate(r)
    assert np.array_equal(est.basis.M, ref["M"]) and est.basis != wsi.H_DAB
    got = stain_load(r, cell=64, basis=est.basis)
    cells, _, _ = lref.load(r, 1, 220, sref.tables(M=ref["M"]), 1, lref.thres_bin(0.15), 64)
    for i, key in enumerate(("tissue", "positive", "bin_sum")):
        assert np.array_equal(got[key], cells[:, :, i]), key
    fixed = stain_load(r, cell=64)
    assert np.array_equal(fixed["tissue"], got["tissue"]) and not np.array_equal(fixed["positive"], got["positive"])
