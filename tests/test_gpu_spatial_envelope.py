"""Random-labelling simulations for the spatial statistics (-m gpu): ay_pair_counts_relabel through wsi.pair_counts_relabel_device,
wsi.spatial_envelope and quantify_region(spatial_envelope=...).  Every output is compared byte for byte: THE RELABEL RULE is integer
sums over THE PAIR RULE's geometry.

Yardstick: tests/spatial_envelope_reference.py (one brute-force enumeration of all pairs, a bincount per simulation; for tiny cases
the plain rule on relabelled rows)."""
import ctypes as C

import numpy as np
import pytest
import torch

import spatial_envelope_reference as er
import spatial_reference as sr
import spatial_window_reference as swr
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd._lib import ptr
from amyloid_yolo_paper_amd.wsi import pair_counts_device, pair_counts_relabel_device, quantify_region, spatial_envelope, spatial_stats

pytestmark = pytest.mark.gpu

H, W, NC = sr.SLIDE_H, sr.SLIDE_W, sr.CLASSES
NAMES = ("sim_pairs", "sim_centres", "sim_inside", "bd", "stats")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def run(dev, rows, H_, W_, C_, min_conf, rq, tab, roi=None, border=True, cell_side=0, mask=None, cell=0):
    t = torch.from_numpy(np.array(rows, np.float32)).reshape(-1, 7).to(dev)      # (a copy: the shared cases are read-only)
    m = None if mask is None else torch.from_numpy(np.array(mask, np.uint8)).to(dev)
    out = pair_counts_relabel_device(t, (H_, W_), rq, C_, np.array(tab, np.uint8), min_conf, roi, border, cell_side, m, cell)
    torch.cuda.synchronize()
    return tuple(out[k].cpu().numpy() for k in NAMES)


def assert_same(got, want, what=""):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        np.testing.assert_array_equal(g, w, err_msg=f"{what} {name}")
        assert g.tobytes() == w.tobytes(), (what, name)


def against_the_reference(dev, rows, H_, W_, C_, min_conf, rq, tab, roi=None, border=True, cell_side=0, mask=None, cell=0, what=""):
    want = er.sim_counts(rows, H_, W_, C_, min_conf, rq, tab, roi, border, mask, cell)
    assert_same(run(dev, rows, H_, W_, C_, min_conf, rq, tab, roi, border, cell_side, mask, cell), want, what)
    return want


def table_of(rows, H_, W_, C_, min_conf, n_sim, seed):
    return er.table(sr.positions(rows, H_, W_, C_, min_conf)[2], C_, n_sim, seed)


# ---- 1. sizes: rows and simulations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", er.ROW_SIZES)
def test_clustered_case_against_the_restatement(dev, M):
    rows, rq, tab, want = er.clustered_sims(M)                  # (the case's not-idle assertions ran on the restatement)
    for S in er.SIM_SIZES if M in (257, 4097) else (1, 65):
        assert_same(run(dev, rows, H, W, NC, 0.5, rq, tab[:, :S]), er.first(want, S), f"M={M} S={S}")


def test_column_0_is_the_plain_call_byte_for_byte(dev):
    rows, rq, tab, _ = er.clustered_sims(4097)
    t = torch.from_numpy(rows.copy()).to(dev)
    plain = pair_counts_device(t, (H, W), rq, NC, 0.5)
    got = run(dev, rows, H, W, NC, 0.5, rq, tab[:, :70])
    torch.cuda.synchronize()
    assert got[0][0].tobytes() == plain["pairs"].cpu().numpy().tobytes() and got[1][0].tobytes() == plain["centres"].cpu().numpy().tobytes()
    assert got[3].tobytes() == plain["bd"].cpu().numpy().tobytes() and got[4].tobytes() == plain["stats"].cpu().numpy().tobytes()
    np.testing.assert_array_equal(got[2][0], plain["stats"].cpu().numpy()[NC:2 * NC])
    # with a mask: the window call's
    rows, rq, mask, _ = swr.ragged_case(1025)
    tab = table_of(rows, swr.SLIDE_H, swr.SLIDE_W, swr.CLASSES, 0.5, 5, 2)
    t, m = torch.from_numpy(rows.copy()).to(dev), torch.from_numpy(mask.copy()).to(dev)
    plain = pair_counts_device(t, (swr.SLIDE_H, swr.SLIDE_W), rq, swr.CLASSES, 0.5, None, True, 0, m, swr.CELL)
    got = run(dev, rows, swr.SLIDE_H, swr.SLIDE_W, swr.CLASSES, 0.5, rq, tab, mask=mask, cell=swr.CELL)
    assert got[0][0].tobytes() == plain["pairs"].cpu().numpy().tobytes() and got[1][0].tobytes() == plain["centres"].cpu().numpy().tobytes()
    assert got[3].tobytes() == plain["bd"].cpu().numpy().tobytes() and got[4].tobytes() == plain["stats"].cpu().numpy().tobytes()
    assert got[0][0].sum() > 0


def test_sums_over_the_classes_do_not_depend_on_the_simulation(dev):
    rows, rq, tab, _ = er.clustered_sims(4097)
    sp, sc, si, _, _ = run(dev, rows, H, W, NC, 0.5, rq, tab[:, :100])
    total, centres = sp.sum(axis=(1, 2)), sc.sum(axis=1)
    assert (total == total[0]).all() and (centres == centres[0]).all() and total[0].min() > 0 and (si.sum(1) == si[0].sum()).all()
    assert (sp[1:] != sp[0]).any()
    # a table in which every column is the observed one: S identical blocks
    same = np.repeat(tab[:, :1], 67, axis=1)
    sp, sc, si, _, _ = run(dev, rows, H, W, NC, 0.5, rq, same)
    for v in (sp, sc, si):
        assert (v == v[0]).all()
    assert sp[0].tobytes() == er.first(er.clustered_sims(4097)[3], 1)[0][0].tobytes()


# ---- 2. the paths of the LDS plan -----------------------------------------------------------------------------------------------------
def test_shapes_of_every_path(dev):
    """C = 8, B = 32: a column of 256 entries holds ONE centre class, eight passes, and the centres kernel takes 32 simulations;
    C = 5, B = 16: three centre classes a pass, two passes, the last with two; C = 4, B = 16: one pass, one wavefront a workgroup;
    C = 3, B = 1: one pass, four wavefronts; C = 2, B = 32: one pass, two wavefronts"""
    many = sr.clustered_rows(1200, 17, C=8)
    rq = sr.radii_q(40 + 8 * np.arange(32))
    want = against_the_reference(dev, many, H, W, 8, 0.5, rq, table_of(many, H, W, 8, 0.5, 69, 3), what="C = 8, B = 32")
    assert want[0].shape == (70, 8, 8, 32) and want[0][:, :, :, -1].min() > 0 and (np.diff(want[1], axis=2) < 0).any()
    rows = sr.clustered_rows(900, 18, C=5)
    against_the_reference(dev, rows, H, W, 5, 0.5, sr.radii_q(16 * (1 + np.arange(16))), table_of(rows, H, W, 5, 0.5, 64, 4), what="C = 5, B = 16")
    rows = sr.clustered_rows(900, 19, C=4)
    against_the_reference(dev, rows, H, W, 4, 0.5, sr.radii_q(16 * (1 + np.arange(16))), table_of(rows, H, W, 4, 0.5, 3, 5), what="C = 4, B = 16")
    rows = sr.clustered_case(257)[0]
    want = against_the_reference(dev, rows, H, W, 3, 0.5, sr.radii_q((64,)), table_of(rows, H, W, 3, 0.5, 65, 6), what="C = 3, B = 1")
    assert want[0].min() > 0
    against_the_reference(dev, rows, H, W, 2, 0.5, sr.radii_q(8 * (1 + np.arange(32))), table_of(rows, H, W, 2, 0.5, 2, 7), what="C = 2, B = 32")


# ---- 3. the window --------------------------------------------------------------------------------------------------------------------
def test_border_roi_and_mask(dev):
    rows, rq, tab, _ = er.clustered_sims(257)
    tab = tab[:, :66]
    against_the_reference(dev, rows, H, W, NC, 0.5, rq, tab, None, False, what="without border")
    roi = sr.roi_q((300.0, 200.5, 3800.25, 2900.0), H, W)
    for border in (True, False):
        want = against_the_reference(dev, rows, H, W, NC, 0.5, rq, tab, roi, border, what=f"roi border={border}")
        assert (want[2] < want[4][:NC]).any()                            # rows outside the window are counted, but not inside
    rows, rq, mask, plain = swr.ragged_case(1025)                        # a mask with holes
    Hs, Ws, Cs = swr.SLIDE_H, swr.SLIDE_W, swr.CLASSES
    tab = table_of(rows, Hs, Ws, Cs, 0.5, 65, 8)
    for border in (True, False):
        want = against_the_reference(dev, rows, Hs, Ws, Cs, 0.5, rq, tab, None, border, 0, mask, swr.CELL, what=f"mask border={border}")
    roi = sr.roi_q((100, 90, 900, 700), Hs, Ws)
    want = against_the_reference(dev, rows, Hs, Ws, Cs, 0.5, rq, tab, roi, True, 0, mask, swr.CELL, what="mask and roi")
    assert want[0].min() > 0 and (want[0][1:] != want[0][0]).any()
    np.testing.assert_array_equal(er.sim_counts(rows, Hs, Ws, Cs, 0.5, rq, tab[:, :1], None, True, mask, swr.CELL)[0][0], plain[0])


# ---- 4. equality, duplicates, a dense cell --------------------------------------------------------------------------------------------
def test_duplicates_and_pairs_at_exactly_the_radius(dev):
    rows = sr.points([[100.25, 50.5]] * 100, cls=np.arange(100) % 3)
    want = against_the_reference(dev, rows, 200, 300, 3, 0.0, sr.radii_q((0.25, 2)), table_of(rows, 200, 300, 3, 0.0, 64, 1), what="duplicates")
    assert (want[0].sum(axis=(1, 2)) == 100 * 99).all() and want[0][0, 0, 0, 0] == 34 * 33
    rows = sr.lattice_rows(16, 1.0, C=2, side=6.0, x0=20.0, y0=24.0)       # 3-4-5 and 5-12-13 pairs at exactly R_k
    tab = table_of(rows, 64, 64, 2, 0.0, 65, 2)
    for border in (False, True):
        at = against_the_reference(dev, rows, 64, 64, 2, 0.0, sr.radii_q((5, 13)), tab, None, border, what="at the radius")
        short = against_the_reference(dev, rows, 64, 64, 2, 0.0, sr.radii_q((4.75, 13)), tab, None, border, what="a quarter pixel shorter")
    qx, qy = sr.positions(rows, 64, 64, 2, 0.0)[:2]
    d2 = (qx[:, None] - qx[None, :]) ** 2 + (qy[:, None] - qy[None, :]) ** 2
    assert (d2 == 20 * 20).sum() >= 100 and (at[0][:, :, :, 0].sum(axis=(1, 2)) > short[0][:, :, :, 0].sum(axis=(1, 2))).all()


def test_a_dense_cell(dev):
    """700 rows inside one 256-px cell: every centre meets ten times the partners of one step of 64 lanes"""
    rng = np.random.default_rng(5)
    xy = np.round(rng.uniform([1024 + 1, 1280 + 1], [1280 - 1, 1536 - 1], (700, 2)) * 8) / 8
    rows = sr.points(xy, cls=rng.integers(0, 3, 700))
    rq = sr.radii_q(sr.RADII_PX)
    want = against_the_reference(dev, rows, H, W, NC, 0.0, rq, table_of(rows, H, W, NC, 0.0, 65, 9), what="a dense cell")
    assert want[0].min() > 0 and want[0][:, :, :, -1].sum(axis=(1, 2)).min() > 400 * 700


# ---- 5. bad table values --------------------------------------------------------------------------------------------------------------
def test_bad_table_values(dev):
    rows, rq, tab, res = er.clustered_sims(257)
    cls = sr.positions(rows, H, W, NC, 0.5)[2]
    counted, other = np.flatnonzero(cls >= 0), np.flatnonzero(cls < 0)
    assert len(other) >= 5
    tab = tab[:, :70].copy()
    junk = tab.copy()
    junk[other] = np.random.default_rng(1).integers(0, 256, (len(other), 70))       # garbage on rows that are not counted: nothing changes
    assert_same(run(dev, rows, H, W, NC, 0.5, rq, junk), er.first(res, 70), "garbage on rows that are not counted")
    bad = tab.copy()
    bad[counted[::7], 3], bad[counted[5:40], 64], bad[counted[0], 69] = 3, 255, 100   # values >= C in the simulations 3, 64 and 69 only
    want = against_the_reference(dev, rows, H, W, NC, 0.5, rq, bad, what="labels >= C")
    assert want[4][2 * NC + 2] & er.FLAG_LABEL and not res[4][2 * NC + 2] & er.FLAG_LABEL
    for s in range(70):
        assert (want[0][s].tobytes() == res[0][s].tobytes()) == (s not in (3, 64, 69)), s
    assert want[2][3].sum() == res[2][3].sum() - (res[3][counted[::7]] >= 0).sum()


# ---- 6. launch behaviour --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [257, 4097])
def test_the_cell_side_does_not_show_and_two_runs_give_the_same_bytes(dev, M):
    rows, rq, tab, res = er.clustered_sims(M)
    want = er.first(res, 65)
    r_max = int(rq[-1])
    for side in (0, 0, r_max, 2 * r_max, 7 * r_max + 3, 4 * W + 5):
        assert_same(run(dev, rows, H, W, NC, 0.5, rq, tab[:, :65], None, True, side), want, f"cell side {side}")


I32P = C.POINTER(C.c_int32)


class Buffers:
    def __init__(self, dev, M, C_, B, S):
        self.sim_pairs = torch.empty(S, C_, C_, B, device=dev, dtype=torch.int64)
        self.sim_centres = torch.empty(S, C_, B, device=dev, dtype=torch.int32)
        self.sim_inside = torch.empty(S, C_, device=dev, dtype=torch.int32)
        self.bd = torch.empty(M, device=dev, dtype=torch.int32)
        self.stats = torch.empty(2 * C_ + 3, device=dev, dtype=torch.int32)

    def all(self):
        return self.sim_pairs, self.sim_centres, self.sim_inside, self.bd, self.stats

    def numpy(self):
        return tuple(t.cpu().numpy() for t in self.all())


def call(L, rows, M, C_, H_, W_, rq, roi, border, side, mask, cell, labels, S, stride, o, ws, nbytes):
    rq = np.ascontiguousarray(rq, np.int32)
    roi_arg = None if roi is None else np.ascontiguousarray(roi, np.int32).ctypes.data_as(I32P)
    return L.ay_pair_counts_relabel(ptr(rows), M, C_, H_, W_, C.c_float(0.5), rq.ctypes.data_as(I32P), len(rq), roi_arg, border, side, ptr(mask), cell,
                                    ptr(labels), S, stride, ptr(o.sim_pairs), ptr(o.sim_centres), ptr(o.sim_inside), ptr(o.bd), ptr(o.stats),
                                    ptr(ws), nbytes, _lib.stream_ptr())


def test_bad_arguments_return_minus_one_with_a_message(dev):
    L = _lib.lib()
    rows = torch.zeros(4, 7, device=dev)
    labels = torch.zeros(4, 64, device=dev, dtype=torch.uint8)
    mask = torch.ones(7, 7, device=dev, dtype=torch.uint8)
    o = Buffers(dev, 4, 8, 32, 64)
    rq = [8, 16, 32]
    need, masked = (int(L.ay_pair_counts_relabel_workspace_bytes(4, 2, 3, 100, 100, 32, 0, cell, 64)) for cell in (0, 16))
    assert masked > need > 0
    ws = torch.zeros(masked + 256, device=dev, dtype=torch.uint8)

    def go(M=4, C_=2, H_=100, W_=100, r=rq, roi=None, side=0, m=None, cell=0, lab=labels, S=8, stride=64, nbytes=need, w=ws):
        return call(L, rows, M, C_, H_, W_, r, roi, 1, side, m, cell, lab, S, stride, o, w, nbytes)

    assert go() == 0 and go(m=mask, cell=16, nbytes=masked) == 0 and go(S=64) == 0 and go(S=8, stride=8) == 0
    for f, word in ((lambda: go(lab=None), b"labels"), (lambda: go(S=0), b"n_sims"), (lambda: go(S=1025, stride=1088), b"n_sims"),
                    (lambda: go(S=8, stride=7), b"label_stride"), (lambda: go(M=-1), b"n_rows"), (lambda: go(C_=0), b"num_classes"),
                    (lambda: go(C_=9), b"num_classes"), (lambda: go(H_=0), b"slide"), (lambda: go(r=[]), b"n_radii"),
                    (lambda: go(r=list(range(1, 34))), b"n_radii"), (lambda: go(r=[16, 8]), b"radii"), (lambda: go(r=[8, 32768]), b"radii"),
                    (lambda: go(roi=[50, 0, 49, 10]), b"roi"), (lambda: go(side=31), b"cell_side"), (lambda: go(m=mask, cell=8, nbytes=masked), b"mask_cell"),
                    (lambda: go(nbytes=need - 256), b"workspace"), (lambda: go(m=mask, cell=16), b"workspace"), (lambda: go(w=ws[4:]), b"aligned")):
        assert f() == -1
        assert b"ay_pair_counts_relabel" in L.ay_last_error() and word in L.ay_last_error(), (word, L.ay_last_error())
    torch.cuda.synchronize()


def test_hip_graph_of_the_call_replays_on_new_rows_and_a_new_table(dev):
    """ay_pair_counts_relabel captured on a side stream and replayed on other rows and another table: kernel launches only, and its own
    kernels reset the outputs"""
    M, S, stride = 1025, 70, 128
    L = _lib.lib()
    rq = sr.radii_q(sr.RADII_PX)
    inputs = [sr.clustered_rows(M, 70 + k) for k in range(3)]
    tables = [table_of(r, H, W, NC, 0.5, S - 1, 40 + k) for k, r in enumerate(inputs)]
    wants = [er.sim_counts(r, H, W, NC, 0.5, rq, t) for r, t in zip(inputs, tables)]
    for w in wants:
        assert w[0].min() > 0 and (w[0][1:] != w[0][0]).any()
    padded = [np.concatenate([t, np.full((M, stride - S), 255, np.uint8)], 1) for t in tables]
    rows, labels = torch.from_numpy(inputs[0]).to(dev), torch.from_numpy(padded[0]).to(dev)
    o = Buffers(dev, M, NC, len(rq), S)
    need = int(L.ay_pair_counts_relabel_workspace_bytes(M, NC, len(rq), H, W, int(rq[-1]), 0, 0, S))
    ws = torch.empty(need, device=dev, dtype=torch.uint8)

    def step():
        assert call(L, rows, M, NC, H, W, rq, None, 1, 0, None, 0, labels, S, stride, o, ws, need) == 0, L.ay_last_error()

    step()                                                            # eager once (loads the code objects)
    torch.cuda.synchronize()
    assert_same(o.numpy(), wants[0], "eager")
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        step()
    torch.cuda.synchronize()
    for k in (1, 2, 0, 1):
        for t in o.all():                                             # the graph's own kernels must reset the outputs
            t.fill_(77)
        rows.copy_(torch.from_numpy(inputs[k]))
        labels.copy_(torch.from_numpy(padded[k]))
        g.replay()
        torch.cuda.synchronize()
        assert_same(o.numpy(), wants[k], f"replay on input {k}")


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------
KEYS = ("K_sim", "L_minus_r_sim", "K_lo", "K_hi", "L_lo", "L_hi", "outside", "T", "p_mad")


def test_spatial_envelope_end_to_end(dev):
    rows, rq, _, _ = er.clustered_sims(257)
    rows = rows.copy()
    cls = sr.positions(rows, H, W, NC, 0.5)[2]
    tab = er.table(cls, NC, 39, 5)
    want = er.sim_counts(rows, H, W, NC, 0.5, rq, tab)
    loops = er.envelope_loops(want[0], want[1], want[2], rq, float(H * W), 2)
    for src in (rows, torch.from_numpy(rows).to(dev)):
        got = spatial_envelope(src, (H, W), sr.RADII_PX, NC, n_sim=39, seed=5, rank=2, min_conf=0.5)
        for name, w in zip(NAMES[:3], want):
            assert got[name].dtype == w.dtype and got[name].tobytes() == w.tobytes(), name
        for key in KEYS:
            np.testing.assert_array_equal(got[key], loops[key], err_msg=key)          # NaN positions included
        for key in ("K_mean", "L_mean"):
            np.testing.assert_allclose(got[key], loops[key], rtol=1e-13, atol=0, err_msg=key)
        np.testing.assert_array_equal(got["K_sim"][0], got["observed"]["K"])
        np.testing.assert_array_equal(got["L_minus_r_sim"][0], got["observed"]["L_minus_r"])
        plain = spatial_stats(src, (H, W), sr.RADII_PX, NC, 0.5)
        assert set(got["observed"]) == set(plain)
        for key, v in plain.items():
            np.testing.assert_array_equal(got["observed"][key], v, err_msg=key)
        assert (got["n_sim"], got["seed"], got["rank"], got["alpha_pointwise"], got["flags"]) == (39, 5, 2, 0.1, int(want[4][-1]))
        assert np.isfinite(got["p_mad"]).all() and got["K_sim"].shape == (40, NC, NC, len(rq))


def test_spatial_envelope_with_a_window(dev):
    rows, rq, mask, _ = swr.ragged_case(257)
    rows = rows.copy()
    Hs, Ws, Cs = swr.SLIDE_H, swr.SLIDE_W, swr.CLASSES
    tab = er.table(sr.positions(rows, Hs, Ws, Cs, 0.5)[2], Cs, 19, 0)
    roi = (50.0, 40.0, 1000.0, 740.0)
    want = er.sim_counts(rows, Hs, Ws, Cs, 0.5, rq, tab, sr.roi_q(roi, Hs, Ws), True, mask, swr.CELL)
    area = swr.window_area(mask, swr.CELL, Hs, Ws, sr.roi_q(roi, Hs, Ws))
    loops = er.envelope_loops(want[0], want[1], want[2], rq, area, 1)
    got = spatial_envelope(rows, (Hs, Ws), swr.RADII_PX, Cs, n_sim=19, seed=0, min_conf=0.5, roi=roi, window=mask.copy(), window_cell=swr.CELL)
    for name, w in zip(NAMES[:3], want):
        assert got[name].tobytes() == w.tobytes(), name
    for key in KEYS:
        np.testing.assert_array_equal(got[key], loops[key], err_msg=key)
    np.testing.assert_array_equal(got["K_sim"][0], got["observed"]["K"])
    assert got["observed"]["window_area"] == area and want[0].sum() > 0 and np.isfinite(got["p_mad"]).any()


def test_quantify_region_with_an_envelope(tmp_cfg_dir, dev):
    from test_gpu_burden import OVERLAP, S, TILE, small_model, synthetic_raster
    m = small_model(tmp_cfg_dir, dev)
    raster = synthetic_raster()
    RH, RW = raster.shape[:2]
    kw = dict(tile=TILE, img_size=S, conf_thres=0.5, nms_thres=0.4, batch_size=4, overlap=OVERLAP, cell=32, field=3, top_k=4)
    radii = (8, 24.5, 64)
    plain = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, **kw)
    got = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, spatial_envelope=19, spatial_seed=3, **kw)
    assert "spatial_envelope" not in plain and set(got) == set(plain) | {"spatial_envelope"}        # exactly one key more
    rows = got["rows"]
    assert torch.equal(rows, plain["rows"]) and len(rows) >= 12
    for key, v in plain["spatial"].items():
        np.testing.assert_array_equal(got["spatial"][key], v, err_msg=key)
    want = spatial_envelope(rows, (RH, RW), radii, 3, 19, 3, 1, 0.0, area=int(got["tissue"].sum()), mpp=0.5)
    env = got["spatial_envelope"]
    assert set(env) == set(want)
    for key, v in want.items():
        if key != "observed":
            np.testing.assert_array_equal(env[key], v, err_msg=key)
    for key, v in want["observed"].items():
        np.testing.assert_array_equal(env["observed"][key], v, err_msg=key)
    ref = er.sim_counts(rows.numpy(), RH, RW, 3, 0.0, sr.radii_q(radii), er.table(sr.positions(rows.numpy(), RH, RW, 3, 0.0)[2], 3, 19, 3))
    assert env["sim_pairs"].tobytes() == ref[0].tobytes() and env["sim_centres"].tobytes() == ref[1].tobytes() and ref[0].sum() > 0
    # the tissue-shaped window goes to the envelope too
    win = quantify_region(m, raster, mpp=0.5, spatial_radii=radii, spatial_window=True, spatial_envelope=19, spatial_seed=3, **kw)
    want = spatial_envelope(rows, (RH, RW), radii, 3, 19, 3, 1, 0.0, mpp=0.5, window=win["spatial_window"], window_cell=32)
    for key in ("sim_pairs", "sim_centres", "sim_inside", "p_mad", "K_lo", "K_hi"):
        np.testing.assert_array_equal(win["spatial_envelope"][key], want[key], err_msg=key)
    np.testing.assert_array_equal(win["spatial_envelope"]["observed"]["K"], win["spatial"]["K"])
