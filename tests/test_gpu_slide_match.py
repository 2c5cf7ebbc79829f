"""Slide-level evaluation (-m gpu): ay_slide_match through stats.match_slide, stats.slide_statistics and wsi.evaluate_region.
Every comparison is exact: the rule only compares fp32 values that both sides compute with the same operations, and best_iou is
compared bit for bit.

Yardsticks: the reference's own true-positive flags (tests/golden/stats_cases.npz); tests/slide_match_reference.py (the rule in
NumPy float32, a sort and a sequential walk against all targets); the per-tile kernel ay_match_detections where it reaches."""
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
import slide_match_reference as smr
from amyloid_yolo_paper_amd import _lib, cfg_gen, parse_config, synth
from amyloid_yolo_paper_amd.models import Darknet
from amyloid_yolo_paper_amd.stats import get_batch_statistics, match_slide, slide_statistics
from amyloid_yolo_paper_amd.wsi import detect_region, evaluate_region

pytestmark = pytest.mark.gpu

EXACT = ("tp", "claim", "best_target", "row_ignored", "target_ignored", "eligible", "claimed")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def device_match(rows, targets, thres, roi=None, cell_side=None):
    m = match_slide(rows, targets, thres, roi, cell_side=cell_side)
    return {k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in m.items()}


def assert_same(got, want):
    for key in EXACT:
        np.testing.assert_array_equal(got[key], want[key], err_msg=key)
    np.testing.assert_array_equal(got["best_iou"].view(np.uint32), want["best_iou"].view(np.uint32), err_msg="best_iou bits")


def as_bytes(got):
    return b"".join(np.ascontiguousarray(got[k]).tobytes() for k in EXACT + ("best_iou",))


# ---- 1. the reference's own flags ------------------------------------------------------------------------------------------------
def test_golden_images_as_slides(dev, golden_dir):
    z = np.load(os.path.join(golden_dir, "stats_cases.npz"))
    outputs, targets = gc.stats_inputs()
    present = [b for b, o in enumerate(outputs) if o is not None]
    assert len(present) == 11
    for k, b in enumerate(present):
        rows, tg = smr.golden_image(outputs, targets, b)
        got = device_match(rows, tg, [0.5, 0.75])
        np.testing.assert_array_equal(got["tp"][0], z[f"t50_tp{k}"].astype(np.uint8))
        np.testing.assert_array_equal(got["tp"][1], z[f"t75_tp{k}"].astype(np.uint8))
        assert_same(got, smr.match_slide(rows, tg, [0.5, 0.75]))


# ---- 2. random slides ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", smr.SIZES_T)        # 2049 and 6000: past the 2048 targets of ay_match_detections
@pytest.mark.parametrize("M", smr.SIZES_M)
def test_random_slide(dev, M, T):
    """Every size asserts on the RESTATEMENT, before the kernel is looked at, that the case is not idle (check_not_idle: a true
    positive, an eligible row that lost its claim, a row whose label no target has).  The five cases with M == 1 assert the true
    positive only: one row cannot be all three.  tests/test_slide_match_cpu.py shows the same for five of the 30 sizes without a
    GPU; the other 25 are asserted here alone."""
    for fractional in (False, True):
        rows, targets = smr.random_slide(M, T, smr.case_seed(M, T), fractional)
        want = smr.match_slide(rows, targets, smr.THRES)
        print(M, T, fractional, "tp, lost claims, label-absent rows:", smr.check_not_idle(rows, targets, want))
        assert_same(device_match(rows, targets, smr.THRES), want)


def test_random_slide_with_roi_and_in_another_order(dev):
    rows, targets = smr.random_slide(1000, 2049, smr.case_seed(1000, 2049), True)
    side = float(targets[:, 3].max())
    roi = (0.25 * side, 0.2 * side, 0.8 * side, 0.75 * side)
    want = smr.match_slide(rows, targets, smr.THRES, roi)
    assert 0.2 < want["row_ignored"].mean() < 0.9 and 0.2 < want["target_ignored"].mean() < 0.9
    smr.check_not_idle(rows, targets, want)
    assert_same(device_match(rows, targets, smr.THRES, roi), want)
    perm = np.random.default_rng(3).permutation(len(rows))       # the rank is by score and index, not by position
    assert_same(device_match(rows[perm], targets, smr.THRES, roi), smr.match_slide(rows[perm], targets, smr.THRES, roi))
    tperm = np.random.default_rng(4).permutation(len(targets))   # the first maximum follows the target index
    assert_same(device_match(rows, targets[tperm], smr.THRES, roi), smr.match_slide(rows, targets[tperm], smr.THRES, roi))


def test_inputs_on_the_device_and_a_scalar_threshold(dev):
    rows, targets = smr.random_slide(65, 300, smr.case_seed(65, 300), True)
    got = match_slide(torch.from_numpy(rows).to(dev), torch.from_numpy(targets).to(dev), 0.5)
    assert got["tp"].is_cuda and got["tp"].shape == (1, 65) and got["claim"].shape == (1, 300)
    assert_same({k: (v.cpu().numpy() if torch.is_tensor(v) else v) for k, v in got.items()}, smr.match_slide(rows, targets, 0.5))


# ---- 3. geometry that stresses the grid ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", smr.GEOMETRY_CASES)
def test_geometry(dev, name):
    rows, targets, big = smr.geometry_case(name)
    want = smr.match_slide(rows, targets, smr.THRES)
    smr.check_not_idle(rows, targets, want, big)
    got = device_match(rows, targets, smr.THRES)
    print(name, "targets", len(targets), "oversize", got["oversize"])
    assert_same(got, want)
    if name == "oversize":
        assert 3 <= got["oversize"] < 30
        assert want["best_target"][-1] in big            # the detection that covers the whole slide
    if name == "far_target":
        assert got["oversize"] < 30 and want["claim"][1][-1] == len(rows) - 1   # bounded grid, and the far target is still found


# ---- 4. the result does not depend on the cell side ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["oversize", "borders", "far_target"])
def test_cell_side_independence(dev, name):
    rows, targets, _ = smr.geometry_case(name)
    base = device_match(rows, targets, smr.THRES)
    oversize = {None: base["oversize"]}
    for side in (4.0, 64.0, 3000.0):                       # every target oversize ... every target in a handful of cells
        got = device_match(rows, targets, smr.THRES, cell_side=side)
        oversize[side] = got["oversize"]
        assert as_bytes(got) == as_bytes(base), side
    print(name, "oversize targets per cell side", oversize)
    if name != "far_target":                               # (there the bounded grid doubles every side far beyond the boxes)
        assert oversize[3000.0] == 0 and oversize[4.0] > max(10, oversize[64.0])   # the sides really bin differently


# ---- 5. empty inputs -----------------------------------------------------------------------------------------------------------
def test_empty_inputs(dev):
    rows, targets = smr.random_slide(65, 64, smr.case_seed(65, 64), True)
    none_r, none_t = np.zeros((0, 7), np.float32), np.zeros((0, 5), np.float32)
    for r, t, roi in ((none_r, targets, None), (rows, none_t, None), (none_r, none_t, None), (rows, targets, (-50.0, -50.0, -40.0, -40.0))):
        got, want = device_match(r, t, smr.THRES, roi), smr.match_slide(r, t, smr.THRES, roi)
        assert_same(got, want)
        assert got["tp"].shape == (3, len(r)) and got["claim"].shape == (3, len(t))
        assert got["tp"].sum() == 0 and (got["claim"] == -1).all() and (got["best_target"] == -1).all() and (got["best_iou"] == 0).all()
    assert got["row_ignored"].all() and got["target_ignored"].all()


def test_bad_arguments(dev):
    rows, targets = smr.random_slide(65, 64, smr.case_seed(65, 64), True)
    with pytest.raises(_lib.AyError):
        match_slide(rows, targets, 0.0)
    with pytest.raises(_lib.AyError):
        match_slide(rows, targets, [0.5] * 17)
    targets[5, 0] = 0.5                                    # a class that is no integer
    with pytest.raises(_lib.AyError):
        match_slide(rows, targets, 0.5)


# ---- 6. determinism --------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes(dev):
    rows, targets = smr.random_slide(5000, 6000, smr.case_seed(5000, 6000), True)
    assert as_bytes(device_match(rows, targets, smr.THRES)) == as_bytes(device_match(rows, targets, smr.THRES))


# ---- 7. the per-tile kernel, where it reaches ------------------------------------------------------------------------------------
def test_agrees_with_the_per_tile_kernel(dev):
    rows, targets = smr.random_slide(1000, 2048, 77, True)
    rows[:, 4] = np.linspace(1.0, 0.5, len(rows), dtype=np.float32)       # strictly decreasing scores: rank order = row order
    rows[:, 5] = 1.0
    assert (np.diff(rows[:, 4]) < 0).all()
    t6 = np.concatenate([np.zeros((len(targets), 1), np.float32), targets], 1)
    (tp_tile, _, _), = get_batch_statistics([torch.from_numpy(rows)], t6, 0.5)
    got = device_match(rows, targets, 0.5)
    assert tp_tile.sum() >= 100 and smr.lost_claims(got) >= 100
    np.testing.assert_array_equal(got["tp"][0], tp_tile.astype(np.uint8))


# ---- 8. end to end -----------------------------------------------------------------------------------------------------------------
def annotations_from(rows, seed=5):
    """annotations derived from a detection run: its boxes, a third shifted by a few pixels, a sixth removed, and a few extra"""
    rng = np.random.default_rng(seed)
    r = rows.numpy()
    keep = rng.uniform(size=len(r)) > 1 / 6
    tb = r[keep, :4].astype(np.float64)
    shift = rng.uniform(size=len(tb)) < 1 / 3
    tb[shift] += rng.integers(-6, 7, (int(shift.sum()), 4))
    extra = rng.uniform(0, 300, (5, 2))
    tb = np.concatenate([tb, np.concatenate([extra, extra + rng.uniform(10, 40, (5, 2))], 1)])
    cls = np.concatenate([r[keep, 6], rng.integers(0, 3, 5)])
    return np.concatenate([cls[:, None], tb], 1).astype(np.float32)


S, TILE, OVERLAP = 128, 192, 64


def small_model(cfg_dir, dev):
    """the 3-class cfg_gen network with synthetic weights, bf16"""
    cfg = cfg_gen.write_cfg(3, cfg_dir)
    defs = parse_config.parse_model_config(cfg)
    wpath = os.path.join(cfg_dir, "slide_match_c3.weights")
    synth.write_darknet_weights(wpath, defs, synth.synth_params(defs, seed=7), seen=12345)
    m = Darknet(cfg, precision="bf16").to(dev).eval()
    m.load_darknet_weights(wpath)
    return m


def synthetic_raster():
    """six synthetic tiles side by side in two rows, doubled to 256-px content, with ragged right and bottom edges"""
    tiles = (gc.model_inputs(S, 6, 40) * 255).astype(np.uint8).transpose(0, 2, 3, 1)
    big = np.concatenate([np.concatenate(list(tiles[:3]), 1), np.concatenate(list(tiles[3:]), 1)], 0)
    return np.repeat(np.repeat(big, 2, 0), 2, 1)[: 2 * S + 77, : 3 * 2 * S - 50]


def test_evaluate_region_end_to_end(tmp_cfg_dir, dev):
    m = small_model(tmp_cfg_dir, dev)
    raster = synthetic_raster()
    kw = dict(tile=TILE, img_size=S, conf_thres=0.5, nms_thres=0.4, batch_size=4)
    base = torch.cat([d for _, _, d in detect_region(m, raster, **kw)])
    targets = annotations_from(base)
    assert len(base) >= 12
    for overlap in (0, OVERLAP):
        rows = torch.cat([d for _, _, d in detect_region(m, raster, overlap=overlap, **kw)])
        want = slide_statistics(rows, targets, [0.5, 0.75], match=smr.match_slide)
        got = evaluate_region(m, raster, targets, [0.5, 0.75], overlap=overlap, **kw)
        assert torch.equal(got["rows"], rows)
        print("overlap", overlap, "rows", len(rows), "counts", got["counts"], "AP", got["metrics"][0][2])
        assert got["counts"][0]["tp"] >= 3 and got["counts"][0]["missed"] >= 1 and got["counts"][0]["false_alarms"] >= 1
        for k in range(2):
            assert got["counts"][k] == want["counts"][k]
            np.testing.assert_array_equal(got["missed"][k], want["missed"][k])
            np.testing.assert_array_equal(got["false_alarms"][k], want["false_alarms"][k])
            for a, b in zip(got["metrics"][k], want["metrics"][k]):
                np.testing.assert_array_equal(a, b)
    # a region of interest: the same through the whole stack
    roi = (0.0, 0.0, 400.0, 300.0)
    got = evaluate_region(m, raster, targets, 0.5, roi=roi, overlap=OVERLAP, **kw)
    want = slide_statistics(got["rows"], targets, 0.5, roi=roi, match=smr.match_slide)
    assert got["counts"] == want["counts"] and 0 < got["counts"][0]["rows"] < len(got["rows"])
    np.testing.assert_array_equal(got["missed"][0], want["missed"][0])
    np.testing.assert_array_equal(got["false_alarms"][0], want["false_alarms"][0])
