"""CPU: pin the oracle (oracle/*.py) against every fixture produced by the imported reference
(oracle/gen_golden.py).  Indices exact; floats within 1e-4 relative (|a-b| <= 1e-4*max(1,|b|))."""
import os

import numpy as np
import pytest
import torch

import golden_cases as gc
from amyloid_yolo_paper_amd import cfg_gen, parse_config, synth
from oracle import boxes_oracle as bo
from oracle.darknet_oracle import OracleDarknet

TOL = 1e-4


def close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    err = np.abs(a - b) / np.maximum(1.0, np.abs(b))
    assert err.max(initial=0.0) <= tol, float(err.max())


def load(golden_dir, name):
    return np.load(os.path.join(golden_dir, name + ".npz"))


def test_kats(golden_dir):
    z = load(golden_dir, "kat")
    np.testing.assert_array_equal(bo.bbox_iou([[100., 100, 200, 200]], [[150., 150, 200, 200], [201, 201, 300, 300], [100, 100, 200, 200]]), z["iou"])
    assert abs(z["iou"][0] - 0.254975) < 1e-6 and z["iou"][1] == 0 and z["iou"][2] == 1  # unit_test.py:141-150 convention
    np.testing.assert_array_equal(bo.bbox_iou([[5., 5, 4, 4]], [[6., 6, 4, 4]], x1y1x2y2=False), z["iou_c"])
    np.testing.assert_array_equal(bo.bbox_wh_iou([3., 4.], [[3., 4], [6, 2], [1, 1]]), z["whiou"])
    b1, b2 = gc.iou_inputs()
    np.testing.assert_array_equal(bo.bbox_iou(b1, b2), z["iou_rand"])
    np.testing.assert_array_equal(bo.bbox_iou(b1, b2, x1y1x2y2=False), z["iou_rand_c"])
    np.testing.assert_array_equal(bo.bbox_iou(b1[:1], b2), z["iou_bcast"])
    np.testing.assert_array_equal(bo.xywh2xyxy(b1), z["xyxy"])
    p = np.zeros((1, 21, 2, 2), np.float32)
    p[0, 0, 1, 0], p[0, 9, 0, 1], p[0, 18, 1, 1] = 1.0, 0.5, 2.0
    dec, _, _ = bo.decode(p, [(10, 13), (16, 30), (33, 23)], 2, 64)
    close(dec, z["decode"], 1e-6)
    rows, keep, clusters = bo.non_max_suppression(z["nms_in"][None].copy(), 0.5, 0.4)
    close(rows[0], z["nms_out"], 1e-6)
    assert keep[0].tolist() == [0, 2, 3] and [c.tolist() for c in clusters[0]] == [[0, 1, 5], [2], [3]]
    rb = bo.rescale_boxes(np.array([[10., 20, 200, 300, .9, .8, 1], [50, 60, 70, 80, .5, .5, 0]], np.float32), 416, (1536, 1024))
    close(rb, z["rescale"], 1e-6)


@pytest.mark.parametrize("name", [c[0] for c in gc.NMS_CASES])
def test_nms_cases(golden_dir, name):
    z = load(golden_dir, "nms_" + name)
    pred, conf_t, nms_t = gc.nms_case_inputs(name)
    rows, keep, _ = bo.non_max_suppression(pred, conf_t, nms_t)
    np.testing.assert_array_equal(pred[0, :8], z["corners0"])  # in-place corner conversion
    for b in range(pred.shape[0]):
        n = int(z[f"n{b}"])
        if n == 0:
            assert rows[b] is None
            continue
        np.testing.assert_array_equal(keep[b], z[f"keep{b}"])  # bit-exact indices
        close(rows[b], z[f"rows{b}"], 1e-5)
        np.testing.assert_array_equal(rows[b][:, 4:], z[f"rows{b}"][:, 4:])  # conf/cls columns untouched


def _oracle_model(C, cfg_dir):
    cfg = cfg_gen.write_cfg(C, cfg_dir)
    defs = parse_config.parse_model_config(cfg)
    m = OracleDarknet(cfg)
    m.set_params(synth.synth_params(defs, seed=7))
    return m, defs


@pytest.mark.parametrize("case", [c if c[2] <= 416 else pytest.param(c, marks=pytest.mark.slow) for c in gc.MODEL_CASES], ids=lambda c: c[0])
def test_model_forward(golden_dir, tmp_cfg_dir, case):
    """every whole-model fixture of the reference, the 1024^2 one included (marked slow: a few seconds of CPU convolutions), so that
    the fixture the GPU tests of BASELINE configs[1] lean on pins the oracle too"""
    name, C, S, B, start = case
    z = load(golden_dir, "model_" + name)
    m, _ = _oracle_model(C, tmp_cfg_dir)
    with torch.no_grad():
        out = m.forward(torch.from_numpy(gc.model_inputs(S, B, start)), collect=True).numpy()
    if "out" in z:
        close(out, z["out"])
    else:   # the 1024^2 fixture stores 256 sampled decode rows instead of all 64 512
        close(out[:, z["out_rows"]], z["out_sel"])
    for k, li in enumerate(z["layer_idx"]):
        f = m.layer_outputs[int(li)].numpy().reshape(-1)
        close(f[z["samp_idx"][k]], z["samp_val"][k])
        close(np.abs(f).max(), z["layer_amax"][k])
    if "out" in z:   # merge-NMS on the reference's own decode output reproduces the reference's rows
        rows_r, keep_r, _ = bo.non_max_suppression(z["out"].copy(), 0.5, 0.4)
        for b in range(B):
            assert (0 if rows_r[b] is None else len(rows_r[b])) == int(z[f"nms_n{b}"])
            if rows_r[b] is not None:
                np.testing.assert_array_equal(keep_r[b], z[f"nms_keep{b}"])
                close(rows_r[b], z[f"nms_rows{b}"], 1e-6)
    # ... and on the oracle's.  Its boxes are held to the decode output's bar in the decode output's own form (centre, size): a corner
    # near 0 is the difference of a centre and a half size of ~10^2 px, where the CPU convolutions' rounding (it differs between
    # instruction sets) passes the 1e-4 bar on the decode output and not on the corner.
    rows, keep, _ = bo.non_max_suppression(out.copy(), 0.5, 0.4)
    for b in range(B):
        assert (0 if rows[b] is None else len(rows[b])) == int(z[f"nms_n{b}"])
        if rows[b] is not None:
            np.testing.assert_array_equal(keep[b], z[f"nms_keep{b}"])
            close(_centre_size(rows[b]), _centre_size(z[f"nms_rows{b}"]))


def _centre_size(rows):
    """NMS rows [n, 7] (x1, y1, x2, y2, conf, cls_conf, cls) -> (cx, cy, w, h, conf, cls_conf, cls)"""
    r = np.asarray(rows, np.float64)
    return np.concatenate([(r[:, :2] + r[:, 2:4]) / 2, r[:, 2:4] - r[:, :2], r[:, 4:]], axis=1)


def test_weights_file_layout(golden_dir, tmp_cfg_dir, tmp_path):
    import hashlib
    z = load(golden_dir, "weights_c2")
    cfg = cfg_gen.write_cfg(2, tmp_cfg_dir)
    defs = parse_config.parse_model_config(cfg)
    path = str(tmp_path / "w.weights")
    synth.write_darknet_weights(path, defs, synth.synth_params(defs, seed=7), seen=12345)
    assert os.path.getsize(path) == int(z["nbytes"]) == 246326928
    assert hashlib.sha256(open(path, "rb").read()).digest() == z["sha256"].tobytes()
    m = OracleDarknet(cfg)
    m.load_darknet_weights(path)
    assert m.seen == 12345


@pytest.mark.parametrize("case", gc.TRAIN_CASES, ids=lambda c: c[0])
def test_train_step(golden_dir, tmp_cfg_dir, case):
    name, C, S, B, seed = case
    z = load(golden_dir, name)
    m, _ = _oracle_model(C, tmp_cfg_dir)
    m.require_grad()
    tg = gc.train_targets(B, C, S, seed)
    np.testing.assert_array_equal(tg, z["targets"])
    loss, out = m.forward(torch.from_numpy(gc.model_inputs(S, B, 10)), torch.from_numpy(tg), train_bn=True)
    loss.backward()
    close(loss.item(), z["loss"])
    keys = list(z["metric_keys"])
    got = np.array([[mm[k] for k in keys] for mm in m.metrics])
    close(got, z["metrics"], 2e-4)
    for li in (0, 2, 81, 93, 105):
        g = m.params[li]["weight"].grad.numpy()
        ref = z[f"gw{li}"]
        scale = np.abs(ref).max()
        assert np.abs(g - ref).max() <= 2e-3 * scale, (li, np.abs(g - ref).max(), scale)
    for li in (0, 80):
        close(m.params[li]["mean"].numpy(), z[f"rmean{li}"], 1e-4)
        close(m.params[li]["var"].numpy(), z[f"rvar{li}"], 1e-4)


@pytest.mark.parametrize("case", gc.TRAIN_CASES, ids=lambda c: c[0])
def test_build_targets(golden_dir, case):
    name, C, S, B, seed = case
    z = load(golden_dir, "bt_" + name)
    G = S // 8
    rng = np.random.Generator(np.random.PCG64(seed + 100))
    pb = rng.uniform(0, G, (B, 3, G, G, 4)).astype(np.float32)
    pc = rng.uniform(0, 1, (B, 3, G, G, C)).astype(np.float32)
    out = bo.build_targets(pb, pc, gc.train_targets(B, C, S, seed), z["anchors"], 0.5)
    names = ["iou_scores", "class_mask", "obj_mask", "noobj_mask", "tx", "ty", "tw", "th", "tcls", "tconf"]
    for n, v in zip(names, out):
        if v.dtype == bool:
            np.testing.assert_array_equal(v, z[n])
        else:
            close(v, z[n], 1e-6)


def test_merge_detections_vs_reference(golden_dir):
    """postprocess.merge_detections against the reference's own mergeDetections outputs (tests/golden/merge_cases.npz,
    generated by oracle/gen_golden_merge.py): same rows in the same order, exact."""
    from amyloid_yolo_paper_amd.postprocess import merge_detections
    z = load(golden_dir, "merge_cases")
    for name, det in gc.merge_inputs().items():
        got = merge_detections(torch.from_numpy(det))
        got = got.reshape(-1, 7).numpy().astype(np.float64) if got.numel() else np.zeros((0, 7))
        ref = z[name]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        np.testing.assert_array_equal(got, ref, err_msg=name)
    assert z["chain3"].shape[0] == 1 and z["touching_edge"].shape[0] == 2 and z["random40"].shape[0] < 40


def test_merge_ordered_oracle_vs_reference(golden_dir):
    """oracle.merge_detections_ordered (the reference's mergeDetections with the set's iteration order made explicit; what the
    device kernel ay_merge_detections implements) against the reference's own outputs, AS SETS of rows: equal wherever the
    result does not depend on which overlapping pair meets first (8 of the 9 fixture cases); on random40 one chain of merges
    comes out with another order under CPython's set, and through the one-pixel shrink per merge (core.py:357) one row's
    edges differ by a few pixels -- same number of rows, same confidences."""
    z = load(golden_dir, "merge_cases")
    for name, det in gc.merge_inputs().items():
        got = bo.merge_detections_ordered(det)
        ref = z[name].reshape(-1, 7)
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        a, b = set(map(tuple, got.tolist())), set(map(tuple, ref.tolist()))
        if name != "random40":
            assert a == b, (name, a ^ b)
        else:
            only_a, only_b = sorted(a - b), sorted(b - a)
            assert len(only_a) == len(only_b) <= 2
            for ra, rb in zip(only_a, only_b):
                assert ra[4:] == rb[4:] and max(abs(p - q) for p, q in zip(ra[:4], rb[:4])) <= 4, (ra, rb)


@pytest.mark.parametrize("thr", [0.5, 0.75])
def test_eval_statistics_oracle_vs_reference(golden_dir, thr):
    """oracle get_batch_statistics / ap_per_class against the reference's outputs (tests/golden/stats_cases.npz)"""
    z = load(golden_dir, "stats_cases")
    tag = f"t{int(thr * 100)}"
    outputs, targets = gc.stats_inputs()
    metrics = bo.get_batch_statistics(outputs, targets, thr)
    assert len(metrics) == int(z[f"{tag}_n"])
    for k, (tp, scores, labels) in enumerate(metrics):
        np.testing.assert_array_equal(tp, z[f"{tag}_tp{k}"])
        np.testing.assert_array_equal(scores, z[f"{tag}_scores{k}"])
    tp, scores, labels = [np.concatenate(x, 0) for x in zip(*metrics)]
    p, r, ap, f1, cls = bo.ap_per_class(tp, scores, labels, targets[:, 1])
    for got, name in ((p, "p"), (r, "r"), (ap, "ap"), (f1, "f1")):
        np.testing.assert_allclose(got, z[f"{tag}_{name}"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(cls, z[f"{tag}_cls"])


def test_giou_closed_form_vectors(golden_dir):
    """oracle GIoU (corner form and the differentiable cxcywh form the loss uses) against exact rationals of the published
    definition on integer boxes (tests/golden/giou_kat.json): the reference has no GIoU, these vectors are the pin."""
    import json
    from oracle.darknet_oracle import giou_cxcywh
    doc = json.load(open(os.path.join(golden_dir, "giou_kat.json")))
    b1 = np.array([c["box1"] for c in doc["cases"]], np.float32)
    b2 = np.array([c["box2"] for c in doc["cases"]], np.float32)
    want = np.array([c["giou"][0] / c["giou"][1] for c in doc["cases"]])
    np.testing.assert_allclose(bo.bbox_giou(b1, b2), want, rtol=0, atol=2e-7)
    np.testing.assert_allclose(bo.bbox_giou(b2, b1), want, rtol=0, atol=2e-7)          # symmetric

    def cxcywh(b):
        return torch.tensor(np.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2, b[:, 2] - b[:, 0], b[:, 3] - b[:, 1]], 1))
    np.testing.assert_allclose(giou_cxcywh(cxcywh(b1), cxcywh(b2)).numpy(), want, rtol=0, atol=2e-7)


def test_layer_modes_override_the_storage_type_per_layer(tmp_cfg_dir):
    """`OracleDarknet.forward(layer_modes=...)` (oracle/parity_sweep.py): an all-fp32 plan is the default forward bit for bit, an all-bf16
    / all-fp16 plan is `mode="bf16"` / `mode="fp16"` bit for bit, and a split plan differs from both"""
    m, _ = _oracle_model(3, tmp_cfg_dir)
    x = torch.from_numpy(gc.model_inputs(64, 1, 0))
    with torch.no_grad():
        base = m.forward(x)
        assert torch.equal(m.forward(x, layer_modes=lambda i: "fp32"), base)
        for mode in ("bf16", "fp16"):
            assert torch.equal(m.forward(x, layer_modes=lambda i, mode=mode: mode), m.forward(x, mode=mode))
        split = m.forward(x, layer_modes=lambda i: "bf16" if i <= 36 else "fp16")
        assert not torch.equal(split, m.forward(x, mode="bf16")) and not torch.equal(split, m.forward(x, mode="fp16"))
