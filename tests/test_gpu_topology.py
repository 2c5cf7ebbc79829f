"""GPU (-m gpu): the graph lowering and both training engines on the cfgs of tests/topology_cases.py -- graphs beyond the
107-block YOLOv3 topology, which is the only one every other model test builds -- against the CPU oracle (oracle/darknet_oracle.py).

Which test reaches the arms no YOLOv3 test reaches (op lists: topology_cases.LOWERED, pinned by tests/test_topology_cpu.py):
  * OP_CONCAT_UPSAMPLE with up1 = 0 (same-resolution two-source route, copied)    A layers 10, 17; B layer 8; cat_into_shortcut layer 3:
                                                                                   test_16bit_plan_equals_host_executor, test_16bit_vs_oracle
  * OP_CONCAT_UPSAMPLE with c2 = 0 (a lone lazy upsample, 16-bit)                  A layer 15 (single-source route), B layer 7 (3x3 reads it): the same
  * fp32 loader, lazy upsample without second source (up1 = 1)                    B layer 7: test_fp32_vs_oracle
  * fp32 loader, two-source route without upsample (up1 = 0, src2)                A layers 11, 18; B layer 9: test_fp32_vs_oracle
  * fp32 OP_CONCAT_UPSAMPLE (up1 1, c2 0), a lone upsample copied                 A layer 15: test_fp32_vs_oracle
  * OP_CONV1X1_CAT with a 64|128 split                                            C layer 7: test_fold_and_traversal_give_the_same_bits, test_16bit_plan_equals_host_executor
  * shortcut fused into a 1x1 layer                                               B layer 2, cat_into_shortcut layer 4: test_16bit_vs_oracle, test_fp32_vs_oracle
  * OP_STEM followed by a plain layer 1                                           B, cat_into_shortcut (default options); A, C (option set "unfused")
  * fuse_block_channels = (64, 128) through the model                             A, option set "block128": test_16bit_plan_equals_host_executor, test_16bit_vs_oracle
  * heads with 2, 4 and 6 anchors, unequal heads, row_offset                      B (2, 6), A (3, 4): every inference test; head + decode fusion in the plan tests
  * BatchNorm layer with linear activation                                        B layer 14
  * 96, 160, 192 channels                                                         A layer 11 (192 -> 96), layer 18 (160 -> 128)
  * 3x3 convolution after a route                                                 A layers 11, 16; B layer 13
  * training: all of the above through train_engine.py (A, B): test_fp32_train_step_vs_oracle
  * a two-source route that a shortcut reads (cat_into_shortcut): 16-bit copies it; fp32 used to fail an assert and now copies it too

Not here: the bf16 training engine (train_engine_bf16.py) on these graphs.  One teacher-forced step on A (with the engine's
single-source route of an upsample made to materialise it) did not return on an MI355X; the cause was not found, so the engine is as
it was and no bf16 training test of these graphs is in the suite.

Outcome per graph and precision: A, B, C correct in fp32, bf16x6, bf16x3, bf16, fp16 and in the fp32 training engine; cat_into_shortcut
correct in all five inference precisions (fp32 and the split modes: now supported); stem16 and bn48 correct in fp32, bf16x6, bf16x3 and
refused by layer index in bf16 / fp16; shortcut_shared, route3 and anchors7 refused by layer index in every precision; maxpool refused by
create_modules.

Measured, worst over the two shapes (64, 2) and (96, 3); the oracle's own spread (fp32 against float64 convolution sums, (64, 2),
tests/test_topology_cpu.py) in brackets; device figures from an MI355X:
  fp32 / bf16x6, rows and every kept layer, bar 1e-4 (close):
      A 5.2e-6 / 2.2e-6 [1.6e-6]   B 3.4e-6 / 2.2e-6 [1.4e-6]   C 3.2e-6 / 1.6e-6 [1.5e-6]
      stem16 2.2e-6 / 1.2e-6 [1.2e-6]   bn48 1.8e-6 / 1.3e-6 [1.1e-6]   cat_into_shortcut 1.0e-6 / 1.0e-6 [1.0e-6]
  bf16x3, deviation from the fp32 path over fp16's, bar 1/8:
      A 0.014   B 0.021   C 0.019   stem16 0.016   bn48 0.014   cat_into_shortcut 0.018      (deviation 1.9e-5 .. 3.4e-5)
  bf16 | fp16, share of a layer's stored activations outside the bound (bar 2e-3 [5e-4]), largest head-logit error (bar 0.5 k [0.05 k]),
  largest confidence error (bar 0.12 k), boxes q99.9 (bar 0.05 k), k = 1 | 1/8:
      A                  0 [0], 1.04e-2 [9.1e-3], 2.3e-3, 6.0e-3  |  0 [0], 1.75e-3 [1.3e-3], 3.7e-4, 9.9e-4
      A block128         0, 9.9e-3, 2.2e-3, 5.9e-3                |  0, 1.75e-3, 3.9e-4, 9.9e-4
      A unfused          0, 1.13e-2, 2.5e-3, 6.4e-3               |  0, 1.66e-3, 4.0e-4, 1.0e-3
      B                  0 [0], 1.14e-2 [8.6e-3], 2.1e-3, 3.1e-3  |  0 [0], 1.46e-3 [1.3e-3], 3.0e-4, 5.8e-4
      C                  0 [0], 8.2e-3 [5.5e-3], 1.8e-3, 3.0e-3   |  0 [0], 1.11e-3 [1.0e-3], 2.3e-4, 5.8e-4
      C unfused          0, 7.1e-3, 1.5e-3, 3.7e-3                |  0, 1.10e-3, 2.4e-4, 6.2e-4
      cat_into_shortcut  0 [0], 6.5e-3 [1.0e-3], 1.3e-3, 1.6e-5   |  0 [0], 1.23e-3 [1.2e-3], 1.9e-4, 1.0e-4
  plan against host executor, folded against copied route, alternate traversal on / off: identical bits.
  fp32 training step at (64, 2), every convolution layer: contract_spread (test_gpu_train) A 1.0e-6 at the heads, 3.3e-6 below layer 18,
  5.5e-6 at layer 0; B 9.8e-7 at the heads, 1.8e-6 down to layer 9, 9.2e-5 at 7, 1.1e-4 at 5 and 4, 2.9e-4 from 2 down.  Device: filter
  gradients in trimmed relative L2 A <= 5.7e-6 (bar 2e-4), B 2.9e-4 at layers 0 to 2 (bar 7.3e-4) and <= 2.4e-6 above; head gradients
  <= 6.0e-6 of their scale (bar 2e-4).
"""
import numpy as np
import pytest
import torch

import golden_cases as gc
import topology_cases as tc
from amyloid_yolo_paper_amd.models import SPLIT_PRECISIONS, Darknet
from oracle.darknet_oracle import OracleDarknet
from test_gpu_parity import TOL, check_model_vs_16bit_oracle, close
from test_gpu_split import deviation

pytestmark = pytest.mark.gpu
SHAPES = [(64, 2, 0), (96, 3, 2)]          # S, B, first tile of golden_cases.model_inputs
ids = lambda v: "x".join(str(x) for x in v) if isinstance(v, tuple) else str(v)
_models = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def model(name, cfg_dir, dev, precision=None, option_set=None):
    """eval-mode Darknet of graph `name` with the synthetic weights loaded through the Darknet .weights format; one per argument set"""
    key = (name, precision, option_set)
    if key not in _models:
        cfg, _, _, wpath = tc.synth_weights(name, cfg_dir)
        m = Darknet(cfg, precision=precision or "bf16")
        if option_set is not None:
            tc.apply_options(m, option_set, precision)
        m = m.to(dev).eval()
        m.load_darknet_weights(wpath)
        _models[key] = m
    return _models[key]


def oracle(name, cfg_dir):
    cfg, _, params, _ = tc.synth_weights(name, cfg_dir)
    o = OracleDarknet(cfg)
    o.set_params(params)
    return o


def inputs(shape):
    S, B, start = shape
    return torch.from_numpy(gc.model_inputs(S, B, start))


# ---------------------------------------------------------------------------------------------------------------- fp32 and the split modes
FP32_GRAPHS = tc.MAIN + tc.FP32_ONLY + ("cat_into_shortcut",)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("precision", ["fp32", "bf16x6"])
@pytest.mark.parametrize("name", FP32_GRAPHS)
def test_fp32_vs_oracle(tmp_cfg_dir, dev, name, precision, shape):
    """precision='fp32' and 'bf16x6' (which test_gpu_split holds to the fp32 bar): decoded rows and EVERY kept layer output within
    TOL = 1e-4 of the oracle (test_gpu_parity.close), whose own spread on these graphs is 1.6e-6 (test_topology_cpu)"""
    S, B, start = shape
    m = model(name, tmp_cfg_dir, dev, precision)
    rows, layers = tc.oracle_forward(name, tmp_cfg_dir, S, B, start)
    m.keep_layer_outputs = True
    try:
        out = m(inputs(shape))
        assert not out.is_cuda and out.shape == (B, m.num_boxes(S), 5 + tc.CLASSES)
        worst = deviation(out.numpy(), rows.numpy())
        kept = sorted(m.layer_outputs)
        for li in kept:
            if m._graph[li]["type"] == "yolo":
                continue
            got = m.layer_output_nchw(li).cpu().numpy()
            worst = max(worst, deviation(got, layers[li].numpy()))
            close(got, layers[li].numpy(), TOL, f"layer {li}")
        print(f"topology {name} {precision} S={S} B={B}: worst deviation {worst:.2e} over the rows and {len(kept)} layers")
        close(out.numpy(), rows.numpy(), TOL, "rows")
        # every layer the lowering materialises is kept: all but convolutions fused into a shortcut, lazy upsamples, folded routes
        assert len(kept) >= sum(e["type"] == "convolutional" and not e["fuse_into_shortcut"] for e in m._graph)
    finally:
        m.keep_layer_outputs = False


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("name", FP32_GRAPHS)
def test_bf16x3_between_fp32_and_fp16(tmp_cfg_dir, dev, name, shape):
    """the bar of test_gpu_split.test_model_bf16x3_between_fp32_and_fp16: bf16x3 deviates from the fp32 path by at most 1/8 of what
    fp16 does.  Over ALL rows here: with the synthetic weights no row of these small graphs reaches a confidence of 0.5 (the largest
    is 0.19), and the ratio of the rounding steps does not depend on the selection.  The fp16 evaluation is the device's fp16 path
    where it runs the graph and the oracle's mode='fp16' where the 16-bit lowering refuses it (stem16, bn48)."""
    S, B, start = shape
    x = inputs(shape)
    ref = model(name, tmp_cfg_dir, dev, "fp32")(x).numpy()
    d3 = deviation(model(name, tmp_cfg_dir, dev, "bf16x3")(x).numpy(), ref)
    if name in tc.FP32_ONLY:
        d16 = deviation(tc.oracle_forward(name, tmp_cfg_dir, S, B, start, mode="fp16")[0].numpy(), tc.oracle_forward(name, tmp_cfg_dir, S, B, start)[0].numpy())
    else:
        d16 = deviation(model(name, tmp_cfg_dir, dev, "fp16")(x).numpy(), ref)
    print(f"topology {name} bf16x3 S={S} B={B}: deviation {d3:.3e}, fp16 {d16:.3e}, ratio {d3 / max(d16, 1e-300):.4f}")
    assert d3 <= d16 / 8.0, (d3, d16)


def test_split_precisions_are_the_ones_tested():
    assert set(SPLIT_PRECISIONS) == {"bf16x6", "bf16x3"}


# ---------------------------------------------------------------------------------------------------------------- bf16 / fp16 inference
PLAN_GRAPHS = tc.MAIN + ("cat_into_shortcut",)


@pytest.mark.parametrize("option_set", tc.PLAN_OPTION_SETS)
@pytest.mark.parametrize("name", PLAN_GRAPHS)
def test_16bit_plan_equals_host_executor(tmp_cfg_dir, dev, name, option_set):
    """(a) ay_plan_forward gives the rows of the host executor of the same op list, bit for bit (the method of
    test_gpu_parity.test_native_plan_equals_per_layer_walk), for every option set; shapes alternate so that the arena is reused
    across differently shaped plans, two forwards each.  The plan fuses every head with its decode (2, 3, 4 and 6 anchors), the host
    executor does not."""
    m = model(name, tmp_cfg_dir, dev, option_set=option_set)
    assert m.use_plan
    try:
        for shape in (SHAPES[0], SHAPES[1], (64, 2, 5)):
            x = inputs(shape)
            m.use_plan = False
            ref = m(x).clone()
            m.use_plan = True
            for rep in range(2):
                assert torch.equal(m(x), ref), (shape, rep)
            assert bool(torch.isfinite(ref).all())
    finally:
        m.use_plan = True


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("name", tc.MAIN)
def test_fold_and_traversal_give_the_same_bits(tmp_cfg_dir, dev, name, precision):
    """(b) the route folded into the 1x1 loader (OP_CONV1X1_CAT, C: 64|128) and the materialised concatenation give the same rows bit
    for bit (as test_conv1x1_cat_kernel shows for the kernel alone); so do alternate_traversal on and off, on every graph"""
    m = model(name, tmp_cfg_dir, dev, precision)
    saved = (m.fold_routes, m.alternate_traversal)
    try:
        for shape in SHAPES:
            x = inputs(shape)
            ref = m(x).clone()
            m.alternate_traversal = not saved[1]
            assert torch.equal(m(x), ref), ("alternate_traversal", shape)
            m.alternate_traversal = saved[1]
            m.fold_routes = False
            assert torch.equal(m(x), ref), ("fold_routes", shape)
            m.fold_routes = True
    finally:
        m.fold_routes, m.alternate_traversal = saved


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name,option_set", [(n, None) for n in PLAN_GRAPHS] + [("A", "block128"), ("A", "unfused"), ("C", "unfused")], ids=str)
def test_16bit_vs_oracle(tmp_cfg_dir, dev, name, option_set, dtype, shape):
    """(c) rows and every kept layer against OracleDarknet(mode=dtype) with the per-layer and decoded-box bounds of
    test_gpu_parity.test_model_bf16_vs_bf16_oracle; with fuse_block_channels = (64, 128) on A (the C=128 fused block through the
    model) and with the unfused option set the same bounds hold"""
    m = model(name, tmp_cfg_dir, dev, dtype, option_set)
    fig = check_model_vs_16bit_oracle(m, oracle(name, tmp_cfg_dir), inputs(shape), dtype)
    print(f"topology {name} {option_set or 'default'} {dtype} S={shape[0]} B={shape[1]}: share outside the bound {fig['share']:.2e}, "
          f"head logits {fig['head']:.2e}, confidence {fig['dconf']:.2e}, boxes q99.9 {fig['box']:.2e}")


# ---------------------------------------------------------------------------------------------------------------- refusals on the device
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_bn48_is_refused_before_any_launch(tmp_cfg_dir, dev, precision):
    """a BN layer with 48 filters: the 16-bit path refuses it by layer index in _prepare, before a weight is folded or packed"""
    cfg, _, _, wpath = tc.synth_weights("bn48", tmp_cfg_dir)
    m = Darknet(cfg, precision=precision).to(dev).eval()
    m.load_darknet_weights(wpath)
    with pytest.raises(NotImplementedError, match=r"layer 1\b"):
        m(inputs(SHAPES[0]))
    assert m._prep is None and not m._act_bufs


# ---------------------------------------------------------------------------------------------------------------- training, fp32
TRAIN_S, TRAIN_B, TRAIN_SEED = 64, 2, 21


def oracle_train_step(name, cfg_dir, x, tg):
    """the reference's training step on graph `name` in the form of tests/golden/train_*.npz (test_gpu_train.check_train_step)"""
    from amyloid_yolo_paper_amd.train_engine import METRIC_KEYS
    o = oracle(name, cfg_dir)
    o.require_grad()
    loss, out = o.forward(x, tg, train_bn=True)
    loss.backward()
    z = {"out": out.numpy(), "loss": float(loss.item()), "metric_keys": METRIC_KEYS,
         "metrics": np.array([[mt[k] for k in METRIC_KEYS] for mt in o.metrics])}
    for li, p in o.params.items():
        z[f"gw{li}"] = p["weight"].grad.numpy()
        if "bias" in p:
            z[f"gb{li}"] = p["bias"].grad.numpy()
        else:
            z[f"ggamma{li}"], z[f"gbeta{li}"] = p["gamma"].grad.numpy(), p["beta"].grad.numpy()
            z[f"rmean{li}"], z[f"rvar{li}"] = p["mean"].numpy(), p["var"].numpy()
    return z, o


@pytest.mark.parametrize("name", ["A", "B"])
def test_fp32_train_step_vs_oracle(tmp_cfg_dir, dev, name):
    """One fp32 training step (train_engine.py) on A and B against the oracle's step: method and bars of
    test_gpu_train.test_train_step_vs_reference with the oracle in the place of the golden file -- loss 1e-4, head-layer gradients
    2e-4 of their scale, every other filter gradient within max(2.5 x spread, 2e-4) in trimmed relative L2 (spread: contract_spread of
    this cfg), BN running statistics 1e-4, num_batches_tracked == 1 -- on EVERY convolution layer."""
    from test_gpu_train import check_train_step, contract_spread
    cfg, _, _, wpath = tc.synth_weights(name, tmp_cfg_dir)
    x = torch.from_numpy(gc.model_inputs(TRAIN_S, TRAIN_B, 10))
    tg = torch.from_numpy(gc.train_targets(TRAIN_B, tc.CLASSES, TRAIN_S, TRAIN_SEED))
    z, o = oracle_train_step(name, tmp_cfg_dir, x, tg)
    layers = tuple(o.params)
    heads = tuple(li for li, p in o.params.items() if "bias" in p)
    spread = contract_spread(cfg, layers, [(x, tg)])
    print(f"topology {name} contract spread:", {li: float(f"{v:.2e}") for li, v in spread.items()})
    m = Darknet(cfg, precision="fp32").to(dev)
    m.load_darknet_weights(wpath)
    m.train()
    check_train_step(m, z, x, tg, layers, heads, spread)
