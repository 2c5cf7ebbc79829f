"""The graph lowering on cfgs beyond Darknet-53, without a GPU: the op lists Darknet._lower gives for the graphs of
tests/topology_cases.py under every option set, ay_plan_create's arena on the 16-bit ones, the refusals (NotImplementedError that names
the layer, before anything is launched), and the reference's own spread on these graphs -- the bars of tests/test_gpu_topology.py rest on
it.  No kernel is launched: weights are host tensors standing in for device pointers (test_plan_cpu.fake_prep)."""
import numpy as np
import pytest
import torch

import topology_cases as tc
from amyloid_yolo_paper_amd import _lib
from amyloid_yolo_paper_amd.models import Darknet
from test_plan_cpu import check_plan_arena, fake_prep, reads_of

KIND = {getattr(_lib, "OP_" + n): n for n in ("STEM_S2_FUSED", "STEM", "CONV", "RESBLOCK", "CONV1X1_CAT", "CONCAT_UPSAMPLE", "DECODE")}
S, B = tc.LOWER_S, tc.LOWER_B
START = 10           # golden_cases.model_inputs(64, 2, 10): the input of the spread test


def op_tuples(low):
    """the op list in the form of topology_cases.LOWERED"""
    out = []
    for o, layer in zip(low.ops, low.op_layer):
        kind = KIND[o.kind]
        out.append((kind, layer, o.up1, o.c1, o.c2, o.res != _lib.PLAN_NONE, o.src2 != _lib.PLAN_NONE, o.row_offset if kind == "DECODE" else None))
    return out


def lower(name, option_set, cfg_dir):
    m = tc.apply_options(Darknet(tc.write(name, cfg_dir)), option_set)
    m._check_16bit_layers()
    return m, m._lower(B, S, fake_prep(m))


LOWER_CASES = [(name, option_set) for name, sets in tc.LOWERED.items() for option_set in sets]


@pytest.mark.parametrize("name,option_set", LOWER_CASES, ids=lambda v: str(v))
def test_lowering_gives_the_listed_ops(tmp_cfg_dir, name, option_set):
    """kind, layer, up1, c1, c2, which ops carry a residual or a second source, the row offset of every decode; dataflow of the list;
    on the 16-bit lists ay_plan_create with the lifetime checks of test_plan_cpu.test_lowering_and_arena"""
    m, low = lower(name, option_set, tmp_cfg_dir)
    got, want = op_tuples(low), tc.LOWERED[name][option_set]
    assert got == want, "\n".join(f"{'  ' if g == w else '!='} {g}   {w}" for g, w in zip(got + [None] * len(want), want + [None] * len(got)))
    g = m._graph
    born = set()
    for i, o in enumerate(low.ops):
        for v in reads_of(o):
            assert v == _lib.PLAN_INPUT or v in born, (i, v)
        if o.kind != _lib.OP_DECODE:
            assert o.dst not in born, (i, o.dst)
            born.add(o.dst)
    assert born == set(range(len(low.values)))
    # every op reads values of the right shape: the channel split of a copy / a loader adds up to what its reader takes
    for o, layer in zip(low.ops, low.op_layer):
        if o.kind == _lib.OP_CONCAT_UPSAMPLE:
            assert o.c1 + o.c2 == g[low.values[o.dst][0]]["channels"]
            assert low.values[o.src][1][2] << o.up1 == low.values[o.dst][1][2] == o.conv.hout
        if o.kind == _lib.OP_CONV and not m._mfma:
            c2 = g[low.values[o.src2][0]]["channels"] if o.src2 != _lib.PLAN_NONE else 0
            assert o.c1 + c2 == o.conv.cin
            assert o.src == _lib.PLAN_INPUT or low.values[o.src][1][2] << o.up1 == o.conv.hin
        if o.kind == _lib.OP_CONV1X1_CAT:
            assert o.c1 + g[low.values[o.src2][0]]["channels"] == o.conv.cin and low.values[o.src][1][2] * 2 == low.values[o.src2][1][2] == o.conv.hin
        if o.res != _lib.PLAN_NONE:
            assert low.values[o.res][1] == low.values[o.dst][1]
    rows = [o.row_offset for o in low.ops if o.kind == _lib.OP_DECODE]
    per_head = [y.num_anchors * (S >> e["log2_down"]) ** 2 for y, e in zip(m.yolo_layers, (e for e in g if e["type"] == "yolo"))]
    assert rows == [int(v) for v in np.cumsum([0] + per_head[:-1])] and sum(per_head) == m.num_boxes(S)
    if m._mfma:
        check_plan_arena(low.ops, low.value_bytes, S, m.num_boxes(S), int(m.precision == "fp16"))


def test_every_listed_arm_is_reached():
    """the arms that no test reached on the YOLOv3 cfg, each named by the op tuple that shows it in LOWERED"""
    L = tc.LOWERED
    assert tc.CAT(0, 64, 128) in L["A"]["default"] and tc.CAT(0, 64, 96) in L["A"]["default"]         # a same-resolution two-source route, copied
    assert tc.CAT(1, 128, 0) in L["A"]["default"] and tc.CAT(1, 64, 0) in L["B"]["default"]           # a lone lazy upsample, 16-bit
    assert tc.F32(7, 64, up1=1) in L["B"]["fp32"]                                                    # fp32 loader: upsample, no second source
    assert tc.F32(11, 64, src2=True) in L["A"]["fp32"] and tc.F32(9, 64, src2=True) in L["B"]["fp32"]  # fp32 loader: route without upsample
    assert tc._op("CONV1X1_CAT", c1=64, src2=True) in L["C"]["default"]                              # 64|128 split
    assert tc.CONV(2, res=True) in L["B"]["default"]                                                 # shortcut fused into a 1x1
    assert L["B"]["default"][:2] == [tc.STEM, tc.CONV(1)]                                            # OP_STEM + a plain layer 1
    assert L["A"]["block128"].count(tc.RESBLOCK) == 2                                                # the C=128 fused block


@pytest.mark.parametrize("name", list(tc.GRAPHS))
def test_oracle_runs_every_graph(tmp_cfg_dir, name):
    """the reference evaluates every graph (maxpool aside, which neither side has); its row count is Darknet.num_boxes"""
    if name == "maxpool":
        with pytest.raises(NotImplementedError, match="maxpool"):
            Darknet(tc.write(name, tmp_cfg_dir))
        return
    rows, layers = tc.oracle_forward(name, tmp_cfg_dir, S, B, START)
    m = Darknet(tc.write(name, tmp_cfg_dir), precision="fp32")
    assert rows.shape == (B, m.num_boxes(S), 5 + tc.CLASSES) and len(layers) == len(m._graph)
    assert bool(torch.isfinite(rows).all())
    for e, t in zip(m._graph, layers):
        if e["type"] != "yolo":
            assert tuple(t.shape) == (B, e["channels"], S >> e["log2_down"], S >> e["log2_down"])


PAIRS = [(name, p) for name in tc.GRAPHS if name != "maxpool" for p in ("bf16", "fp16", "fp32")]


@pytest.mark.parametrize("name,precision", PAIRS, ids=lambda v: str(v))
def test_refused_or_lowered(tmp_cfg_dir, name, precision):
    """every (graph, precision) either lowers -- and is then in LOWERED, so a GPU test compares it with the oracle -- or raises
    NotImplementedError that names the layer, from the checks _prepare runs first or from _lower: before any launch"""
    m = Darknet(tc.write(name, tmp_cfg_dir), precision=precision)
    layer = tc.REFUSED.get((name, precision))
    if layer is None:
        option_set = {"bf16": "default"}.get(precision, precision)
        assert option_set in tc.LOWERED[name]
        m._check_16bit_layers()
        m._lower(B, S, fake_prep(m))
        return
    with pytest.raises(NotImplementedError, match=rf"layer {layer}\b"):
        m._check_16bit_layers()
        m._lower(B, S, fake_prep(m))


# ---------------------------------------------------------------------------------------------------------------- the reference's spread
def close_err(a, b):
    """the measure of test_gpu_parity.close"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max(initial=0.0))


def spread_figures(name, cfg_dir, mode):
    """OracleDarknet with fp32 convolution sums against float64 ones on graph `name`: fp32 -> the close-style error over the rows and
    every layer; 16-bit -> (largest share of a layer's stored activations outside test_model_bf16_vs_bf16_oracle's per-layer bound,
    largest head-logit difference)"""
    (rows_a, lay_a), (rows_b, lay_b) = (tc.oracle_forward(name, cfg_dir, S, B, START, mode=mode, conv_f64=f) for f in (False, True))
    defs = tc.synth_weights(name, cfg_dir)[1][1:]
    if mode == "fp32":
        return max([close_err(rows_a, rows_b)] + [close_err(a, b) for a, b, d in zip(lay_a, lay_b, defs) if d["type"] != "yolo"])
    k = 1.0 if mode == "bf16" else 0.125
    share, head = 0.0, 0.0
    for a, b, d in zip(lay_a, lay_b, defs):
        if d["type"] not in ("convolutional", "shortcut", "route"):
            continue
        err = (a - b).abs()
        if d["type"] == "convolutional" and not int(d["batch_normalize"]):
            head = max(head, float(err.max()))
        else:
            share = max(share, float((err > (b.abs() * 2.0 ** -6 + 0.03) * k).float().mean()))
    return share, head


SPREAD_GRAPHS = tc.MAIN + tc.FP32_ONLY + ("cat_into_shortcut",)


@pytest.mark.parametrize("name", SPREAD_GRAPHS)
def test_oracle_spread_fp32(tmp_cfg_dir, name):
    """two evaluations of the fp32 contract (ATen's summation order, exact sums) agree to 1e-5 on rows and layers: the device is
    held to 1e-4"""
    err = spread_figures(name, tmp_cfg_dir, "fp32")
    print(f"oracle spread {name} fp32: {err:.2e}")
    assert err <= 1e-5, err


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
@pytest.mark.parametrize("name", tc.MAIN + ("cat_into_shortcut",))
def test_oracle_spread_16bit(tmp_cfg_dir, name, mode):
    """two evaluations of the 16-bit contract: at most 5e-4 of a layer's stored activations outside the per-layer bound (a quarter of
    the 2e-3 the device is allowed), head logits within 0.05 k (a tenth of the device's 0.5 k)"""
    share, head = spread_figures(name, tmp_cfg_dir, mode)
    print(f"oracle spread {name} {mode}: share outside the bound {share:.2e}, head logits {head:.2e}")
    k = 1.0 if mode == "bf16" else 0.125
    assert share <= 5e-4 and head <= 0.05 * k, (share, head)
