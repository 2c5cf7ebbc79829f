"""Rate and parity of the split-bf16 precisions against precision="fp32" in ONE process: yolov3-custom (cfg_gen, synthetic weights
of seed 7 as in bench.py), B tiles of S x S resident on the device, the three models built from the same parameters.
RATE: after WARM forwards per mode, ROUNDS rounds; in each round the modes take turns (fp32, bf16x6, bf16x3), each timing PER
forwards (convolution stack + decode, `forward_device`) between two device events.  Per mode: tiles/s from the sum of its blocks,
min .. max over the blocks, and the ratio to fp32's rate of the same run.  Repeat the script to get the spread between runs.
PARITY on the same batch, against the fp32 path: largest deviation |a - b| / max(1, |b|) of the output rows, of the rows with an
fp32 confidence above 0.5, largest confidence difference, whether NMS (0.5 / 0.4) keeps the same indices, and the layers with the
largest deviation of their outputs (`--layers N`; 0 skips the per-layer pass).
LAYER TIMES (`--layer-times N`): device events around every convolution launch of the host executor, N forwards, by layer shape.
usage: python scripts/bench_split.py [--batch 8] [--size 1024] [--rounds 4] [--per 5] [--warm 2] [--layers 5] [--layer-times 0]
                                     [--out FILE (appended)]"""
import argparse
import sys

import harness
import numpy as np
import torch

from amyloid_yolo_paper_amd import cfg_gen, parse_config, synth
from amyloid_yolo_paper_amd import utils as ay
from amyloid_yolo_paper_amd.models import Darknet

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--classes", type=int, default=2)
ap.add_argument("--rounds", type=int, default=4)
ap.add_argument("--per", type=int, default=5, help="forwards per timed block")
ap.add_argument("--warm", type=int, default=2)
ap.add_argument("--layers", type=int, default=5, help="report that many layers with the largest deviation from the fp32 path")
ap.add_argument("--layer-times", type=int, default=0, help="time every convolution launch over that many forwards, by layer shape")
ap.add_argument("--modes", default="fp32,bf16x6,bf16x3")
ap.add_argument("--cfg-dir", default=None, help="where to write the generated cfg (default: a temporary directory)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
MODES = a.modes.split(",")
assert MODES[0] == "fp32", "the first mode is the reference of the ratios"
assert a.rounds * a.per >= 20, "at least 20 timed forwards per mode"

report = harness.Report()
say = report.say

if not torch.cuda.is_available():
    sys.exit("bench_split.py measures on the GPU: no HIP device")
dev = torch.device("cuda", 0)
if a.cfg_dir is None:
    import tempfile
    _tmp = tempfile.TemporaryDirectory()
    a.cfg_dir = _tmp.name
cfg = cfg_gen.write_cfg(a.classes, a.cfg_dir)
params = synth.synth_params(parse_config.parse_model_config(cfg), seed=7)


def make_model(precision):
    m = Darknet(cfg, img_size=a.size, precision=precision)
    sd = m.state_dict()
    for i, p in params.items():
        for k, name in (("weight", f"conv_{i}.weight"), ("bias", f"conv_{i}.bias"), ("gamma", f"batch_norm_{i}.weight"),
                        ("beta", f"batch_norm_{i}.bias"), ("mean", f"batch_norm_{i}.running_mean"), ("var", f"batch_norm_{i}.running_var")):
            if k in p:
                sd[f"module_list.{i}.{name}"].copy_(torch.from_numpy(p[k]))
    return m.to(dev).eval()


B, S = a.batch, a.size
models = {p: make_model(p) for p in MODES}
x = torch.from_numpy(synth.synth_tiles(B, S, start=0)).to(dev)

say(f"# split-bf16 precisions against precision='fp32' on {torch.cuda.get_device_name(0)}: yolov3-custom ({a.classes} classes), B = {B} at "
    f"{S}^2, one process; {a.warm} warm forwards per mode, then {a.rounds} rounds of [{' | '.join(MODES)}] x {a.per} forwards between "
    f"two device events (forward_device: convolution stack + decode)")
forwards = [lambda p=p: models[p].forward_device(x) for p in MODES]
harness.time_calls(forwards, a.warm, 0)
blocks = dict(zip(MODES, harness.time_calls(forwards, 0, a.rounds, per=a.per)))
rate = {p: B * 1e3 * len(blocks[p]) / sum(blocks[p]) for p in MODES}
for p in MODES:
    ms = blocks[p]
    say(f"{p:7s} {rate[p]:9.1f} tiles/s   {sum(ms) / len(ms):8.2f} ms per forward (blocks {min(ms):.2f} .. {max(ms):.2f})   "
        f"x{rate[p] / rate['fp32']:.3f} of fp32   (block ratios to fp32 of the same round: "
        f"{', '.join(f'{f / m:.3f}' for f, m in zip(blocks['fp32'], ms))})")


def deviation(got, ref):
    return float(((got.double() - ref.double()).abs() / ref.double().abs().clamp_min(1.0)).max()) if ref.numel() else 0.0


say("# parity on this batch against the fp32 path: deviation = largest |a - b| / max(1, |b|)")
outs = {p: models[p].forward_device(x).clone() for p in MODES}
keep = {p: ay.non_max_suppression(o.cpu(), 0.5, 0.4).keep_idx for p, o in outs.items()}
sel = outs["fp32"][..., 4] > 0.5
for p in MODES[1:]:
    same = sum(int(np.array_equal(u, v)) for u, v in zip(keep[p], keep["fp32"]))
    say(f"{p:7s} rows: deviation {deviation(outs[p], outs['fp32']):.3e}; {int(sel.sum())} rows with fp32 confidence > 0.5: "
        f"{deviation(outs[p][sel], outs['fp32'][sel]):.3e}; largest confidence difference "
        f"{float((outs[p][..., 4] - outs['fp32'][..., 4]).abs().max()):.3e}; NMS kept indices equal to fp32's in {same} of {B} tiles")
if a.layers > 0:
    for m in models.values():
        m.keep_layer_outputs = True
        m.forward_device(x)
    ref = models["fp32"].layer_outputs
    for p in MODES[1:]:
        devs = sorted(((deviation(t, ref[i]), i) for i, t in models[p].layer_outputs.items()), reverse=True)
        say(f"{p:7s} layer outputs, largest deviations (layer: deviation): " + ", ".join(f"{i}: {d:.2e}" for d, i in devs[:a.layers])
            + f"; median over {len(devs)} layers {devs[len(devs) // 2][0]:.2e}")
if a.layer_times:
    # device events around every convolution launch of the host executor (Darknet.profile_layers), summed per layer shape
    import collections
    for m in models.values():
        m.keep_layer_outputs = False
    g = models["fp32"]._graph
    convs = {i for i, e in enumerate(g) if e["type"] == "convolutional"}
    ms = {}
    for p in MODES:
        m = models[p]
        m.forward_device(x)
        m.profile_layers, m.profile_events = convs, []
        for _ in range(a.layer_times):
            m.forward_device(x)
        torch.cuda.synchronize()
        ms[p] = collections.defaultdict(float)
        for layer, e0, e1 in m.profile_events:
            ms[p][layer] += e0.elapsed_time(e1) / a.layer_times
        m.profile_layers = None
    shapes = collections.defaultdict(lambda: [0, 0.0] + [0.0] * len(MODES))
    for i in sorted(convs):
        e, h = g[i], S >> g[i]["log2_down"]
        v = shapes[(e["k"], e["stride"], e["cin"], e["cout"], h)]
        v[0] += 1
        v[1] += 2.0 * B * h * h * e["cin"] * e["cout"] * e["k"] ** 2 / 1e9
        for j, p in enumerate(MODES):
            v[2 + j] += ms[p][i]
    say(f"# convolution launches by layer shape (k, stride, cin, cout, hout): ms per forward between two device events per launch, mean of "
        f"{a.layer_times} forwards; ratios are fp32's time over the mode's")
    say(f"{'shape':28s} {'n':>3s} {'GFLOP':>8s} " + " ".join(f"{p:>8s}" for p in MODES) + "  " + " ".join(f"{p + '/fp32':>11s}" for p in MODES[1:]))
    for key, v in sorted(shapes.items(), key=lambda kv: -kv[1][2]):
        say(f"{str(key):28s} {v[0]:3d} {v[1]:8.1f} " + " ".join(f"{t:8.3f}" for t in v[2:]) + "  " + " ".join(f"{v[2] / t:11.2f}" for t in v[3:]))
    say("all convolutions" + " " * 25 + " ".join(f"{sum(v[2 + j] for v in shapes.values()):8.3f}" for j in range(len(MODES))))
report.write(a.out, append=True)
