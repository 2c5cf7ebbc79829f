"""Small cfg graphs beyond the 107-block YOLOv3 topology: every arm of the graph lowering (Darknet._analyse / _lower, ay_plan_create)
and of the two training engines that cfg_gen.yolov3_cfg_text never reaches, plus graphs the lowering refuses.

All graphs take 3 input channels, 2 classes, cfg_gen.ANCHORS and a 3x3 stride-1 stem.  Notation of the comments: c(f,k,s) conv + BN + leaky,
lin = linear activation, head(n) = 1x1 convolution without BN, sc(from) shortcut.

LOWERED[name][option set] is the op list Darknet._lower must give, one tuple per op:
    (kind, layer of an OP_CONV | None, up1, c1, c2, carries a residual, carries a second source, row_offset of a decode | None)
written down from the graph by hand and checked by tests/test_topology_cpu.py; the GPU tests run exactly these lists."""
import os

from amyloid_yolo_paper_amd import cfg_gen
from amyloid_yolo_paper_amd.cfg_gen import _conv

CLASSES = 2
K = 5 + CLASSES


def c(filters, size, stride=1, act="leaky"):
    return _conv(filters, size, stride, True, act)


def head(filters):
    return _conv(filters, 1, 1, False, "linear")


def sc(frm):
    return ["[shortcut]", f"from={frm}", "activation=linear", ""]


def route(*layers):
    return ["[route]", "layers = " + ", ".join(str(v) for v in layers), ""]


def up():
    return ["[upsample]", "stride=2", ""]


def yolo(*mask):
    return ["[yolo]", "mask = " + ",".join(str(v) for v in mask), f"anchors = {cfg_gen.ANCHORS}", f"classes={CLASSES}", "num=9", "jitter=.3",
            "ignore_thresh = .7", "truth_thresh = 1", "random=1", ""]


def maxpool():
    return ["[maxpool]", "size=2", "stride=2", ""]


def _net(size=64):
    return ["[net]", "batch=16", "subdivisions=1", f"width={size}", f"height={size}", "channels=3", "momentum=0.9", "decay=0.0005", ""]


def _text(blocks):
    out = _net()
    for b in blocks:
        out += b
    return "\n".join(out) + "\n"


GRAPHS = {
    # layer:  0        1            2        3        4       5             6        7         8      9         10             11
    "A": [c(32, 3), c(64, 3, 2), c(32, 1), c(64, 3), sc(-3), c(128, 3, 2), c(64, 1), c(128, 3), sc(-3), c(64, 1), route(-1, -2), c(96, 3),
          # 12           13         14    15         16        17             18         19        20             21         22        23
          c(256, 3, 2), c(128, 1), up(), route(-1), c(64, 3), route(-1, 11), c(128, 1), head(21), yolo(0, 1, 2), route(13), head(28),
          yolo(3, 4, 5, 6)],
    # layer:  0        1            2        3       4             5        6     7         8             9          10        11
    "B": [c(32, 3), c(64, 3, 1), c(64, 1), sc(-2), c(128, 3, 2), c(64, 1), up(), c(64, 3), route(-1, 3), c(128, 1), head(14), yolo(0, 1),
          # 12       13           14                    15        16
          route(4), c(64, 3, 2), c(64, 1, 1, "linear"), head(42), yolo(3, 4, 5, 6, 7, 8)],
    # layer:  0        1            2             3             4        5     6             7          8         9
    "C": [c(32, 3), c(64, 3, 2), c(128, 3, 2), c(256, 3, 2), c(64, 1), up(), route(-1, 2), c(128, 1), head(21), yolo(0, 1, 2)],
    # ---- graphs a lowering refuses (or one precision does)
    # the convolution in front of the shortcut has a second reader, so the add cannot ride its epilogue
    "shortcut_shared": [c(32, 3), c(64, 3, 2), c(64, 1), sc(-2), route(2), head(21), yolo(0, 1, 2)],
    "route3": [c(32, 3), c(64, 3, 2), c(64, 1), c(64, 1), route(-1, -2, -3), head(21), yolo(0, 1, 2)],
    "anchors7": [c(32, 3), c(64, 3, 2), head(49), yolo(0, 1, 2, 3, 4, 5, 6)],
    "stem16": [c(16, 3), c(32, 3, 2), c(64, 3, 2), head(21), yolo(0, 1, 2)],
    "bn48": [c(32, 3), c(48, 3, 2), c(64, 1), head(21), yolo(0, 1, 2)],
    # layer:                  0        1         2         3              4         5       6         7
    "cat_into_shortcut": [c(32, 3), c(32, 1), c(32, 1), route(-1, -2), c(64, 1), sc(-2), head(21), yolo(0, 1, 2)],
    "maxpool": [c(32, 3), maxpool(), head(21), yolo(0, 1, 2)],
}

MAIN = ("A", "B", "C")
FP32_ONLY = ("stem16", "bn48")                 # the 16-bit lowering refuses them; precision="fp32" runs them
ORACLE_GRAPHS = tuple(n for n in GRAPHS if n != "maxpool")   # the oracle has no maxpool either


def cfg_text(name):
    return _text(GRAPHS[name])


def write(name, directory):
    """Write (once) and return the path of the cfg of graph `name`, in the manner of cfg_gen.write_cfg."""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, f"topology-{name}.cfg")
    text = cfg_text(name)
    if not os.path.exists(path) or open(path).read() != text:
        tmp = path + f".tmp{os.getpid()}"
        with open(tmp, "w") as fh:
            fh.write(text)
        os.replace(tmp, path)
    return path


# ---------------------------------------------------------------------------------------------------------------- option sets
OPTION_SETS = {
    "default": dict(),
    "block128": dict(fuse_block_channels=(64, 128)),
    "unfused": dict(fold_routes=False, fuse_blocks=False, stem_mode="fp32"),
    "fp16": dict(precision="fp16"),
    "fp32": dict(precision="fp32"),
}
PLAN_OPTION_SETS = ("default", "block128", "unfused", "fp16")     # the 16-bit ones: what ay_plan_create takes


def apply_options(m, option_set, precision=None):
    """set the attributes of an option set on a Darknet (`precision`: instead of the option set's own storage type);
    fuse_block_channels is read by _analyse, which is run again"""
    opts = dict(OPTION_SETS[option_set])
    m.precision = precision or opts.pop("precision", "bf16")
    opts.pop("precision", None)
    for k, v in opts.items():
        setattr(m, k, v)
    if "fuse_block_channels" in opts:
        m._graph = m._analyse()
    m._prep = None
    return m


# ---------------------------------------------------------------------------------------------------------------- expected op lists
def _op(kind, layer=None, up1=0, c1=0, c2=0, res=False, src2=False, row=None):
    return (kind, layer, up1, c1, c2, res, src2, row)


def CONV(layer, res=False):
    return _op("CONV", layer, res=res)


def F32(layer, c1, up1=0, res=False, src2=False):
    """an fp32 convolution: its loader reads c1 channels of src (x2 upsampled when up1), then src2's"""
    return _op("CONV", layer, up1=up1, c1=c1, res=res, src2=src2)


def CAT(up1, c1, c2):
    return _op("CONCAT_UPSAMPLE", up1=up1, c1=c1, c2=c2, src2=c2 > 0)


def DECODE(row):
    return _op("DECODE", row=row)


STEM_S2, STEM, RESBLOCK = _op("STEM_S2_FUSED"), _op("STEM"), _op("RESBLOCK")

# rows per image at S = 64, which the row offsets below are for: A 3*16*16 + 4*8*8, B 2*64*64 + 6*16*16, C 3*16*16
LOWER_S, LOWER_B = 64, 2

_A_TAIL = [CONV(9), CAT(0, 64, 128), CONV(11), CONV(12), CONV(13), CAT(1, 128, 0), CONV(16), CAT(0, 64, 96), CONV(18), CONV(19), DECODE(0),
           CONV(22), DECODE(768)]
_A_DEFAULT = [STEM_S2, RESBLOCK, CONV(5), CONV(6), CONV(7, res=True)] + _A_TAIL
_B_DEFAULT = [STEM, CONV(1), CONV(2, res=True), CONV(4), CONV(5), CAT(1, 64, 0), CONV(7), CAT(0, 64, 64), CONV(9), CONV(10), DECODE(0),
              CONV(13), CONV(14), CONV(15), DECODE(8192)]
_C_DEFAULT = [STEM_S2, CONV(2), CONV(3), CONV(4), _op("CONV1X1_CAT", c1=64, src2=True), CONV(8), DECODE(0)]
_C_UNFOLDED = [CONV(2), CONV(3), CONV(4), CAT(1, 64, 128), CONV(7), CONV(8), DECODE(0)]

_CIS_DEFAULT = [STEM, CONV(1), CONV(2), CAT(0, 32, 32), CONV(4, res=True), CONV(6), DECODE(0)]

LOWERED = {
    "A": {
        "default": _A_DEFAULT,
        "block128": [STEM_S2, RESBLOCK, CONV(5), RESBLOCK] + _A_TAIL,
        "unfused": [STEM, CONV(1), CONV(2), CONV(3, res=True), CONV(5), CONV(6), CONV(7, res=True)] + _A_TAIL,
        "fp16": _A_DEFAULT,
        "fp32": [F32(0, 3), F32(1, 32), F32(2, 64), F32(3, 32, res=True), F32(5, 64), F32(6, 128), F32(7, 64, res=True), F32(9, 128),
                 F32(11, 64, src2=True), F32(12, 96), F32(13, 256), CAT(1, 128, 0), F32(16, 128), F32(18, 64, src2=True), F32(19, 128),
                 DECODE(0), F32(22, 128), DECODE(768)],
    },
    "B": {
        "default": _B_DEFAULT,
        "block128": _B_DEFAULT,
        "unfused": _B_DEFAULT,
        "fp16": _B_DEFAULT,
        "fp32": [F32(0, 3), F32(1, 32), F32(2, 64, res=True), F32(4, 64), F32(5, 128), F32(7, 64, up1=1), F32(9, 64, src2=True), F32(10, 128),
                 DECODE(0), F32(13, 128), F32(14, 64), F32(15, 64), DECODE(8192)],
    },
    "C": {
        "default": _C_DEFAULT,
        "block128": _C_DEFAULT,
        "unfused": [STEM, CONV(1)] + _C_UNFOLDED,
        "fp16": _C_DEFAULT,
        "fp32": [F32(0, 3), F32(1, 32), F32(2, 64), F32(3, 128), F32(4, 256), F32(7, 64, up1=1, src2=True), F32(8, 128), DECODE(0)],
    },
    # the 16-bit lowering of a two-source route that a shortcut reads as well: materialised, the 1x1 carries the residual
    "cat_into_shortcut": {
        "default": _CIS_DEFAULT,
        "fp16": _CIS_DEFAULT,
        # fp32: the convolution's loader reads the two sources, the shortcut reads the materialised copy (two channel copies)
        "fp32": [F32(0, 3), F32(1, 32), F32(2, 32), CAT(0, 32, 32), F32(4, 32, res=True, src2=True), F32(6, 64), DECODE(0)],
    },
    "stem16": {"fp32": [F32(0, 3), F32(1, 16), F32(2, 32), F32(3, 64), DECODE(0)]},
    "bn48": {"fp32": [F32(0, 3), F32(1, 32), F32(2, 48), F32(3, 64), DECODE(0)]},
}

# (graph, precision) -> the layer the NotImplementedError names, before anything is launched; every other pair of a graph listed in
# LOWERED lowers and must then agree with the oracle
REFUSED = {
    ("shortcut_shared", "bf16"): 3, ("shortcut_shared", "fp16"): 3, ("shortcut_shared", "fp32"): 3,
    ("route3", "bf16"): 4, ("route3", "fp16"): 4, ("route3", "fp32"): 4,
    ("anchors7", "bf16"): 3, ("anchors7", "fp16"): 3, ("anchors7", "fp32"): 3,
    ("stem16", "bf16"): 0, ("stem16", "fp16"): 0,
    ("bn48", "bf16"): 1, ("bn48", "fp16"): 1,           # Darknet._check_16bit_layers, the first thing _prepare does
}


# ---------------------------------------------------------------------------------------------------------------- the reference
_ORACLE = {}
_PARAMS = {}


def synth_weights(name, directory):
    """(cfg path, parsed blocks with [net], synth.synth_params(seed=7), path of the Darknet .weights file) of graph `name`"""
    from amyloid_yolo_paper_amd import parse_config, synth
    if name not in _PARAMS:
        cfg = write(name, directory)
        defs = parse_config.parse_model_config(cfg)
        params = synth.synth_params(defs, seed=7)
        wpath = os.path.join(directory, f"topology-{name}.weights")
        synth.write_darknet_weights(wpath, defs, params, seen=0)
        _PARAMS[name] = (cfg, defs, params, wpath)
    return _PARAMS[name]


def oracle_forward(name, directory, S, B, start, mode="fp32", conv_f64=False, stem_bf16=True):
    """OracleDarknet of graph `name` on golden_cases.model_inputs(S, B, start): (rows [B,N,7], list of layer outputs), computed once
    per argument set and shared; callers must not write into the tensors."""
    import torch
    import golden_cases as gc
    from oracle.darknet_oracle import OracleDarknet
    key = (name, S, B, start, mode, conv_f64, stem_bf16)
    if key not in _ORACLE:
        cfg, _, params, _ = synth_weights(name, directory)
        o = OracleDarknet(cfg)
        o.set_params(params)
        o.conv_f64 = conv_f64
        with torch.no_grad():
            rows = o.forward(torch.from_numpy(gc.model_inputs(S, B, start)), mode=mode, collect=True, stem_bf16=stem_bf16)
        _ORACLE[key] = (rows, o.layer_outputs)
    return _ORACLE[key]
