"""ctypes binding of libamyloid_yolo_hip.so (the C ABI declared in include/amyloid_yolo.h).

The signatures (``_SIGS``) and the ``AY_*`` constants (``CONSTANTS``) are read from that header at import: a new entry point takes its
prototype there and its definition in a ``.hip`` file, and no line here.  Only the structs are restated (tests/test_abi_cpu.py holds
their fields against the header's).

``include/amyloid_yolo.h`` is a frozen list of prototypes (tests/golden/abi_sigs.json, ``AY_ABI_VERSION``).  Entry points added after
the freeze are declared in the headers of ``MORE_HEADER_PATHS`` and read into a second table, ``_SIGS_MORE``; their constants join
``CONSTANTS``, and ``lib()`` binds both tables.

There is no CPU fallback: if the HIP library is missing or a call fails this raises.
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libamyloid_yolo_hip.so")
HEADER_PATH = os.path.join(HERE, "..", "include", "amyloid_yolo.h")   # where build.py finds it
MORE_HEADER_PATHS = (os.path.join(HERE, "..", "include", "amyloid_yolo_spatial_sim.h"),)


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "batch", "cin", "cout", "hin", "win", "hout", "wout", "ksize", "stride", "leaky", "out_f32", "cout_pad")]


class PlanOp(C.Structure):
    """ay_plan_op (include/amyloid_yolo.h)"""
    _fields_ = [("kind", C.c_int32), ("src", C.c_int32), ("src2", C.c_int32), ("res", C.c_int32), ("dst", C.c_int32),
                ("conv", ConvDesc), ("c1", C.c_int32), ("c2", C.c_int32), ("up1", C.c_int32), ("leaky2", C.c_int32),
                ("num_anchors", C.c_int32), ("num_classes", C.c_int32), ("grid", C.c_int32), ("row_offset", C.c_int32),
                ("anchors_wh", C.c_float * 12),
                ("w", C.c_void_p), ("scale", C.c_void_p), ("shift", C.c_void_p),
                ("w2", C.c_void_p), ("scale2", C.c_void_p), ("shift2", C.c_void_p)]


class AugParams(C.Structure):
    """ay_aug_params (include/amyloid_yolo.h, THE AUGMENTATION RULE): one record per image of ay_augment_ingest_u8"""
    _fields_ = [("src_offset", C.c_int64), ("h", C.c_int32), ("w", C.c_int32), ("inv", C.c_float * 6), ("flip", C.c_int32),
                ("sharpen_alpha", C.c_float), ("drop_threshold", C.c_uint32), ("drop_seed", C.c_uint32),
                ("color", C.c_float * 9), ("bright", C.c_float)]


class AugWindowParams(C.Structure):
    """ay_aug_window_params (include/amyloid_yolo.h, THE WINDOW RULE): one record per image of ay_augment_ingest_window_u8"""
    _fields_ = [("src_offset", C.c_int64), ("row_stride", C.c_int64), ("bh", C.c_int32), ("bw", C.c_int32), ("x0", C.c_int32),
                ("y0", C.c_int32), ("context", C.c_int32), ("fill", C.c_float), ("aug", AugParams)]


class StainParams(C.Structure):
    """ay_stain_params (include/amyloid_yolo.h, THE STAIN RULE): the tables of one stain map, uploaded once per slide"""
    _fields_ = [("od", C.c_float * 256), ("D", C.c_float * 9), ("A", C.c_float * 9), ("T", C.c_float * 257)]


class StainBasisParams(C.Structure):
    """ay_stain_basis_params (include/amyloid_yolo.h, THE BASIS RULE): the integer optical density of every byte"""
    _fields_ = [("odq", C.c_int32 * 256)]


class AyError(RuntimeError):
    pass


_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
            "int64_t": C.c_int64, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "ay_stream_t": C.c_void_p}


def _ctype(decl, proto, is_return=False):
    """One parameter (``const float* w``, ``size_t n``) or return type of a prototype -> its ctypes type.  Every pointer travels as
    ``c_void_p`` (callers hand over ``byref``, ctypes arrays, ``c_void_p`` or None), except a returned ``const char*``."""
    words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    if "*" in words:
        return C.c_char_p if is_return and words == ["char", "*"] else C.c_void_p
    base = " ".join(words if is_return or len(words) == 1 else words[:-1])       # a parameter's last word is its name
    if is_return and base == "void":
        return None
    if base not in _SCALARS:
        raise AyError(f"{HEADER_PATH}: no ctypes type for `{decl.strip()}` in `{proto}`")
    return _SCALARS[base]


def parse_header(text):
    """The text of include/amyloid_yolo.h -> (signatures, constants): ``name -> (restype, [argtypes])`` of every ``ret ay_name(args);``
    and the value of every integer ``#define AY_*`` and of the enumerators.  A type outside the map above is an ``AyError`` that
    names the prototype, never a default."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    constants = {name: int(value) for name, value in re.findall(r"^#define\s+(AY_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in filter(None, map(str.strip, body.split(","))):
            m = re.fullmatch(r"(AY_\w+)\s*=\s*(-?\d+)", item)
            if not m:
                raise AyError(f"{HEADER_PATH}: enumerator `{item}` has no integer value written out")
            constants[m.group(1)] = int(m.group(2))
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    sigs = {}
    for ret, name, params in re.findall(r"([\w*][\w\s*]*?)\b(ay_\w+)\s*\(([^()]*)\)\s*;", text):
        proto = " ".join(f"{ret}{name}({params})".split())
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_ctype(ret, proto, is_return=True), [_ctype(p, proto) for p in params])
    unread = set(re.findall(r"\b(ay_\w+)\s*\(", text)) - set(sigs)
    if unread:
        raise AyError(f"{HEADER_PATH}: cannot read the prototype of {sorted(unread)}")
    return sigs, constants


def _read_header(path=None):
    path = HEADER_PATH if path is None else path
    if not os.path.exists(path):
        raise AyError(f"{path} is missing: the ctypes signatures and the AY_* constants are read from it")
    with open(path) as f:
        return parse_header(f.read())


_SIGS, CONSTANTS = _read_header()
_SIGS_MORE = {}
for _path in MORE_HEADER_PATHS:
    _sigs, _constants = _read_header(_path)
    if set(_sigs) & (set(_SIGS) | set(_SIGS_MORE)) or set(_constants) & set(CONSTANTS):
        raise AyError(f"{_path} declares a name that an earlier header has")
    _SIGS_MORE.update(_sigs)
    CONSTANTS.update(_constants)
ABI_VERSION = CONSTANTS["AY_ABI_VERSION"]      # lib() compares it with ay_version() of the library it loads
PLAN_INPUT, PLAN_NONE = CONSTANTS["AY_PLAN_INPUT"], CONSTANTS["AY_PLAN_NONE"]
(OP_STEM_S2_FUSED, OP_STEM, OP_CONV, OP_RESBLOCK, OP_CONV1X1_CAT, OP_CONCAT_UPSAMPLE, OP_DECODE) = (
    CONSTANTS["AY_OP_" + n] for n in ("STEM_S2_FUSED", "STEM", "CONV", "RESBLOCK", "CONV1X1_CAT", "CONCAT_UPSAMPLE", "DECODE"))

_lib = None


def exported_symbols():
    return sorted(_SIGS)


def exported_symbols_more():
    """the entry points declared behind the frozen header (``MORE_HEADER_PATHS``)"""
    return sorted(_SIGS_MORE)


def lib():
    """The loaded library (loads on first use)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AyError(
                f"{LIB_PATH} is missing: build it with `python -m amyloid_yolo_paper_amd.build` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the hot path.")
        l = C.CDLL(LIB_PATH)
        l.ay_version.restype = C.c_int
        have = l.ay_version()
        if have != ABI_VERSION:   # a stale .so would take e.g. ay_plan_create's out pointer for a dtype: refuse it before any call
            raise AyError(f"{LIB_PATH} exports ABI version {have}, this binding needs {ABI_VERSION}: rebuild it "
                          "(python -m amyloid_yolo_paper_amd.build --force)")
        for name, (res, args) in list(_SIGS.items()) + list(_SIGS_MORE.items()):
            fn = getattr(l, name)  # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        _lib = l
    return _lib


def check(rc, what=""):
    if rc != 0:
        msg = lib().ay_last_error()
        raise AyError(f"{what} failed ({rc}): {msg.decode() if msg else ''}")


def ptr(t):
    """device (or host) pointer of a torch tensor, None -> NULL"""
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)
