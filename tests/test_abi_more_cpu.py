"""CPU: the entry points declared behind the frozen header (include/amyloid_yolo_spatial_sim.h) are exported and bound, and the frozen
table is what it was."""
import ctypes
import os
import re

from amyloid_yolo_paper_amd import _lib, build

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name):
    text = open(os.path.join(REPO, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(ay_[a-z0-9_]+)\s*\(", text)))


def test_every_symbol_of_the_second_header_is_exported_and_bound():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    declared = header_symbols("amyloid_yolo_spatial_sim.h")
    assert declared == ["ay_pair_counts_relabel", "ay_pair_counts_relabel_workspace_bytes"]
    assert _lib.exported_symbols_more() == declared
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared:
        assert hasattr(dll, name), f"{name} declared in include/amyloid_yolo_spatial_sim.h but not exported"
    bound = _lib.lib()
    res, args = _lib._SIGS_MORE["ay_pair_counts_relabel"]
    assert bound.ay_pair_counts_relabel.restype is res is ctypes.c_int and list(bound.ay_pair_counts_relabel.argtypes) == args and len(args) == 24
    assert args[5] is ctypes.c_float and args[13] is ctypes.c_void_p and args[14] is args[15] is ctypes.c_int and args[22] is ctypes.c_size_t
    res, args = _lib._SIGS_MORE["ay_pair_counts_relabel_workspace_bytes"]
    assert bound.ay_pair_counts_relabel_workspace_bytes.restype is res is ctypes.c_size_t and args == [ctypes.c_int] * 9
    # the workspace size needs no device: 0 for arguments the call refuses, and the plain call's workspace is part of it
    f, plain = bound.ay_pair_counts_relabel_workspace_bytes, bound.ay_pair_counts_workspace_bytes(1000, 3072, 4096, 1024, 0)
    assert f(1000, 3, 6, 3072, 4096, 1024, 0, 0, 100) > plain > 0
    assert f(1000, 3, 6, 3072, 4096, 1024, 0, 16, 100) > f(1000, 3, 6, 3072, 4096, 1024, 0, 0, 100)
    for bad in ((1000, 0, 6, 3072, 4096, 1024, 0, 0, 100), (1000, 9, 6, 3072, 4096, 1024, 0, 0, 100), (1000, 3, 0, 3072, 4096, 1024, 0, 0, 100),
                (1000, 3, 33, 3072, 4096, 1024, 0, 0, 100), (1000, 3, 6, 3072, 4096, 1024, 0, 0, 0), (1000, 3, 6, 3072, 4096, 1024, 0, 0, 1025),
                (1000, 3, 6, 3072, 4096, 1024, 0, 8, 100), (1000, 3, 6, 3072, 4096, 1024, 1000, 0, 100), (-1, 3, 6, 3072, 4096, 1024, 0, 0, 100)):
        assert f(*bad) == 0, bad


def test_the_frozen_table_is_what_it_was():
    assert len(_lib._SIGS) == 128 and not set(_lib._SIGS) & set(_lib._SIGS_MORE)
    assert _lib.exported_symbols() == header_symbols("amyloid_yolo.h") and _lib.ABI_VERSION == 2


def test_the_constants_of_the_second_header_are_readable():
    assert _lib.CONSTANTS["AY_PAIR_RELABEL_MAX_SIMS"] == 1024 and _lib.CONSTANTS["AY_PAIR_RELABEL_FLAG_LABEL"] == 4
    assert _lib.CONSTANTS["AY_PAIR_MAX_CLASSES"] == 8 and _lib.CONSTANTS["AY_ABI_VERSION"] == 2          # and the first header's as before
