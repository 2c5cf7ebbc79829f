"""CPU: the overlapping tile grid (wsi.tile_grid), the restatement of the seam-merge rule against hand-written cases (so that the
yardstick of tests/test_gpu_seam.py is itself pinned), and the new symbols in the library and in the ctypes table."""
import ctypes
import os

import numpy as np
import pytest

import seam_reference as sr
from amyloid_yolo_paper_amd import _lib, build, wsi

NEW_SYMBOLS = ["ay_ingest_region_tiles_step_u8", "ay_seam_append", "ay_seam_merge_workspace_bytes", "ay_seam_merge"]


def test_tile_grid_without_overlap_is_the_abutting_grid():
    for tile in (1, 7, 32, 1536):
        for extent in list(range(1, 200)) + [1535, 1536, 1537, 100000]:
            assert wsi.tile_grid(extent, 3 * extent + 1, tile) == (-(-extent // tile), -(-(3 * extent + 1) // tile), tile)
            assert wsi.tile_grid(extent, extent, tile, 0) == wsi.tile_grid(extent, extent, tile)


def test_tile_grid_with_overlap_covers_the_slide_and_wastes_no_tile():
    for tile, overlap in [(32, 1), (32, 8), (32, 31), (192, 48), (1536, 128), (5, 4)]:
        step = tile - overlap
        for extent in list(range(1, 4 * tile + 3)) + [100000]:
            ty, tx, s = wsi.tile_grid(extent, 2 * extent, tile, overlap)
            assert s == step
            for n, e in ((ty, extent), (tx, 2 * extent)):
                assert n >= 1
                assert (n - 1) * step + tile >= e                  # the tiles cover the slide
                if n > 1:
                    assert (n - 2) * step + tile < e               # and the last one is needed
                if e <= overlap:
                    assert n == 1                                  # an extent inside one overlap band: one tile


def test_tile_grid_refuses_an_overlap_that_leaves_no_step():
    for overlap in (32, 33, -1):
        with pytest.raises(ValueError):
            wsi.tile_grid(100, 100, 32, overlap)


@pytest.mark.parametrize("name", sorted(sr.hand_cases()))
def test_restatement_on_hand_cases(name):
    rows, tile_id, thres, expect = sr.hand_cases()[name]
    assert sr.seam_merge(rows, tile_id, thres).tolist() == expect
    assert sr.seam_merge_binned(rows, tile_id, thres).tolist() == expect


def test_restatement_hand_case_geometry():
    """the numbers the hand cases rely on"""
    c = np.asarray(sr.hand_cases()["chain"][0], np.float32)
    assert sr.ov(c[0, :4], c[1:2, :4])[0] == np.float32(0.6) and sr.ov(c[1, :4], c[2:3, :4])[0] == np.float32(0.6)
    assert sr.ov(c[0, :4], c[2:3, :4])[0] == np.float32(0.2)
    h = np.asarray(sr.hand_cases()["half_cut"][0], np.float32)
    assert sr.ov(h[0, :4], h[1:2, :4])[0] == 1.0
    inter, union = 50.0 * 100.0, 100.0 * 100.0
    assert inter / union == 0.5                                    # IoU of the half-cut box: not above a threshold of 0.5


def test_restatement_corner_chain_and_empty():
    rows, tile_id = sr.corner_case()
    assert sr.seam_merge(rows, tile_id).tolist() == [True, False, False, False, True]
    rows, tile_id = sr.staircase(320)
    keep = sr.seam_merge(rows, tile_id)
    assert keep.tolist() == [k % 2 == 0 for k in range(320)]
    assert (sr.seam_merge_binned(rows, tile_id) == keep).all()
    assert sr.seam_merge(np.zeros((0, 7), np.float32), np.zeros(0, np.int32)).shape == (0,)
    assert sr.seam_merge(rows[:1], tile_id[:1]).tolist() == [True]


@pytest.mark.slow
def test_binned_restatement_equals_the_plain_one_on_a_synthetic_slide():
    rows, tile_id = sr.synthetic_slide(3000, 6, 7, seed=1, big=3)
    keep = sr.seam_merge(rows, tile_id)
    assert (sr.seam_merge_binned(rows, tile_id) == keep).all()
    assert 0.2 <= 1.0 - keep.mean() <= 0.7


def test_library_exports_the_seam_symbols():
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library()
    dll = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(dll, name), f"{name} not exported"
        assert name in _lib.exported_symbols(), f"{name} not in the ctypes table"
        assert getattr(_lib.lib(), name).argtypes is not None
    assert "ay_seam.hip" in build.SOURCES
    L = _lib.lib()
    small, large = L.ay_seam_merge_workspace_bytes(0), L.ay_seam_merge_workspace_bytes(100000)
    assert 0 < small < large < 100000 * 200                       # linear in the rows, a few tens of bytes each


def test_seam_entry_points_refuse_bad_arguments():
    """host-side argument checks, no GPU"""
    L = _lib.lib()
    p = ctypes.c_void_p(0x1000)
    assert L.ay_seam_append(None, p, 1, 8, ctypes.c_float(1.0), p, p, p, p, p, 8, None) == -1
    assert L.ay_seam_append(p, p, 1, 8, ctypes.c_float(1.0), p, p, p, p, p, 0, None) == -1
    assert L.ay_ingest_region_tiles_step_u8(p, 8, 8, 24, 1, 8, 9, 1, 1, 8, p, None) == -1       # step > tile
    assert L.ay_ingest_region_tiles_step_u8(p, 8, 8, 24, 1, 8, 0, 1, 1, 8, p, None) == -1       # no step
    assert L.ay_seam_merge(p, p, -1, ctypes.c_float(0.5), p, p, p, 1 << 20, None) == -1
