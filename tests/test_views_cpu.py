"""CPU: the view and vote rules' NumPy restatement is self-consistent; views.check_views; detect_region / RegionTileStream reject
bad view arguments before any device use; the four entry points of csrc/ay_views.hip are in the header, the binding and the
library, refuse bad arguments on the host, and their kernels use no scratch memory."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import views_reference as vr
from amyloid_yolo_paper_amd import _lib, build
from amyloid_yolo_paper_amd.views import ALL_VIEWS, FLIPS, check_views
from amyloid_yolo_paper_amd.wsi import RegionTileStream, detect_region

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ay_ingest_region_tiles_views_u8", "ay_unview_rows", "ay_view_votes", "ay_view_select")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [5, 8])
def test_box_rule_is_the_inverse_of_the_pixel_rule(S):
    """the centre of view pixel (x, y) goes back to the centre of the pixel of I0 it shows, for every view"""
    for v in ALL_VIEWS:
        for y in range(S):
            for x in range(S):
                sx, sy = vr.source_pixel(v, x, y, S)
                X, Y, W, H = vr.unview_box(v, x + 0.5, y + 0.5, 2.0, 3.0, S)
                assert (float(X), float(Y)) == (sx + 0.5, sy + 0.5)
                assert (float(W), float(H)) == ((3.0, 2.0) if v & 4 else (2.0, 3.0))


@pytest.mark.parametrize("S", [5, 8])
def test_views_of_an_asymmetric_image_differ_and_view_0_is_the_identity(S):
    img = np.arange(3 * S * S, dtype=np.float32).reshape(3, S, S)
    views = [vr.view_image(img, v) for v in ALL_VIEWS]
    assert np.array_equal(views[0], img)
    for i in range(8):
        assert np.array_equal(views[i], vr.view_image_fast(img, i))          # flips, then the transpose
        assert np.array_equal(np.sort(views[i].ravel()), np.sort(img.ravel()))   # a permutation
        for j in range(i):
            assert not np.array_equal(views[i], views[j])


def test_unview_rows_restatement_follows_the_box_rule():
    rng = np.random.default_rng(0)
    pred = rng.uniform(0, 33, (6, 7, 7)).astype(np.float32)
    views = (6, 0, 3)
    out = vr.unview_rows(pred, views, 33)
    for i in range(6):
        for r in range(7):
            assert tuple(out[i, r, :4]) == vr.unview_box(views[i % 3], *pred[i, r, :4], 33)
    assert np.array_equal(out[..., 4:], pred[..., 4:])
    assert out.dtype == np.float32


def test_vote_restatement_on_a_hand_case():
    N = 2
    pred = np.zeros((1, 3 * N, 7), np.float32)
    pred[0, :, :4] = [1000, 1000, 1010, 1010]            # far away
    pred[0, :, 4] = 0.9
    pred[0, :, 5:] = [0.1, 0.8]                          # class 1
    pred[0, 1, :4] = [10, 10, 30, 30]                    # view 0
    pred[0, 4, :4] = [11, 10, 31, 30]                    # view 2
    rows = np.zeros((1, 4, 7), np.float32)
    rows[0, 0] = [10, 10, 30, 30, 0.9, 0.8, 1]
    rows[0, 1] = [10, 10, 30, 30, 0.9, 0.8, 0]           # another class: no votes
    rows[0, 2] = [10, 10, 30, 30, 0.9, 0.8, 1]           # behind count
    votes = vr.view_votes(pred, 3, 0.5, 0.4, rows, [2])
    assert votes.tolist() == [[0b101, 0, 0, 0]]
    assert vr.popcount(votes).tolist() == [[2, 0, 0, 0]]
    r2, k2, c2 = vr.view_select(rows, np.arange(4, dtype=np.int32)[None], [2], votes, 2)
    assert c2.tolist() == [1] and k2[0, 0] == 0 and np.array_equal(r2[0, 0], rows[0, 0])
    _, _, c3 = vr.view_select(rows, None, [9], votes, 2)   # count > max_det is preserved
    assert c3.tolist() == [9]


# ---- views.check_views and the argument checks of the product path -------------------------------------------------------------
def test_check_views():
    assert ALL_VIEWS == tuple(range(8)) and FLIPS == (0, 1, 2, 3)
    assert check_views([6, 0, 3]) == (6, 0, 3) and check_views(np.array([1, 2])) == (1, 2) and check_views(ALL_VIEWS) == ALL_VIEWS
    for bad in ((), [], (0, 0), (1, 2, 1), (8,), (-1,), (0, 9), None, 3, (0.5,), ("0",), (True,)):
        with pytest.raises(ValueError):
            check_views(bad)


def test_bad_view_arguments_raise_value_error_before_any_device_use():
    """ValueError, not AyError('no HIP device') and not an AttributeError on the model: the checks come first"""
    r = np.zeros((64, 64, 3), np.uint8)
    for kw in (dict(views=()), dict(views=(0, 0)), dict(views=(8,)), dict(views=(0, -1)),
               dict(min_views=2), dict(min_views=0), dict(views=(0, 1), min_views=3), dict(views=FLIPS, min_views=1.5),
               dict(views=FLIPS, min_views=2, vote_thres=-0.1), dict(views=FLIPS, vote_thres=1.5), dict(views=FLIPS, vote_thres=float("nan")),
               dict(views=(0, 1), overlap=8, min_views=3), dict(views=(3, 3), overlap=8)):
        with pytest.raises(ValueError):
            detect_region(None, r, tile=32, img_size=32, **kw)
    for bad in ((), (0, 0), (8,), (1, -1)):
        with pytest.raises(ValueError):
            RegionTileStream(r, 32, 32, views=bad)


# ---- header, binding, library ---------------------------------------------------------------------------------------------------
def test_header_binding_and_library_have_the_four_symbols():
    text = open(os.path.join(REPO, "include", "amyloid_yolo.h")).read()
    assert re.search(r"#define AY_ABI_VERSION 2\b", text) and _lib.ABI_VERSION == 2
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = _lib.lib()
    assert L.ay_version() == 2
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, code), name
        assert name in _lib._SIGS and name in _lib.exported_symbols()
        assert getattr(L, name).argtypes == _lib._SIGS[name][1]
    assert "THE VIEW RULE" in text and "THE VOTE RULE" in text


def test_entry_points_refuse_bad_arguments_on_the_host():
    """host-side checks, no GPU: null pointers, a repeated id, an id out of range, n_views of 0 and 9"""
    L = _lib.lib()
    p = C.c_void_p(0x1000)
    ids = lambda *v: (C.c_int * max(len(v), 1))(*v)
    ok = ids(0, 5)

    def ingest(region=p, origins=p, views=ok, nv=2, out=p, S=32):
        return L.ay_ingest_region_tiles_views_u8(region, 64, 64, 192, 1, 32, origins, 1, views, nv, S, out, None)

    def unview(pred=p, views=ok, nv=2):
        return L.ay_unview_rows(pred, 2, views, nv, 10, 1, 32, None)

    def votes(pred=p, nv=2, rows=p, count=p, out=p):
        return L.ay_view_votes(pred, 1, nv, 10, 1, C.c_float(0.5), C.c_float(0.4), rows, count, 16, out, None)

    def select(rows=p, count=p, v=p, min_views=1):
        return L.ay_view_select(rows, None, count, v, 1, 16, min_views, None)

    bad = [ingest(region=None), ingest(origins=None), ingest(out=None), ingest(views=None),
           ingest(views=ids(3, 3)), ingest(views=ids(0, 8)), ingest(views=ids(-1, 0)), ingest(nv=0), ingest(views=ids(*range(9)), nv=9),
           ingest(S=0),
           unview(pred=None), unview(views=None), unview(views=ids(3, 3)), unview(views=ids(0, 8)), unview(nv=0),
           unview(views=ids(*range(9)), nv=9),
           votes(pred=None), votes(rows=None), votes(count=None), votes(out=None), votes(nv=0), votes(nv=9),
           select(rows=None), select(count=None), select(v=None), select(min_views=0), select(min_views=9)]
    assert bad == [-1] * len(bad)
    assert ingest(views=ids(3, 3)) == -1 and b"distinct" in L.ay_last_error()


def test_view_kernels_use_no_scratch(tmp_path):
    """hipcc's resource remarks: every kernel of csrc/ay_views.hip has ScratchSize 0"""
    p = subprocess.run([build._hipcc()] + build.FLAGS + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                                         os.path.join(build.CSRC, "ay_views.hip"), "-o", str(tmp_path / "ay_views.o")],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    found, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            found[name] = int(m.group(1))
    assert sum("region_tiles_views_u8_kernel" in n for n in found) == 2
    for k in ("unview_rows_kernel", "view_votes_kernel", "view_select_kernel", "zero_i32_kernel"):
        assert any(k in n for n in found), (k, found)
    assert all(v == 0 for v in found.values()), found
