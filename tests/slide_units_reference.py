"""The launch geometry of the slide-level passes restated from their sources, and the inputs of tests/test_gpu_slide_units.py (TEST
INFRASTRUCTURE ONLY).  Every capped launch lets a workgroup (a wavefront, a group of 16 lanes) loop over the work that is left; the
functions here say how many units a launch has, how many workgroups take them and how many trips each makes, so that a test can assert
that its input reaches the second trip before it compares anything.  A later change of a cap or a unit size then fails the test's
geometry assertion: it cannot silently stop covering the case.

Nothing here comes from the product: the constants are restated (csrc/ay_slide_pass.h, ay_stain.hip, ay_load.hip, ay_focus.hip,
ay_tissue.hip, ay_segment.hip, ay_spatial.hip, ay_cut.h, ay_ingest.hip, ay_views.hip), the contents are NumPy's."""
import functools

import numpy as np

import load_reference as lr
import segment_reference as sg
import spatial_reference as sp

F32 = np.float32
ITEM = 48                                         # bytes of an item of the read stream
CAP = 256 * 8                                     # workgroups of a slide pass (slide_units)
HIST, LOAD, FOCUS = (16, 2048), (16, 256), (32, 32)      # (BAND rows, XQ items) of a work unit: hist and basis, load, focus
HIST_FLUSH = 2048                                 # units of one workgroup between two flushes of its LDS histogram
TISSUE_CAP, TISSUE_BAND = 256 * 32, 32            # ay_tile_tissue_u8
BOX_WAVES = 4                                     # box_walk: one wavefront per box, four per workgroup
BOX_CAP = BOX_WAVES * CAP                         # boxes in flight
SEG_CAP = CAP                                     # box_segments_kernel: one workgroup per row
PAIR_GROUP, PAIR_BLOCKS = 16, 2048                # pair_search_kernel: 16 lanes per centre, 16 centres per workgroup
PAIR_CAP = (256 // PAIR_GROUP) * PAIR_BLOCKS      # centres in flight
ELEMENT_CAP = 256 * 32 * 256                      # threads of the element loops (apply, cut, ingest, unview)
BG = sg.BG


def cdiv(a, b):
    return -(-a // b)


def trips(units, blocks):
    """units dealt round to `blocks` takers (u = b, b + blocks, ..) -> (the smallest, the largest) number of trips of a taker"""
    return units // blocks, cdiv(units, blocks)


def slide_units(W, shrink, rows, BAND, XQ):
    """-> (nq, n_xc, units, blocks): items of a row, units across a row, units, workgroups (slide_units of ay_slide_pass.h; W and rows
    of the (halved) image)"""
    nq = cdiv(W * 3 * shrink, ITEM)
    n_xc = cdiv(nq, XQ)
    units = cdiv(rows, BAND) * n_xc
    return nq, n_xc, units, min(units, CAP)


def focus_units(W, shrink, H):
    """the focus pass of one call that owns every row: the centre rows are 1 .. H - 2"""
    return slide_units(W, shrink, H - 2, *FOCUS)


def unit_wq(u, n_xc, nq, XQ):
    """items across unit u"""
    return min(XQ, nq - (u % n_xc) * XQ)


def tissue_units(H, W, tile, step):
    """-> (m, n_yint, n_bands, n_xint, units, blocks) of ay_tile_tissue_u8 on an H x W (halved) image"""
    m = 2 if tile % step else 1
    n_yint, n_xint, n_bands = cdiv(H, step) * m, cdiv(W, step) * m, cdiv(step, TISSUE_BAND)
    units = n_yint * n_bands * n_xint
    return m, n_yint, n_bands, n_xint, units, min(units, TISSUE_CAP)


def box_walk_waves(M):
    return min(cdiv(M, BOX_WAVES), CAP) * BOX_WAVES


def segment_blocks(M):
    return min(M, SEG_CAP)


def pair_groups(M):
    """groups of 16 lanes of the search launch of a call with M rows"""
    return min(max(cdiv(M * PAIR_GROUP, 256), 1), PAIR_BLOCKS) * (256 // PAIR_GROUP)


def element_threads(total):
    return min(cdiv(total, 256), 256 * 32) * 256


# ---- contents ------------------------------------------------------------------------------------------------------------------------
def content(H, W, seed):
    """uint8 [H, W, 3] in 2 x 2 blocks of one kind each (so that the halved image holds the same kinds): random bytes, glass of 225 ..
    255, and segment_reference's POSITIVE, CORE and NEGATIVE colours.  Independent draws: no vertical period."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(5, size=(cdiv(H, 2), cdiv(W, 2)), p=[0.40, 0.25, 0.15, 0.10, 0.10]).astype(np.uint8)
    kind = np.repeat(np.repeat(kind, 2, 0), 2, 1)[:H, :W]
    r = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
    glass = rng.integers(225, 256, size=(H, W, 3), dtype=np.uint8)
    r[kind == 1] = glass[kind == 1]
    for k, colour in ((2, sg.POSITIVE), (3, sg.CORE), (4, sg.NEGATIVE)):
        r[kind == k] = colour
    r.setflags(write=False)
    return r


def source_shape(H, W, shrink):
    """the source raster of an H x W (halved) image: odd sides for shrink 2, whose last row and column belong to no pixel"""
    return (H, W) if shrink == 1 else (2 * H + 1, 2 * W + 1)


STRIP_W, STRIP_H = 37, 16 * (2 * CAP + 300) - 5               # 70 331 rows: 4 396 units of 16 rows, 2 or 3 per workgroup
FOCUS_A = (40, 32 * (2 * CAP + 300) - 5, 48)                  # W, H, cell: 4 396 units, n_xc = 1
FOCUS_B = (520, 32 * 1030 + 7, 64)                            # n_xc = 2 (32 items, 1 item); 2 062 units
FOCUS_C = (1030, 32 * 690 + 9, 64)                            # n_xc = 3 (32, 32, 1 items): 2048 % 3 != 0, so wq changes between trips
FLUSH_H = 16 * (HIST_FLUSH * CAP + CAP + 9)                   # 67 141 776 rows of one pixel
FLUSH_PERIOD = 4099                                           # rows of the repeated block: a prime, so it divides no 16 * 2048 * k
TISSUE_CASES = ((1000, 24, 16), (1460, 16, 16))               # side, tile, step
BOX_HW, BOX_M = (300, 400), 2 * BOX_CAP + 77
APPLY_SIDE = 1500


@functools.lru_cache(maxsize=None)
def strip_raster(shrink):
    return content(*source_shape(STRIP_H, STRIP_W, shrink), 100 + shrink)


@functools.lru_cache(maxsize=None)
def focus_raster(case, shrink):
    W, H, _ = {"a": FOCUS_A, "b": FOCUS_B, "c": FOCUS_C}[case]
    return content(*source_shape(H, W, shrink), 200 + 10 * "abc".index(case) + shrink)


@functools.lru_cache(maxsize=None)
def flush_column():
    """-> (column uint8 [FLUSH_H, 1, 3], block [FLUSH_PERIOD, 1, 3], repeats, rows of the remainder): the block tiled down the column"""
    block = content(FLUSH_PERIOD, 1, 300)
    reps, rem = divmod(FLUSH_H, FLUSH_PERIOD)
    col = np.concatenate([np.tile(block, (reps, 1, 1)), block[:rem]])       # (left writable, so that torch takes it without a copy)
    return col, block, reps, rem


@functools.lru_cache(maxsize=None)
def tissue_raster(side, shrink):
    return content(*source_shape(side, side, shrink), 400 + side % 7 + shrink)


@functools.lru_cache(maxsize=None)
def box_case():
    """-> (raster 300 x 400, rows [2 * 8192 + 77, 7], k): random boxes; rows k, k + 8192 and k + 16384, the three boxes of one
    wavefront, are a NaN row, an empty row and a row off the slide"""
    H, W = BOX_HW
    rows = lr.random_boxes(BOX_M, H, W, 500, cuts=(13, 14))
    k = 40
    rows[k, :4] = (float("nan"), 10.0, 30.0, 40.0)
    rows[k + BOX_CAP, :4] = (50.0, 60.0, 50.0, 90.0)
    rows[k + 2 * BOX_CAP, :4] = (W + 5.0, 20.0, W + 40.0, 60.0)
    rows[k + 1, :4] = (30.0, 40.0, 20.0, 50.0)                       # an inverted row first, then two ordinary boxes
    rows.setflags(write=False)
    return content(H, W, 501), rows, k


# ---- the segmenter's rows --------------------------------------------------------------------------------------------------------------
SEG_H, SEG_W, SEG_BLANK_X, SEG_SHORT, SEG_MARGIN, SEG_M = 300, 520, 300, 280, 8, 2 * SEG_CAP + 37
SEG_BIG_EACH = 12                                 # workgroups per succession that holds a window above 96 (what the reference's time allows)


@functools.lru_cache(maxsize=None)
def segment_raster():
    """segment_reference.blob_raster on 300 x 520 with everything right of column 300 repainted without a positive pixel (NEGATIVE, some
    glass): a window there holds none"""
    r, _ = sg.blob_raster(SEG_H, SEG_W, 60, 1, radius=6)
    r = r.copy()
    r[:, SEG_BLANK_X:] = sg.NEGATIVE
    glass = np.zeros((SEG_H, SEG_W), bool)
    glass[:, SEG_BLANK_X:] = np.random.default_rng(61).random((SEG_H, SEG_W - SEG_BLANK_X)) < 0.1
    r[glass] = sg.GLASS
    r.setflags(write=False)
    return r


def _blob_centres(pos, n, rng, half=10):
    """n pixels whose (2 half + 1)^2 neighbourhood is almost all positive: the inside of a sizeable blob"""
    c = np.pad(pos, half).astype(np.int64).cumsum(0).cumsum(1)
    c = np.pad(c, ((1, 0), (1, 0)))
    s = 2 * half + 1
    full = c[s:, s:] - c[:-s, s:] - c[s:, :-s] + c[:-s, :-s]
    ys, xs = np.nonzero(full[:, :SEG_BLANK_X - 20] >= 0.8 * s * s)
    pick = rng.integers(0, len(ys), n)
    return xs[pick].astype(np.float64), ys[pick].astype(np.float64)


def _boxes(cx, cy, w, h):
    out = np.zeros((len(cx), 7), F32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2
    out[:, 4:6] = 0.9
    return out


@functools.lru_cache(maxsize=None)
def segment_rows():
    """rows [2 * 2048 + 37, 7] on segment_raster(), ordered so that the boxes m, m + 2048 (and m + 4096) of one workgroup follow each
    other as the successions named in SUCCESSIONS; test_slide_units_cpu.py counts them on the reference's output"""
    import stain_reference as sref
    rng = np.random.default_rng(62)
    r = segment_raster()
    t, q = lr.classes(r, 1, sg.BG, sref.tables(), 1)
    pos = t & (q >= sg.THRES_BIN)
    u = lambda lo, hi, n: rng.uniform(lo, hi, n)

    def small(n):                                 # windows of at most 36 + 16 pixels a side, anywhere left of the blank part
        return _boxes(u(20, SEG_BLANK_X - 20, n), u(20, SEG_SHORT - 50, n), u(4, 36, n), u(4, 36, n))

    def big(n):                                   # windows of 116 .. 176 pixels a side
        return _boxes(u(100, SEG_BLANK_X - 90, n), u(100, SEG_SHORT - 110, n), u(100, 160, n), u(100, 160, n))

    def small_blob(n):
        return _boxes(*_blob_centres(pos, n, rng), u(24, 44, n), u(24, 44, n))

    def big_blob(n):
        cx, cy = _blob_centres(pos, n, rng)
        return _boxes(np.clip(cx, 100, SEG_BLANK_X - 90), np.clip(cy, 100, SEG_SHORT - 110), u(100, 160, n), u(100, 160, n))

    def small_blank(n):
        return _boxes(u(SEG_BLANK_X + 60, SEG_W - 60, n), u(60, SEG_SHORT - 70, n), u(4, 56, n), u(4, 56, n))

    def big_blank(n):
        return _boxes(u(SEG_BLANK_X + 110, SEG_W - 110, n), u(110, SEG_SHORT - 120, n), u(100, 160, n), u(100, 160, n))

    def small_wide(n):
        return _boxes(u(60, SEG_BLANK_X - 60, n), u(60, SEG_SHORT - 80, n), u(66, 78, n), u(66, 78, n))

    def small_narrow(n):                          # fewer words a row (at most 31 + 16 pixels) and fewer rows than small_wide
        return _boxes(u(30, SEG_BLANK_X - 30, n), u(30, SEG_SHORT - 50, n), u(3, 12, n), u(3, 30, n))

    def big_wide(n):
        return _boxes(u(130, SEG_BLANK_X - 120, n), u(125, SEG_SHORT - 130, n), u(200, 230, n), u(200, 230, n))

    def big_narrow(n):                            # above 96 by its height alone
        return _boxes(u(30, SEG_BLANK_X - 30, n), u(80, SEG_SHORT - 90, n), u(3, 40, n), u(100, 140, n))

    def nonfinite(n):
        b = small(n)
        b[np.arange(n), rng.integers(0, 4, n)] = np.asarray([np.nan, np.inf, -np.inf], F32)[rng.integers(0, 3, n)]
        return b

    def empty(n):
        b = small(n)
        b[:, 2] = b[:, 0] - rng.integers(0, 2, n) * 3.0            # no column, or inverted
        return b

    def large(n):
        return _boxes(u(150, 350, n), u(130, 170, n), u(245, 400, n), u(20, 60, n))

    def not_resident_small(n):                    # the window reaches below row SEG_SHORT, which the region of the C ABI test lacks
        return _boxes(u(20, SEG_BLANK_X - 20, n), u(SEG_SHORT - 10, SEG_H - 5, n), u(10, 50, n), u(30, 50, n))

    def not_resident_big(n):
        return _boxes(u(100, SEG_BLANK_X - 90, n), u(SEG_SHORT - 60, SEG_SHORT - 40, n), u(100, 160, n), u(130, 170, n))

    with_big = [(big_blob, big_blank, small), (big_wide, big_narrow, empty), (small, big, small), (big, small, nonfinite),
                (big, not_resident_big, small), (big, large, small)]
    small_only = [(small_blob, small_blank, small), (small_wide, small_narrow, small_blob), (small, nonfinite, small), (small, empty, small),
                  (small, large, small), (small, not_resident_small, small)]
    plan = [s for s in with_big for _ in range(SEG_BIG_EACH)]
    plan += [small_only[i % len(small_only)] for i in range(SEG_CAP - len(plan))]
    rows = np.zeros((SEG_M, 7), F32)
    for m, s in enumerate(plan):
        for k in range(3):
            if m + k * SEG_CAP < SEG_M:
                rows[m + k * SEG_CAP] = s[k](1)[0]
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def segment_want():
    """the reference on segment_rows(), computed once -> (out, flags) of ONE call on the rows [0, SEG_SHORT) of the slide that owns every
    row, and (out, flags) on the whole slide (any strip plan gives that): the two differ in the NOT_RESIDENT rows of the first"""
    import stain_reference as sref
    r, rows = segment_raster(), segment_rows()
    args = (1, sg.BG, sref.tables(), 1, sg.THRES_BIN, sg.CORE_BIN, SEG_MARGIN, 1)
    short, short_flags = sg.segment(r, *args, rows, plan=[(0, SEG_SHORT, 0, SEG_H)])
    away = np.flatnonzero(short[:, 0] == sg.NOT_RESIDENT)
    whole = short.copy()
    whole[away], _ = sg.segment(r, *args, rows[away])
    for a in (short, whole):
        a.setflags(write=False)
    return short, int(short_flags[0]), whole, int(np.bitwise_or.reduce(whole[:, 0]))


def segment_successions(out):
    """the reference's rows [M, 20] of ONE call -> {name: count}: how often a workgroup's consecutive boxes (m, m + 2048) follow each
    other in the named way.  Both of a pair pass through the same kernel instance where the name says "same instance": the instance
    of a window is that of its larger side (<= 96, above), that of a row without a window the first."""
    out = np.asarray(out)
    a, b = out[:-SEG_CAP], out[SEG_CAP:]                            # a workgroup's box and its next
    side = lambda o: np.maximum(o[:, 3], o[:, 4])
    window = lambda o: (o[:, 0] == 0) | (o[:, 0] == sg.NOT_RESIDENT)
    labelled = lambda o: o[:, 0] == 0
    small = lambda o: window(o) & (side(o) <= 96)
    bigw = lambda o: window(o) & (side(o) > 96)
    counts = {"large component, then no positive pixel (<= 96, same instance)":
                  (labelled(a) & (a[:, 7] >= 200) & labelled(b) & (b[:, 5] == 0) & small(a) & small(b)).sum(),
              "large component, then no positive pixel (> 96, same instance)":
                  (labelled(a) & (a[:, 7] >= 200) & labelled(b) & (b[:, 5] == 0) & bigw(a) & bigw(b)).sum(),
              "wide, then narrower and shorter (<= 96, same instance)":
                  (labelled(a) & labelled(b) & small(a) & small(b) & (cdiv(b[:, 3], 32) < cdiv(a[:, 3], 32)) & (b[:, 4] < a[:, 4]) & (a[:, 5] > 0)
                   & (b[:, 5] > 0)).sum(),
              "wide, then narrower and shorter (> 96, same instance)":
                  (labelled(a) & labelled(b) & bigw(a) & bigw(b) & (cdiv(b[:, 3], 32) < cdiv(a[:, 3], 32)) & (b[:, 4] < a[:, 4]) & (a[:, 5] > 0)
                   & (b[:, 5] > 0)).sum(),
              "<= 96, then > 96": (labelled(a) & labelled(b) & small(a) & bigw(b)).sum(),
              "> 96, then <= 96": (labelled(a) & labelled(b) & bigw(a) & small(b)).sum()}
    for name, status in (("NONFINITE", sg.NONFINITE), ("EMPTY", sg.EMPTY), ("LARGE", sg.LARGE), ("NOT_RESIDENT", sg.NOT_RESIDENT)):
        counts[f"window, then {name}"] = (labelled(a) & (a[:, 5] > 0) & (b[:, 0] == status)).sum()
    counts["NOT_RESIDENT above 96"] = ((out[:, 0] == sg.NOT_RESIDENT) & (side(out) > 96)).sum()
    return {k: int(v) for k, v in counts.items()}


# ---- the pair search's rows ------------------------------------------------------------------------------------------------------------
PAIR_M, PAIR_CLASSES, PAIR_RADII_PX = 71000, 3, (8, 16, 32, 64)


@functools.lru_cache(maxsize=None)
def pair_rows():
    rows = sp.clustered_rows(PAIR_M, 700)
    rows.setflags(write=False)
    return rows
