"""The union-merge (`ay_merge_detections`, csrc/ay_merge.hip) on the CPU with counters, and the inputs that reach what random float
corners never do (TEST INFRASTRUCTURE ONLY -- never imported by the product).

The specification stays `oracle.boxes_oracle.merge_detections_ordered`: the function that tests/golden/merge_cases.npz pins to the
reference's own outputs.  `ordered_counted` restates it with counters so that a test can SHOW that a case walks the branch it was built
for (a merged row that is already in the set, a merged row whose value was removed earlier, a live row skipped for its value);
tests/test_merge_cpu.py holds the restatement to the oracle's rows on every case.  `floor_variant` is the same walk with `math.floor`
for `int()`: it exists only to prove that a case tells the two rules apart.

Rows are (x1, y1, x2, y2, conf, cls_conf, cls_pred) float32.  Every builder is cached: the walk is pure Python and a 1024-row image
costs seconds, so it runs once per process (the arrays that come back are read-only)."""
import functools
import math

import numpy as np

from oracle import boxes_oracle as bo

MAX_ROWS = 1024


def _walk(det, trunc):
    rows, seen = [], set()
    st = dict(dups=0, merges=0, passes=0, present=0, present_flagged=0, flagged=0, value_skips=0, rows_ever=0, present_rows=[], merged_pairs=[])
    for r in np.asarray(det, np.float32).reshape(-1, 7).tolist():
        t = tuple(r)
        if t in seen:
            st["dups"] += 1
            continue
        seen.add(t)
        rows.append(t)
    st["rows_ever"] = len(rows)
    live = [True] * len(rows)
    removed = set()
    while True:
        st["passes"] += 1
        changed = False
        limit = len(rows)
        for i in range(limit):
            for j in range(i + 1, limit):
                ei, ej = rows[i], rows[j]
                if not live[i] or not live[j]:
                    continue
                if not ((ei[6] == 1 == ej[6]) or (ei[6] == 0 == ej[6])):
                    continue
                if ei in removed or ej in removed:
                    st["value_skips"] += 1
                    continue
                xi, yi, wi, hi = trunc(ei[0]), trunc(ei[1]), trunc(ei[2] - ei[0]), trunc(ei[3] - ei[1])
                xj, yj, wj, hj = trunc(ej[0]), trunc(ej[1]), trunc(ej[2] - ej[0]), trunc(ej[3] - ej[1])
                if wi <= 0 or hi <= 0 or wj <= 0 or hj <= 0:
                    continue
                if min(xi + wi, xj + wj) <= max(xi, xj) or min(yi + hi, yj + hj) <= max(yi, yj):
                    continue
                left, top = min(xi, xj), min(yi, yj)
                right, bottom = max(xi + wi, xj + wj) - 1, max(yi + hi, yj + hj) - 1
                new = (left, top, right, bottom, min(ei[4], ej[4]), min(ei[5], ej[5]), ei[6])
                if any(live[k] and rows[k] == new for k in range(len(rows))):
                    st["present"] += 1
                    st["present_flagged"] += new in removed
                    st["present_rows"].append(i)
                    continue
                if new in removed:
                    st["flagged"] += 1
                rows.append(new)
                live.append(True)
                live[i] = live[j] = False
                removed.add(ei)
                removed.add(ej)
                changed = True
                st["merges"] += 1
                st["merged_pairs"].append((i, j))
        if not changed:
            break
    st["rows_ever"] += st["merges"]
    return np.asarray([rows[k] for k in range(len(rows)) if live[k]], np.float64).reshape(-1, 7), st


def ordered_counted(det):
    """`merge_detections_ordered` with counters -> (rows float64 [m,7] in list order, stats).  stats: `dups` input rows collapsed by
    set(); `merges`; `passes` (the last, idle one included); `present` pairs skipped because their merged row is live by value;
    `present_flagged` those of them whose live twin is itself flagged; `flagged` merged rows appended whose value is in `removed`
    (they never merge again); `value_skips` pairs of live same-class rows skipped because one's value is in `removed`;
    `rows_ever` distinct inputs + merges (the table the kernel needs);
    `present_rows` the i of every `present` skip and `merged_pairs` the (i, j) of every merge, as list indices after set()."""
    return _walk(det, int)


def floor_variant(det):
    """the same walk with floor for int(): NOT the rule -- the two differ for negative fractional corners"""
    return _walk(det, math.floor)[0]


def want_bits(rows64):
    """the rows a float32 kernel must give, as uint32 [m,7]: every value has to be a float32 exactly (the input is left as it is)"""
    rows64 = np.asarray(rows64, np.float64).reshape(-1, 7)
    f32 = rows64.astype(np.float32)
    assert np.array_equal(f32.astype(np.float64), rows64) and np.array_equal(np.signbit(f32), np.signbit(rows64))
    return f32.view(np.uint32).copy()


def row_set(rows):
    return set(map(tuple, np.asarray(rows, np.float64).reshape(-1, 7).tolist()))


_expected = {}


def expected(det):
    """the oracle's rows for `det` as (uint32 bits [m,7], float64 rows), once per distinct input and process"""
    det = np.ascontiguousarray(det, np.float32).reshape(-1, 7)
    key = det.tobytes()
    if key not in _expected:
        rows = bo.merge_detections_ordered(det)
        bits = want_bits(rows)
        rows.setflags(write=False)
        bits.setflags(write=False)
        _expected[key] = (bits, rows)
    return _expected[key]


def _frozen(a):
    a = np.ascontiguousarray(a, np.float32)
    a.setflags(write=False)
    return a


# ---- 1. lattice: integer corners on a small square, so that merged rectangles coincide with rows that exist or existed ------------------
# name -> (n, side of the square, lowest corner, labels, PCG64 seed, largest box side).  Image d was searched for (one seed in some
# hundreds has it): a pair whose merged row equals a LIVE row whose value is also in `removed` (state 1 | 16 in the kernel) -- the
# only input on which "is this row in the set" must look past the flag.
LATTICE = {"a": (200, 24, -12, (0, 1, 2), 2, 5), "b": (MAX_ROWS, 64, -32, (0, 1), 3, 5), "c": (MAX_ROWS, 40, 0, (0, 1), 4, 5),
           "d": (150, 12, -6, (1,), 61, 3)}


@functools.lru_cache(maxsize=None)
def lattice(name):
    n, side, low, labels, seed, longest = LATTICE[name]
    rng = np.random.Generator(np.random.PCG64(seed))
    xy = rng.integers(low, low + side, (n, 2))
    wh = rng.integers(0, longest + 1, (n, 2))
    conf = rng.choice([0.5, 0.75], (n, 2))
    lab = rng.choice(labels, (n, 1))
    return _frozen(np.concatenate([xy, xy + wh, conf, lab], 1))


# ---- 2. capacity: n nested boxes merge n - 1 times, the table holds 2n - 1 rows ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def capacity(n=MAX_ROWS):
    i = np.arange(n, dtype=np.float64)
    c = 0.5 + i / 4096
    return _frozen(np.stack([3000 - 3 * i, 3000 - 3 * i, 3002 + 3 * i, 3002 + 3 * i, c, c, np.ones(n)], 1))


# ---- 3. search strides: a grid of disjoint boxes with partners planted at chosen distances -----------------------------------------------
def grid(n=MAX_ROWS, label=0.0):
    """n disjoint 3 x 3 px boxes, 10 px apart, 32 to a line, confidences distinct and rising with the index"""
    k = np.arange(n)
    x, y = 10.0 * (k % 32), 10.0 * (k // 32)
    c = 0.5 + k / 4096
    return np.stack([x, y, x + 3, y + 3, c, c - 0.25, np.full(n, label)], 1).astype(np.float32)


def _plant(det, i, j, shift):
    det[j, :4] = det[i, :4] + shift


STRIDE_DISTANCES = (1, 63, 64, 65, 128, 1023)
STRIDE_STARTS = (0, 1, 63, 64)


@functools.lru_cache(maxsize=None)
def stride_plan():
    """every (i, i + d) that fits into 1024 rows, dealt into images so that no row is used twice: a tuple of tuples of pairs"""
    images = []
    for d in STRIDE_DISTANCES:
        for i in STRIDE_STARTS:
            if i + d >= MAX_ROWS:
                continue
            for img in images:
                if not ({i, i + d} & {r for p in img for r in p}):
                    img.append((i, i + d))
                    break
            else:
                images.append([(i, i + d)])
    return tuple(tuple(img) for img in images)


STRIDES_WIDE = 3                                      # the image of the plan that holds the pair (0, 1023)


@functools.lru_cache(maxsize=None)
def strides(k):
    """image k of the plan: row j is its mate i moved by (2, 2): the two share one pixel, the merged box is 5 px wide.  Only the
    image with the pair (0, 1023) needs 1024 rows; the others hold 256 (three strides behind the furthest partner's mate)"""
    det = grid(MAX_ROWS if any(j >= 256 for _, j in stride_plan()[k]) else 256)
    for i, j in stride_plan()[k]:
        _plant(det, i, j, 2)
    return _frozen(det)


PRESENT_THEN_MERGE = ((0, 1, 65), (63, 64, 128))      # (i, first partner, second partner >= 64 rows further on)


@functools.lru_cache(maxsize=None)
def strides_present():
    """row i's first partner sits at mate + (1, 1): their merged box IS the mate (one pixel short of the union, the mate's lower
    confidences), so the pair is skipped as present; the second partner, a stride or more further on, merges"""
    det = grid(256)
    for i, j1, j2 in PRESENT_THEN_MERGE:
        _plant(det, i, j1, 1)
        _plant(det, i, j2, 2)
    return _frozen(det)


# ---- 4. duplicates -----------------------------------------------------------------------------------------------------------------------
DUP_AT = (63, 64, 65, 127, 128, 199)


@functools.lru_cache(maxsize=None)
def dups_strides():
    """copies of row 0 on both sides of the 64-lane strides of the set() prologue and in the last row; row 5 merges with row 0,
    so a copy that survived would show as a second merge"""
    det = grid(200)
    _plant(det, 0, 5, 2)
    for k in DUP_AT:
        det[k] = det[0]
    return _frozen(det), len(DUP_AT)


@functools.lru_cache(maxsize=None)
def dups_small():
    """three equal rows; (-0.0, +0.0) and (+0.0, -0.0) in x1, equal as values: the first one's bits survive; seven rows that differ
    from row 0 in one column each: none collapses"""
    a = [100, 100, 130, 140, 0.75, 0.5, 0]
    rows = [a, a, a, [-0.0, 300, 9, 309, 0.75, 0.5, 2], [0.0, 300, 9, 309, 0.75, 0.5, 2], [0.0, 400, 9, 409, 0.75, 0.5, 2],
            [-0.0, 400, 9, 409, 0.75, 0.5, 2]]
    for c, v in enumerate((101, 101, 131, 141, 0.625, 0.625, 1)):
        r = list(a)
        r[c] = v
        rows.append(r)
    return _frozen(rows), 4


# ---- 5. truncation: int() is toward zero, floor is not ------------------------------------------------------------------------------------
OFFSETS = (0.0, 0.5, 0.75)


@functools.lru_cache(maxsize=None)
def truncation(seed=5, n=300):
    rng = np.random.Generator(np.random.PCG64(seed))
    xy = rng.integers(-24, 24, (n, 2)) + rng.choice(OFFSETS, (n, 2))
    wh = rng.integers(0, 5, (n, 2)) + rng.choice(OFFSETS, (n, 2))
    det = np.concatenate([xy, xy + wh, rng.choice([0.5, 0.625, 0.75], (n, 2)), rng.choice([0, 1, 2], (n, 1))], 1)
    det[7, 2] = det[7, 0] - 1.5             # x2 < x1: a negative width never overlaps
    det[150, 2] = det[150, 0] - 0.5
    det[7, 6] = det[150, 6] = 1
    return _frozen(det)


@functools.lru_cache(maxsize=None)
def truncation_pairs(seed=6):
    """the pair-only twin: 16 x 16 cells of 16 px around the origin, each with one box or two that (mostly) overlap, corners of the
    same kind; no cluster has more than two rows, so the result does not depend on the order of a set.  The last pair lies at
    100 000 px (slide coordinates: float32 still holds quarters there)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rows = []
    for cell in range(256):
        org = np.array([16.0 * (cell % 16 - 8), 16.0 * (cell // 16 - 8)])
        lab = float(rng.integers(0, 2))
        xy = org + rng.integers(0, 4, 2) + rng.choice(OFFSETS, 2)
        wh = rng.integers(0, 5, 2) + rng.choice(OFFSETS, 2)
        rows.append([*xy, *(xy + wh), *rng.choice([0.5, 0.625, 0.75], 2), lab])
        if rng.integers(0, 3):
            xy = xy + rng.integers(0, 3, 2) + rng.choice(OFFSETS, 2)
            wh = rng.integers(0, 5, 2) + rng.choice(OFFSETS, 2)
            rows.append([*xy, *(xy + wh), *rng.choice([0.5, 0.625, 0.75], 2), lab])
    rows.append([100000.5, 100000.25, 100040.5, 100030.75, 0.75, 0.5, 1])
    rows.append([100020.75, 100010.5, 100060.25, 100050.5, 0.5, 0.75, 1])
    return _frozen(rows)


# ---- 6. labels ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def labels():
    """overlapping pairs, 100 px apart: labels 2, -1, 0.5, 3 stay; (-0.0, 0.0) and (0.0, -0.0) merge and keep the label bits of the
    lower-index row; 0 over 1 on the same pixels stays; a pair of 1s merges"""
    rows = []
    for k, (la, lb) in enumerate([(2, 2), (-1, -1), (0.5, 0.5), (3, 3), (-0.0, 0.0), (0.0, -0.0), (0, 1), (1, 1)]):
        x = 100.0 * k - 300
        rows.append([x, 10, x + 20, 30, 0.75, 0.5, la])
        rows.append([x + 5, 15, x + 25, 35, 0.5, 0.75, lb])
    return _frozen(rows)


# ---- 7. counts and strides ----------------------------------------------------------------------------------------------------------------
def filler(m):
    """m overlapping, distinct class-1 boxes over everything: what lies behind count[b] (a kernel that read them would merge them)"""
    k = np.arange(m, dtype=np.float64)
    return np.stack([-100 - k, -100 - k, 200 + k, 5000 + k, np.full(m, 0.875), np.full(m, 0.875), np.ones(m)], 1).astype(np.float32)


COUNT_MAX_ROWS = (1, 7, 64, 65, 1000, 1024)


@functools.lru_cache(maxsize=None)
def count_batch(max_rows):
    """-> (rows float32 [6, max_rows, 7], count int32 [6], valid [6]): one image per count rule, every image from another source
    (so that a wrong image stride reads a neighbour's rows), `filler` behind count[b].  At 1000 and 1024 rows the full images are
    the 1024-row cases above (cut), so that no further large image is built."""
    wide = strides(STRIDES_WIDE)
    sources = [wide, lattice("b"), wide] if max_rows == 1000 else \
              [lattice("b"), lattice("c"), wide] if max_rows == MAX_ROWS else [lattice("a"), truncation(), strides_present()]
    sources += [truncation()[::-1], lattice("a"), lattice("a")[50:]]
    counts = [max_rows, max_rows + 5, 1 << 30, 1, 0, -3]
    rows = np.empty((6, max_rows, 7), np.float32)
    valid = [min(max(c, 0), max_rows) for c in counts]
    for b, (src, v) in enumerate(zip(sources, valid)):
        rows[b, :v] = src[:v]
        rows[b, v:] = filler(max_rows - v)
    rows.setflags(write=False)
    return rows, np.asarray(counts, np.int32), valid


# ---- the registry, and the inputs of the one older GPU test ----------------------------------------------------------------------------------
def cases():
    """name -> builder of every image above, in a fixed order (nothing is built until it is called)"""
    out = {f"lattice_{k}": functools.partial(lattice, k) for k in LATTICE}
    out["capacity"] = capacity
    for k in range(len(stride_plan())):
        out[f"strides{k}"] = functools.partial(strides, k)
    out["strides_present"] = strides_present
    out["dups_strides"] = lambda: dups_strides()[0]
    out["dups_small"] = lambda: dups_small()[0]
    out["truncation"] = truncation
    out["truncation_pairs"] = truncation_pairs
    out["labels"] = labels
    return out


LARGE = ("lattice_b", "lattice_c", "capacity", f"strides{STRIDES_WIDE}")        # the 1024-row images: seconds each on the CPU
PAIR_ONLY = tuple(f"strides{k}" for k in range(len(stride_plan()))) + ("truncation_pairs",)      # no cluster of more than two rows


def parity_inputs():
    """the inputs of tests/test_gpu_parity.py::test_merge_detections_device, restated: the fixtures and its four cluster batches"""
    import golden_cases as gc
    out = dict(gc.merge_inputs())
    rng = np.random.Generator(np.random.PCG64(123))
    for k, (n, ncl, spread) in enumerate([(300, 12, 60.0), (1024, 40, 25.0), (64, 3, 5.0), (0, 1, 1.0)]):
        centers = rng.uniform(50, 1450, (ncl, 2))
        xy = centers[rng.integers(0, ncl, n)] + rng.normal(0, spread, (n, 2))
        wh = rng.uniform(6, 90, (n, 2))
        det = np.concatenate([xy, xy + wh, rng.uniform(0.5, 1, (n, 2)), rng.integers(0, 3, (n, 1))], 1).astype(np.float32)
        if n >= 64:
            det[5] = det[2]
            det[40] = det[2]
        out[f"clusters{k}"] = det
    return out
