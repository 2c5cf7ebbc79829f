"""CPU: the inputs of tests/test_gpu_merge.py reach what they were built for, on the reference alone.

tests/merge_reference.py restates `oracle.boxes_oracle.merge_detections_ordered` with counters; here every case is held to the oracle's
rows (so the counters count the oracle's walk), to float32 exactness, and to the condition that makes it a test of the kernel:
merged rows that already sit in the set or sat in it, a full 2n - 1 table, partners in later 64-lane strides, duplicates on stride
boundaries, corners where int() and floor part.  The last test records why the file exists: the inputs of the one older GPU test
(test_gpu_parity.py::test_merge_detections_device) never reach the value-set branches.

Counters measured (present / flagged / value_skips / merges / passes / rows ever):
  lattice_a 5 / 1 / 80 / 48 / 5 / 248;  lattice_b 23 / 1 / 1834 / 414 / 8 / 1438;  lattice_c 12 / 2 / 7544 / 631 / 21 / 1654 (1 duplicate);
  lattice_d 5 / 1 / 281 / 53 / 5 / 200 (3 duplicates; 3 of the 5 present hits meet a live row that is itself flagged: the only such case);
  capacity 0 / 0 / 0 / 1023 / 11 / 2047;  strides_present 2 / 2 / 501 / 4 / 3 / 260;  truncation 0 / 0 / 0 / 22 / 5 / 322."""
import functools

import numpy as np
import pytest
import torch

import merge_reference as mr
from amyloid_yolo_paper_amd.postprocess import merge_detections
from oracle import boxes_oracle as bo

CASES = mr.cases()


@functools.lru_cache(maxsize=None)
def counted(name):
    return mr.ordered_counted(CASES[name]())


def by_cost(names):
    return [pytest.param(n, marks=pytest.mark.slow) if n in mr.LARGE else n for n in names]


@pytest.mark.parametrize("name", by_cost(CASES))
def test_the_restatement_gives_the_oracles_rows_and_they_are_float32(name):
    det = CASES[name]()
    before = det.copy()
    rows, st = counted(name)
    bits, want = mr.expected(det)                                     # the oracle's rows (merge_detections_ordered), walked once
    assert rows.shape == want.shape and np.array_equal(rows, want) and np.array_equal(np.signbit(rows), np.signbit(want))
    assert np.array_equal(bits, mr.want_bits(want))
    assert bits.dtype == np.uint32 and bits.shape == want.shape and np.array_equal(bits.view(np.float32).astype(np.float64), want)
    assert np.array_equal(det, before) and np.isfinite(det).all() and len(det) <= mr.MAX_ROWS
    assert st["rows_ever"] == len(det) - st["dups"] + st["merges"] <= 2 * len(det) - 1
    print(name, {k: v for k, v in st.items() if not isinstance(v, list)})


def test_want_bits_refuses_what_float32_cannot_hold_and_keeps_the_sign_of_zero():
    rows = np.array([[-0.0, 0.0, 1.5, 2.0 ** 24, 0.1, 0.5, 1.0]])
    with pytest.raises(AssertionError):
        mr.want_bits(rows)                                            # 0.1 is a double
    rows[0, 4] = np.float32(0.1)
    keep = rows.copy()
    bits = mr.want_bits(rows)
    assert bits[0, 0] == 0x80000000 and bits[0, 1] == 0 and bits[0, 3] == 0x4B800000 and np.array_equal(rows, keep)
    with pytest.raises(AssertionError):
        mr.want_bits(np.array([[2.0 ** 24 + 1, 0, 0, 0, 0, 0, 0]]))


@pytest.mark.parametrize("name", by_cost(["lattice_a", "lattice_b", "lattice_c", "lattice_d"]))
def test_lattice_reaches_the_value_set_branches(name):
    n, side, low, labels, _, longest = mr.LATTICE[name[-1]]
    det = CASES[name]()
    assert len(det) == n and det[:, :2].min() >= low and det[:, :2].max() < low + side and set(det[:, 6]) == set(labels)
    assert (det[:, :4] == np.round(det[:, :4])).all() and ((det[:, 2:4] - det[:, :2]) <= longest).all() and ((det[:, 2:4] - det[:, :2]) >= 0).all()
    assert (det[:, :2].min() < 0) == (low < 0)
    _, st = counted(name)
    print(name, {k: v for k, v in st.items() if not isinstance(v, list)})
    assert st["present"] >= 5 and st["flagged"] >= 1 and st["value_skips"] >= 1 and st["passes"] >= 5
    if name == "lattice_d":                          # a merged row that equals a live row which is itself flagged
        assert st["present_flagged"] >= 1


@pytest.mark.slow
def test_capacity_fills_the_table():
    rows, st = counted("capacity")
    print("capacity", {k: v for k, v in st.items() if not isinstance(v, list)})
    assert st["rows_ever"] == 2 * mr.MAX_ROWS - 1 and st["merges"] == mr.MAX_ROWS - 1 and len(rows) == 1
    # the outermost box, one pixel short on the far sides per level of the ten-level merge tree (1024 = 2^10)
    assert st["passes"] == 11 and rows[0].tolist() == [3000 - 3 * 1023, 3000 - 3 * 1023, 3002 + 3 * 1023 - 10, 3002 + 3 * 1023 - 10, 0.5, 0.5, 1]


def test_the_stride_plan_holds_every_pair_once():
    plan = mr.stride_plan()
    pairs = [p for img in plan for p in img]
    assert sorted(pairs) == sorted((i, i + d) for i in mr.STRIDE_STARTS for d in mr.STRIDE_DISTANCES if i + d < mr.MAX_ROWS)
    assert {j - i for i, j in pairs} == set(mr.STRIDE_DISTANCES) and (0, 1023) in plan[mr.STRIDES_WIDE]
    for img in plan:
        used = [r for p in img for r in p]
        assert len(used) == len(set(used))


@pytest.mark.parametrize("k", [pytest.param(k, marks=pytest.mark.slow) if k == mr.STRIDES_WIDE else k for k in range(len(mr.stride_plan()))])
def test_every_planned_pair_merges(k):
    _, st = counted(f"strides{k}")
    assert sorted(st["merged_pairs"]) == sorted(mr.stride_plan()[k]) and st["present"] == 0 and st["dups"] == 0


def test_a_partner_one_pixel_on_is_present_and_the_next_one_merges():
    _, st = counted("strides_present")
    print("strides_present", {k: v for k, v in st.items() if not isinstance(v, list)})
    for i, j1, j2 in mr.PRESENT_THEN_MERGE:
        assert j2 - j1 >= 64 and i in st["present_rows"] and (i, j2) in st["merged_pairs"]
    assert st["present"] >= 1 and st["merges"] >= 1
    # without the second partner nothing merges at all: the merged box is the mate itself
    det = mr.grid(256)
    mr._plant(det, 0, 1, 1)
    rows, st = mr.ordered_counted(det)
    assert st["merges"] == 0 and st["present"] == 1 and np.array_equal(rows, det.astype(np.float64))


def test_duplicates_collapse_as_planned():
    det, planned = mr.dups_strides()
    rows, st = counted("dups_strides")
    assert st["dups"] == planned == 6 and all((det[k] == det[0]).all() for k in mr.DUP_AT) and st["merges"] == 1
    det, planned = mr.dups_small()
    rows, st = counted("dups_small")
    assert st["dups"] == planned == 4
    assert len(mr.row_set(det[7:])) == 7 and not any(mr.row_set(det[7 + c:8 + c]) & mr.row_set(det[:1]) for c in range(7))
    assert ((det[7:] != det[0]).sum(1) == 1).all() and sorted((det[7:] != det[0]).argmax(1)) == list(range(7))
    zeros = rows[rows[:, 6] == 2]
    assert zeros[:, 0].tolist() == [0, 0] and np.signbit(zeros[:, 0]).tolist() == [True, False]      # the first one's bits survive


def test_truncation_case_tells_int_from_floor():
    det = CASES["truncation"]()
    rows, st = counted("truncation")
    print("truncation", {k: v for k, v in st.items() if not isinstance(v, list)})
    side = det[:, 2:4] - det[:, :2]
    assert len(det) == 300 and (det[:, 0] < 0).any() and ((side > 0) & (side < 1)).any() and (side[:, 0] < 0).sum() == 2
    assert set(np.unique(det[:, :4] % 1)) == {0.0, 0.5, 0.75, 0.25} and set(det[:, 6]) == {0, 1, 2}
    assert st["merges"] >= 20
    floor = mr.floor_variant(det)
    print("floor variant:", len(floor), "rows, int():", len(rows), "rows,", len(mr.row_set(floor) ^ mr.row_set(rows)), "rows differ")
    assert mr.row_set(floor) != mr.row_set(rows)
    pairs = CASES["truncation_pairs"]()
    assert mr.row_set(mr.floor_variant(pairs)) != mr.row_set(counted("truncation_pairs")[0])
    assert (pairs[-2:, :4] >= 100000).all() and counted("truncation_pairs")[0][-1].tolist() == [100000, 100000, 100058, 100049, 0.5, 0.5, 1]   # widths int(40), int(39.5)


def test_labels_other_than_zero_and_one_stay():
    rows, st = counted("labels")
    assert st["merges"] == 3 and len(rows) == 13
    assert [r for r in rows.tolist() if r[6] not in (0, 1)] == [r for r in CASES["labels"]().astype(np.float64).tolist() if r[6] not in (0, 1)]
    merged = rows[-3:]
    assert merged[:, 6].tolist() == [0, 0, 1] and np.signbit(merged[:, 6]).tolist() == [True, False, False]
    assert (merged[:, 2] - merged[:, 0] == 24).all() and (merged[:, 4:6] == 0.5).all()
    assert rows[8:10].tolist() == CASES["labels"]()[12:14].astype(np.float64).tolist()               # 0 over 1: both stay


@pytest.mark.parametrize("name", by_cost(mr.PAIR_ONLY))
def test_host_twin_and_oracle_agree_on_pair_only_images(name):
    """postprocess.merge_detections walks in the order of CPython's set; where no cluster has more than two rows the order cannot show"""
    det = CASES[name]()
    _, st = counted(name)
    hit = {r for p in st["merged_pairs"] for r in p}
    assert len(hit) == 2 * st["merges"] and max(hit) < len(det) and st["passes"] == 2            # no row merges twice, no merged row again
    got = merge_detections(torch.from_numpy(det.copy()))
    assert got.dtype == torch.float32 and mr.row_set(got.numpy()) == mr.row_set(counted(name)[0])


def test_count_batches_are_what_the_gpu_test_takes_them_for():
    for m in mr.COUNT_MAX_ROWS[:4]:
        rows, count, valid = mr.count_batch(m)
        assert rows.shape == (6, m, 7) and count.tolist() == [m, m + 5, 1 << 30, 1, 0, -3] and valid == [m, m, m, min(1, m), 0, 0]
        assert len({rows[b].tobytes() for b in range(3)}) == 3
        for b in range(6):
            tail = rows[b, valid[b]:]
            assert (tail[:, 6] == 1).all() and len(mr.row_set(tail)) == len(tail)
            if len(tail) > 1:                                                  # read by mistake, the rows behind count[b] would merge
                assert len(bo.merge_detections_ordered(tail)) == 1


@pytest.mark.slow
def test_the_older_gpu_tests_inputs_never_reach_the_value_set_branches():
    total = 0
    for name, det in mr.parity_inputs().items():
        rows, st = mr.ordered_counted(det)
        assert np.array_equal(rows, bo.merge_detections_ordered(det)), name
        assert st["present"] == 0 and st["flagged"] == 0 and st["value_skips"] == 0, (name, st)
        assert len(det) == 0 or det[:, :4].min() > 0
        total += st["merges"]
    assert total > 500                                                          # not for want of merges
