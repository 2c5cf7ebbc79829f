"""The restatement of the merge in the kernels' order (tests/nms_exact_reference.py) against the oracle, and the property of the
shared inputs that makes the order of the sums visible.  No GPU."""
import numpy as np
import pytest

import nms_exact_reference as R


@pytest.mark.parametrize("C", [3, 6])
def test_restatement_agrees_with_the_oracle(C):
    """Same heads by construction; the merged corners within the 1e-5 relative bound that tests/test_gpu_nms.py holds the kernels to."""
    case = R.exact_case(C)
    np.testing.assert_array_equal((case.pred[..., 4] >= np.float32(R.CONF_THRES)).sum(1), case.ncand)
    for b, rows in enumerate(case.rows):
        if rows is None:
            assert case.ncand[b] == 0
            continue
        a, o = rows.astype(np.float64), case.o_rows[b].astype(np.float64)
        assert a.shape == o.shape == (len(case.keep[b]), 7)
        err = np.abs(a - o) / np.maximum(1.0, np.abs(o))
        assert err.max() <= 1e-5, (b, float(err.max()))
        np.testing.assert_array_equal(rows[:, 4:].view(np.uint32), case.o_rows[b][:, 4:].view(np.uint32))


@pytest.mark.parametrize("C", [3, 6])
def test_inputs_make_the_order_of_the_sums_visible(C):
    """Every image with at least 1 000 candidates has a cluster of 8 or more members that spread over three or more alive words
    (j >> 6) and put two members into one lane (j & 63): its sums depend on the word order, the lane assignment and the butterfly."""
    case = R.exact_case(C)
    for b, n in enumerate(case.ncand):
        if n < 1000:
            continue
        pos = R.sorted_positions(case.corners[b])
        telling = 0
        for members in case.clusters[b]:
            j = pos[members]
            telling += j.size >= 8 and np.unique(j >> 6).size >= 3 and np.unique(j & 63).size < j.size
        assert telling >= 1, (b, int(n))
