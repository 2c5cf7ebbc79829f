"""CPU: the layout of a buffer that carries pixels and their records in one copy (upload.record_offset, upload.pack_records)."""
import numpy as np
import pytest

from amyloid_yolo_paper_amd.upload import pack_records, record_offset


@pytest.mark.parametrize("n,tab", [(0, 0), (1, 16), (15, 16), (16, 16), (17, 32)])
def test_records_lie_on_the_next_16_bytes_behind_the_pixels(n, tab):
    records = np.random.default_rng(n).integers(0, 2 ** 32, size=12, dtype=np.uint32)       # a 48-byte record block
    before = np.random.default_rng(100 + n).integers(0, 256, size=tab + 48 + 8, dtype=np.uint8)
    buf = before.copy()
    assert record_offset(n) == tab and tab % 16 == 0 and n <= tab < n + 16
    assert pack_records(buf, n, records) == tab
    assert buf[tab:tab + 48].tobytes() == records.tobytes()
    assert np.array_equal(buf[:tab], before[:tab]) and np.array_equal(buf[tab + 48:], before[tab + 48:])      # the gap and the rest stay
