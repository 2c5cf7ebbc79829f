"""Host -> device streaming (-m gpu): upload.Uploader's round trip with reuse and growth, a run that is left early, an exception
in fill; wsi.StripStream's blocks against the raster slices the rule names; wsi.SlideSampler across an abandoned iteration against
what the commit before the uploader yielded (tests/sampler_sequence.py).  Every comparison is of bytes."""
import json
import os

import numpy as np
import pytest
import torch

import sampler_sequence
from amyloid_yolo_paper_amd.upload import Uploader
from amyloid_yolo_paper_amd.wsi import StripStream, tile_grid

pytestmark = pytest.mark.gpu

SIZES = [3, 4096, 100003, 16, 250000, 1, 65536]      # with capacity 4096: buffer 0 takes 3, 100003, 250000, 65536 and grows twice
CAPACITY = 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module")
def busy(dev):
    """a few milliseconds of unrelated work on the current stream: an upload two jobs later is ready before a read queued behind it
    has run, so a read that is not ordered by ``consumed`` sees the later job's bytes"""
    a = torch.ones(2048, 2048, device=dev)

    def work():
        for _ in range(8):
            torch.mm(a, a)
    work()
    torch.cuda.synchronize()
    return work


def payloads(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=n, dtype=np.uint8) for n in sizes]


def stream(up, data, dev, busy, calls=None, fail_at=None, leave_after=None, release=True):
    """the jobs ``data`` through ``up`` -> (idx, what the device buffer held, read behind ``busy`` on the current stream)"""
    def fill(idx, host):
        if calls is not None:
            calls.append(idx)
        if idx == fail_at:
            raise KeyError(f"job {idx}")
        host(data[idx].size)[:data[idx].size] = data[idx]
        return idx, data[idx].size

    for k, idx, buf, nbytes in up.run(len(data), fill):
        busy()
        held = torch.empty(nbytes, dtype=torch.uint8, device=dev).copy_(buf[:nbytes])
        if release or idx != leave_after:
            up.release(k)
        yield idx, held
        if idx == leave_after:
            break


def run(*args, **kw):
    return list(stream(*args, **kw))


def assert_jobs(got, data, n=None):
    torch.cuda.synchronize()
    assert [idx for idx, _ in got] == list(range(len(data) if n is None else n))
    for idx, t in got:
        assert t.cpu().numpy().tobytes() == data[idx].tobytes(), f"job {idx}"


@pytest.mark.parametrize("lead", [0, 1])     # one 1-byte job in front: the other buffer then takes the large jobs and grows twice
def test_round_trip_with_reuse_and_growth(dev, busy, lead):
    data = payloads(lead, [1] * lead + SIZES)
    up = Uploader(dev, CAPACITY)
    first = [b.data_ptr() for b in up._device]
    assert_jobs(run(up, data, dev, busy), data)
    assert up._device[lead].numel() == up._pinned[lead].numel() == 250000 * 5 // 4         # by way of 100003 * 5 // 4
    assert up._device[1 - lead].numel() == up._pinned[1 - lead].numel() == CAPACITY
    assert up._device[1 - lead].data_ptr() == first[1 - lead]         # the buffer that never had to grow was not replaced


@pytest.mark.parametrize("release", [True, False])
def test_a_run_that_is_left_early_costs_the_next_one_nothing(dev, busy, release):
    a, b = payloads(2, [5000, 300, 70000, 9, 1234]), payloads(3, [1234, 70001, 2, 4097, 640])
    up = Uploader(dev, CAPACITY)
    calls = []
    assert_jobs(run(up, a, dev, busy, calls, leave_after=2, release=release), a, 3)
    assert_jobs(run(up, b, dev, busy), b)
    assert calls == [0, 1, 2, 3]              # job 3 was staged ahead when the run was left; nothing of the first run after that


def test_an_exception_in_fill_reaches_the_consumer_at_its_job(dev, busy):
    data = payloads(4, [700, 5000, 33, 100, 8])
    up = Uploader(dev, CAPACITY)
    got = []
    with pytest.raises(KeyError, match="job 3"):
        for item in stream(up, data, dev, busy, fail_at=3):
            got.append(item)
    assert_jobs(got, data, 3)
    assert_jobs(run(up, data, dev, busy), data)


@pytest.mark.parametrize("spans", [False, True])
@pytest.mark.parametrize("shrink", [1, 2])
def test_strip_geometry(dev, shrink, spans):
    """37 x 21 x 3: rows 63 bytes apart, no multiple of 16; height 16, step 14: two shared rows, a ragged last strip"""
    raster = np.random.default_rng(7).integers(0, 256, size=(37, 21, 3), dtype=np.uint8)
    height, step = 16, 14
    count = tile_grid(37 // shrink, 21 // shrink, height, height - step)[0]
    assert count == {1: 3, 2: 2}[shrink]
    jobs = [(j, j + 1, 21 - 2 * j) for j in range(count) if j != 1] if spans else None      # strip 1 is skipped
    strips = StripStream(raster, height, step, shrink, jobs)
    assert strips.count == count
    seen = []
    for j, k, rows, width in strips:
        block = strips.blocks[k][:rows * width * 3].clone()
        assert strips.args(k, rows, width)[1:] == (rows, width, width * 3, shrink)
        strips.release(k)
        c0, c1 = (j + 1, 21 - 2 * j) if spans else (0, 21)
        want = raster[j * step * shrink:(j * step + height) * shrink, c0:c1]
        assert (rows, width) == want.shape[:2]
        assert block.cpu().numpy().tobytes() == want.tobytes(), f"strip {j}"
        seen.append(j)
    assert seen == [j for j in range(count) if not (spans and j == 1)]
    assert strips.staged_bytes() == sum(raster[j * step * shrink:(j * step + height) * shrink, c0:c1].size
                                        for j, c0, c1 in strips.jobs)


def test_sampler_across_an_abandoned_iteration_yields_what_it_yielded_before(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "sampler_abandoned.json")))
    assert len(want["whole"]) == 4 and len(want["left_first"]) == 1 and len(want["left_again"]) == 4
    assert sampler_sequence.sequence() == want
