"""Host -> device streaming, stated once: the double-buffered upload under every whole-slide pass and the slide sampler, and the
layout of a buffer that carries pixels and their records in one copy.  Nothing here knows about slides.

THE UPLOAD PROTOCOL (:class:`Uploader`).  Job ``idx`` uses pinned host buffer and device buffer ``k = idx & 1``.
  1. ``fill(idx, host)`` runs on the one staging thread, one job ahead of the consumer.  ``host(nbytes)`` hands it pinned buffer
     ``k`` only after the last upload out of that buffer has run (``uploaded[k]``, waited for on the host).
  2. The upload runs on the copy stream, behind ``consumed[k]``: every kernel that read device buffer ``k`` is done.
  3. The current stream waits for ``uploaded[k]``; the consumer issues its kernels there and calls ``release(k)``, which records
     ``consumed[k]``.
So no kernel sees a half-written buffer, and job ``idx + 1`` stages and uploads under the kernels of job ``idx``."""
from concurrent.futures import ThreadPoolExecutor, wait

import numpy as np
import torch


def record_offset(n):
    """where the record table starts behind ``n`` bytes of pixels: the next multiple of 16 (the kernels load records 16 bytes wide)"""
    return (int(n) + 15) // 16 * 16


def pack_records(buf, n, records):
    """Writes ``records`` (a contiguous NumPy array, taken as its bytes) into the flat uint8 view ``buf`` behind ``n`` bytes of
    pixels -> their offset, ``record_offset(n)``.  Pixels and records then go up in one copy; the bytes between are not touched."""
    rec = np.ascontiguousarray(records).reshape(-1).view(np.uint8)
    tab = record_offset(n)
    buf[tab:tab + rec.size] = rec
    return tab


def pinned(nbytes):
    """a pinned uint8 host tensor of ``nbytes``"""
    return torch.empty(nbytes, dtype=torch.uint8, pin_memory=nbytes > 0)


class Uploader:
    """THE UPLOAD PROTOCOL on device ``dev``: two pinned buffers, two device buffers, a copy stream, the staging thread and a pool of
    four copy threads (``pool``, for ``fill`` to split its copy over), all per instance.  ``capacity`` bytes are allocated up front
    (a caller that knows its largest job allocates nothing inside the loop); a larger job grows its buffers to 5/4 of its size."""

    def __init__(self, dev, capacity=0):
        self.dev = dev
        self.pool = ThreadPoolExecutor(max_workers=4)       # the parts of one staging copy
        self._stager = ThreadPoolExecutor(max_workers=1)    # one job ahead of the consumer
        self._copy = torch.cuda.Stream(device=dev)
        self._pinned = [pinned(capacity) for _ in range(2)]
        self._device = [torch.empty(capacity, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._uploaded = [None, None]    # event: the job landed in _device[k]
        self._consumed = [None, None]    # event: every kernel that read _device[k] is done
        self._ahead = None               # the job that is staged ahead, until the consumer takes it
        self._open = False               # a job was handed out and not released

    def _host(self, k, nbytes):
        if self._uploaded[k] is not None:
            self._uploaded[k].synchronize()      # the host buffer is free again once its last copy has run
        if self._pinned[k].numel() < nbytes:
            self._pinned[k] = pinned(nbytes * 5 // 4)
        return self._pinned[k].numpy()

    def _upload(self, k, nbytes, main):
        assert nbytes <= self._pinned[k].numel(), "fill returned more bytes than it asked host() for"
        if self._consumed[k] is not None:
            self._copy.wait_event(self._consumed[k])
        if self._device[k].numel() < nbytes:
            if self._consumed[k] is not None:
                self._consumed[k].synchronize()
            self._device[k] = torch.empty(self._pinned[k].numel(), dtype=torch.uint8, device=self.dev)
            self._copy.wait_stream(main)         # the memory may have served the current stream until now
        with torch.cuda.stream(self._copy):
            self._device[k][:nbytes].copy_(self._pinned[k][:nbytes], non_blocking=True)
            self._uploaded[k] = torch.cuda.Event()
            self._uploaded[k].record(self._copy)

    def run(self, n, fill):
        """Generator over jobs ``0 .. n - 1``.  ``fill(idx, host) -> (payload, nbytes)`` writes the job into ``host(nbytes)[:nbytes]``
        (a flat uint8 NumPy view of the pinned buffer) on the staging thread, with the device set.  Yields ``(k, payload,
        device_buffer, nbytes)`` once the current stream waits for the upload; the consumer issues every kernel that reads
        ``device_buffer[:nbytes]`` on the current stream and then calls ``release(k)``.  An exception of ``fill`` is raised here, at
        the job it belongs to.  When a run was left early, the next one waits for the job that was staged ahead and drops it."""
        main = torch.cuda.current_stream(self.dev)
        if self._ahead is not None:
            wait([self._ahead])
        if self._open:                           # left between a job and its release: that job's kernels carry no event
            self._copy.wait_stream(main)

        def job(idx):
            torch.cuda.set_device(self.dev)
            return fill(idx, lambda nbytes: self._host(idx & 1, nbytes))

        self._ahead = self._stager.submit(job, 0) if n else None
        for idx in range(n):
            fut, self._ahead = self._ahead, None
            payload, nbytes = fut.result()
            self._upload(idx & 1, nbytes, main)
            if idx + 1 < n:                      # staged while the consumer's work on this job runs
                self._ahead = self._stager.submit(job, idx + 1)
            main.wait_event(self._uploaded[idx & 1])
            self._open = True
            yield idx & 1, payload, self._device[idx & 1], nbytes

    def release(self, k):
        """device buffer ``k`` may be refilled behind everything the current stream holds now"""
        self._consumed[k] = torch.cuda.Event()
        self._consumed[k].record(torch.cuda.current_stream(self.dev))
        self._open = False
