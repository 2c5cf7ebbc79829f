"""Child process of tests/test_gpu_streams.py::test_more_streams_than_the_table_holds (the table of counter-set owners is
process-wide and never shrinks, so this cannot run inside the pytest process): one few-size dynamic launch on each of 18 distinct
streams, every output compared with the exact periodic reference.  Prints one line per stream

    stream <i> slot <slot> launches <sets taken> exact <0|1>

and a last line `nonzero <words>`; exits 0 when it got that far (the parent asserts on the lines)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import streams_reference as SR  # noqa: E402
from test_gpu_streams import probe  # noqa: E402

N_STREAMS = 18


def main():
    assert torch.cuda.is_available()
    dev = torch.device("cuda", 0)
    name, dtype = sys.argv[1], sys.argv[2]
    B, _, _ = SR.geometry(name, "few")
    p = SR.Prepared(dev, name, 7, dtype, B)
    streams = []
    for _ in range(64):      # distinct streams (torch hands its pool out in rotation)
        s = torch.cuda.Stream(device=dev)
        if all(s.cuda_stream != t.cuda_stream for t in streams):
            streams.append(s)
        if len(streams) == N_STREAMS:
            break
    assert len(streams) == N_STREAMS, len(streams)
    outs = []
    for s in streams:
        with torch.cuda.stream(s):
            outs.append(p.launch())
    torch.cuda.synchronize()
    nonzero = 0
    for i, (s, out) in enumerate(zip(streams, outs)):
        try:
            p.verify(out, f"stream {i}")
            exact = 1
        except AssertionError as exc:
            print(exc, file=sys.stderr)
            exact = 0
        slot, launches, nonzero = probe(s)
        print(f"stream {i} slot {slot} launches {launches} exact {exact}")
    print(f"nonzero {nonzero}")


if __name__ == "__main__":
    main()
