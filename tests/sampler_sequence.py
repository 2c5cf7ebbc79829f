"""What a wsi.SlideSampler yields across an abandoned iteration, as SHA-256 digests (tests/test_gpu_upload.py).

Two samplers with the same seed over one host raster: ``whole`` is iterated once to the end; ``left`` is iterated for one batch,
left, and iterated again to the end.  The batch that was staged ahead when ``left`` was abandoned is dropped with its draws, so the
second iteration of ``left`` starts two batches into the random stream.

The expectation in tests/golden/sampler_abandoned.json was written by the commit BEFORE the sampler moved onto upload.Uploader:

    python tests/sampler_sequence.py tests/golden/sampler_abandoned.json

run there on the GPU, never by the code under test."""
import hashlib
import json
import sys

import numpy as np

KW = dict(tile=32, img_size=32, batch_size=2, batches=4, seed=11)


def slide():
    rng = np.random.default_rng(5)
    raster = rng.integers(0, 256, size=(200, 240, 3), dtype=np.uint8)
    raster[:40, :60] = 255
    targets = np.array([[0, 20, 30, 44, 52], [1, 100, 90, 131, 118], [0, 180, 150, 206, 171], [1, 60, 160, 84, 190]], np.float64)
    return raster, targets


def digest(imgs, targets):
    h = hashlib.sha256()
    for t in (imgs, targets):
        a = t.cpu().numpy()
        h.update(str((a.dtype, a.shape)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def sequence():
    from amyloid_yolo_paper_amd.wsi import SlideSampler
    raster, targets = slide()
    mask = np.ones((-(-raster.shape[0] // KW["tile"]), -(-raster.shape[1] // KW["tile"])), np.bool_)
    whole, left = (SlideSampler([(raster, targets)], tile_mask=mask, **KW) for _ in range(2))
    out = {"whole": [digest(*b) for b in whole], "left_first": [], "left_again": []}
    for b in left:
        out["left_first"].append(digest(*b))
        break
    out["left_again"] = [digest(*b) for b in left]
    return out


if __name__ == "__main__":
    import amyloid_yolo_paper_amd
    print("written by", amyloid_yolo_paper_amd.__file__)
    with open(sys.argv[1], "w") as fh:
        json.dump(sequence(), fh, indent=1)
        fh.write("\n")
