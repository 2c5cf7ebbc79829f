"""Training augmentation on the device (-m gpu): ay_augment_ingest_u8 against the NumPy restatement of THE AUGMENTATION RULE
(tests/augment_reference.py) BIT FOR BIT, against ay_ingest_tiles_u8 under identity records, the image and its labels moving
together through the public DeviceAugmenter, and train(augment=True) end to end.  No tolerance anywhere on pixel values: a case
that is not exact means the rule or the kernel's operation order is wrong."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest
import torch

import augment_reference as ar
from amyloid_yolo_paper_amd import _lib, augment as ag, cfg_gen, synth
from amyloid_yolo_paper_amd._lib import check, ptr
from amyloid_yolo_paper_amd.datasets import ingest_tiles_device

pytestmark = pytest.mark.gpu

GUARD = 64
# (h, w, S): square, wide, tall, S % 4 != 0
GEOMETRIES = [(96, 96, 64), (90, 150, 96), (150, 90, 70), (64, 48, 33)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "run on the GPU box"
    return torch.device("cuda", 0)


def rand_img(seed, h, w):
    """random pixels with a few flat and saturated patches (so that clamps and exact zeros occur)"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    img[: h // 5, : w // 4] = 255
    img[h // 2: h // 2 + h // 6, w // 3: w // 2] = 0
    return img


def run_kernel(dev, imgs, recs, S, misalign=0, src_bytes=None):
    """the raw entry point on a ragged batch: imgs (list of uint8 [h,w,3]) packed one after another, recs (AUG_DTYPE rows, used as
    they are); the output starts `misalign` floats behind a 16-byte boundary and is followed by guard words.  Two runs."""
    B = len(imgs)
    src = torch.from_numpy(np.concatenate([np.asarray(i).reshape(-1) for i in imgs])).to(dev)
    table = torch.from_numpy(np.ascontiguousarray(recs).view(np.uint8).reshape(-1).copy()).to(dev)
    n = B * 3 * S * S
    buf = torch.empty(misalign + n + GUARD, device=dev, dtype=torch.float32)
    assert buf.data_ptr() % 16 == 0
    outs = []
    for fill in (-7.0, 9.0):
        buf.fill_(fill)
        check(_lib.lib().ay_augment_ingest_u8(ptr(src), src.numel() if src_bytes is None else src_bytes, ptr(table), B, S,
                                              C.c_void_p(buf.data_ptr() + 4 * misalign), _lib.stream_ptr()), "ay_augment_ingest_u8")
        host = buf.cpu().numpy()
        assert (host[:misalign] == fill).all() and (host[misalign + n:] == fill).all()      # nothing written around the output
        outs.append(host[misalign:misalign + n].reshape(B, 3, S, S).copy())
    assert outs[0].tobytes() == outs[1].tobytes()                                          # two runs, the same bytes
    return outs[0]


def assert_bits(got, want, what):
    if got.tobytes() != want.tobytes():
        bad = got.view(np.uint32) != want.view(np.uint32)
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} values differ, first at {i}: {got[i]!r} vs {want[i]!r}, "
                             f"max |diff| {np.abs(got - want).max()}")


# ---- 1. identity records: the ingest ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,S", GEOMETRIES + [(1536, 1536, 1024)])
def test_identity_equals_ingest(dev, h, w, S):
    imgs = [rand_img(h + w + k, h, w) for k in range(2)]
    want = ingest_tiles_device(np.stack(imgs), S, pad_value=0.0).cpu().numpy()
    got = run_kernel(dev, imgs, ag.identity_params([(h, w)] * 2).dev, S)
    assert_bits(got, want, "identity vs ay_ingest_tiles_u8")
    got = ag.augment_ingest_device(imgs, ag.identity_params([(h, w)] * 2), S).cpu().numpy()   # and through the public wrapper
    assert_bits(got, want, "augment_ingest_device(identity) vs ay_ingest_tiles_u8")


# ---- 2. the rule, exact ----------------------------------------------------------------------------------------------------------
ALONE = {
    "rotate": dict(rotate=20.0), "translate": dict(translate=0.2), "flip": dict(fliplr=1.0), "sharpen": dict(sharpen=0.2),
    "dropout": dict(dropout=0.01), "brightness": dict(brightness=30.0), "hue": dict(hue=20.0),
    "all": dict(rotate=20.0, translate=0.2, fliplr=0.5, sharpen=0.2, dropout=0.01, brightness=30.0, hue=20.0),
    "harsh": dict(rotate=180.0, translate=0.6, fliplr=0.5, sharpen=1.0, dropout=0.3, brightness=200.0, hue=127.0),
}


def ranges_of(name):
    return ag.AugmentRanges(**{**vars(ag.OFF), **ALONE[name]})


def reference(imgs, table, S):
    return np.stack([ar.augment(img, S, ar.from_row(table.dev[i])) for i, img in enumerate(imgs)])


@pytest.mark.parametrize("op", list(ALONE))
def test_rule_bit_for_bit_on_ragged_batches(dev, op):
    """every operation alone, all together, and far beyond the default ranges; each batch is ragged (the four geometries in one
    buffer), each output size occurs with an aligned and with a misaligned output base"""
    sizes = [(h, w) for h, w, _ in GEOMETRIES]
    for seed in range(3):
        imgs = [rand_img(seed * 10 + k, h, w) for k, (h, w) in enumerate(sizes)]
        table = ag.sample_params(np.random.default_rng([seed, len(op)]), sizes, ranges_of(op))
        for S in (64, 96, 70, 33):
            want = reference(imgs, table, S)
            for misalign in (0, 1):
                assert_bits(run_kernel(dev, imgs, table.dev, S, misalign), want, f"{op} seed {seed} S {S} misalign {misalign}")


def test_rule_bit_for_bit_at_tile_scale(dev):
    """1536^2 -> 1024^2, everything on, two tiles"""
    sizes = [(1536, 1536)] * 2
    imgs = [(synth.synth_tiles(1, 1536, start=k)[0] * 255).astype(np.uint8).transpose(1, 2, 0).copy() for k in range(2)]
    table = ag.sample_params(np.random.default_rng(77), sizes, ranges_of("all"))
    assert_bits(run_kernel(dev, imgs, table.dev, 1024), reference(imgs, table, 1024), "1536^2 -> 1024^2")


def test_a_record_that_does_not_fit_the_buffer_reads_nothing(dev):
    """records whose image would not lie inside the source buffer are all padding (colour of black + brightness), the others of the
    batch are unaffected"""
    h, w, S = 96, 96, 64
    imgs = [rand_img(k, h, w) for k in range(4)]
    table = ag.sample_params(np.random.default_rng(3), [(h, w)] * 4, ranges_of("all"))
    want = reference(imgs, table, S)
    recs = table.dev.copy()
    n = 4 * h * w * 3
    recs[0]["h"] = 4096                                  # claims more rows than the buffer holds
    recs[1]["src_offset"] = -3
    recs[3]["src_offset"] = n - h * w * 3 + 1            # one byte over the end
    got = run_kernel(dev, imgs, recs, S)
    assert_bits(got[2], want[2], "the consistent record")
    for i in (0, 1, 3):
        black = ar.from_row(recs[i])
        black["h"], black["w"] = h, w
        assert_bits(got[i], ar.augment(np.zeros((h, w, 3), np.uint8), S, black), f"record {i}")


def test_bad_arguments_are_refused(dev):
    L = _lib.lib()
    x = torch.zeros(64, device=dev)
    assert L.ay_augment_ingest_u8(None, 10, ptr(x), 1, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_u8(ptr(x), 0, ptr(x), 1, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_u8(ptr(x), 10, ptr(x), 0, 8, ptr(x), None) == -1
    assert L.ay_augment_ingest_u8(ptr(x), 10, ptr(x), 1, 0, ptr(x), None) == -1 and b"ay_augment_ingest_u8" in L.ay_last_error()


# ---- 3. the image and its labels move together -----------------------------------------------------------------------------------
def pick_seed(h, w, box, ranges):
    """the first seed whose record (the one DeviceAugmenter(seed) draws first) flips, rotates by at least 10 degrees, shifts by at
    least 5 % and keeps the box 3 px inside the image -- decided on the CPU, before the GPU runs"""
    for seed in range(1000):
        t = ag.sample_params(np.random.default_rng([seed, 0]), [(h, w)], ranges)
        A = t.A[0]
        deg = abs(math.degrees(math.atan2(A[1, 0], A[0, 0])))
        if not (t[0].flip and deg >= 10.0 and abs(A[0, 2]) >= 0.05 * w and abs(A[1, 2]) >= 0.05 * h):
            continue
        _, bx, by, bw, bh = box[0]
        xs = np.array([bx - bw / 2, bx + bw / 2, bx - bw / 2, bx + bw / 2]) * w - w / 2
        ys = np.array([by - bh / 2, by - bh / 2, by + bh / 2, by + bh / 2]) * h - h / 2
        X = A[0, 0] * xs + A[0, 1] * ys + A[0, 2] + w / 2        # (the flip mirrors about the centre: inside stays inside)
        Y = A[1, 0] * xs + A[1, 1] * ys + A[1, 2] + h / 2
        if X.min() >= 3 and X.max() <= w - 3 and Y.min() >= 3 and Y.max() <= h - 3:
            return seed, t
    raise AssertionError("no seed found")


@pytest.mark.parametrize("h,w,S", [(300, 300, 200), (240, 320, 160), (320, 240, 200)])
def test_image_and_labels_move_together(dev, h, w, S):
    ranges = ag.AugmentRanges(rotate=20.0, translate=0.12, fliplr=1.0, brightness=0.0, hue=0.0, dropout=0.0, sharpen=0.0)
    box = np.array([[1.0, 0.45, 0.55, 0.30, 0.20]])
    seed, table = pick_seed(h, w, box, ranges)
    img = np.zeros((h, w, 3), np.uint8)
    x1, x2 = round(w * (0.45 - 0.15)), round(w * (0.45 + 0.15))
    y1, y2 = round(h * (0.55 - 0.10)), round(h * (0.55 + 0.10))
    assert abs(x1 - w * 0.30) < 1e-9 and abs(x2 - w * 0.60) < 1e-9 and abs(y1 - h * 0.45) < 1e-9 and abs(y2 - h * 0.65) < 1e-9
    img[y1:y2, x1:x2] = 255                                 # pixels [x1, x2) x [y1, y2): exactly the label's box
    aug = ag.DeviceAugmenter(seed, rank=0, ranges=ranges)
    imgs, targets = aug([torch.from_numpy(img)], [box], S)
    assert imgs.shape == (1, 3, S, S) and imgs.is_cuda and targets.is_cuda and targets.shape == (1, 6)
    t = targets.cpu().numpy().astype(np.float64)[0]
    want = ar.labels(box, h, w, table.A[0], 1)[0]
    assert t[0] == 0.0 and np.allclose(t[1:], want, atol=1e-6)     # sample index, then the restated label rule (float32 storage)
    D = max(h, w)
    ys, xs = np.nonzero((imgs[0, 0] > 0.5).cpu().numpy())
    assert len(xs) > 0
    q = D / S
    got = np.array([xs.min() * q, (xs.max() + 1) * q, ys.min() * q, (ys.max() + 1) * q])        # pixel i spans [i, i+1)
    _, cx, cy, bw, bh = t[1:]                               # a target row is (sample, class, cx, cy, w, h)
    exp = np.array([(cx - bw / 2) * D, (cx + bw / 2) * D, (cy - bh / 2) * D, (cy + bh / 2) * D])
    err = np.abs(got - exp)
    print(f"sides off by {err} source px, bound {q + 1}")
    assert (err <= q + 1).all(), (got, exp)


# ---- 4. train(augment=True) ------------------------------------------------------------------------------------------------------
def test_train_with_augmentation_is_finite_and_reproducible(tmp_path, tmp_cfg_dir):
    from PIL import Image
    from amyloid_yolo_paper_amd.train import train
    rng = np.random.Generator(np.random.PCG64(9))
    img_dir, lab_dir = tmp_path / "images", tmp_path / "labels"
    img_dir.mkdir()
    lab_dir.mkdir()
    paths = []
    for i, (h, w) in enumerate([(96, 96), (96, 96), (80, 120), (120, 80), (96, 96), (96, 96), (96, 96), (96, 96)]):
        arr = synth.synth_tile(50 + i, 120)[:h, :w]
        p = img_dir / f"t{i}.png"
        Image.fromarray(np.ascontiguousarray(arr)).save(p)
        n = int(rng.integers(1, 4))
        rows = [(int(rng.integers(0, 2)), *rng.uniform(0.3, 0.7, 2), *rng.uniform(0.1, 0.3, 2)) for _ in range(n)]
        (lab_dir / f"t{i}.txt").write_text("\n".join("%d %.6f %.6f %.6f %.6f" % r for r in rows) + "\n")
        paths.append(str(p))
    (tmp_path / "train.txt").write_text("\n".join(paths) + "\n")
    (tmp_path / "classes.names").write_text("CAA\nCored\n")
    (tmp_path / "custom.data").write_text(f"classes= 2\ntrain={tmp_path}/train.txt\nnames={tmp_path}/classes.names\n")
    cfg = cfg_gen.write_cfg(2, tmp_cfg_dir)
    digests = []
    for run in range(2):
        aug = ag.DeviceAugmenter(5, rank=0)
        seen = []
        aug.hooks.append(lambda imgs, targets: seen.append((hashlib.sha256(imgs.cpu().numpy().tobytes()).hexdigest(),
                                                            hashlib.sha256(targets.cpu().numpy().tobytes()).hexdigest(),
                                                            tuple(imgs.shape))))
        model, hist = train(epochs=1, batch_size=2, gradient_accumulations=2, model_def=cfg, data_config=str(tmp_path / "custom.data"),
                            n_cpu=0, img_size=96, multiscale_training=False, checkpoint_dir=str(tmp_path / f"ckpt{run}"), max_batches=4,
                            seed=5, precision="bf16", augment=True, augmenter=aug)
        assert len(hist) == 4 and all(np.isfinite(hist)), hist
        assert len(seen) == 4 and all(s[2] == (2, 3, 96, 96) for s in seen)
        digests.append(seen)
    assert digests[0] == digests[1]                               # the same seed: byte-identical batches and targets
    # and with the augmenter train() makes itself (DeviceAugmenter(seed, rank))
    _, hist = train(epochs=1, batch_size=2, gradient_accumulations=2, model_def=cfg, data_config=str(tmp_path / "custom.data"), n_cpu=0,
                    img_size=96, multiscale_training=False, checkpoint_dir=str(tmp_path / "ckpt2"), max_batches=2, seed=5, augment=True)
    assert len(hist) == 2 and all(np.isfinite(hist)), hist
    assert len({s[0] for s in digests[0]}) == 4                   # ... which differ from batch to batch
