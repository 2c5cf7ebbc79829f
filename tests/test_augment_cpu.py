"""Training augmentation, host side (no GPU): the NumPy restatement of THE AUGMENTATION RULE against the ingest oracle, the parameter
sampler, the label rule in closed form, and the raw form of the loader."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
from PIL import Image

import augment_reference as ar
from amyloid_yolo_paper_amd import _lib, augment as ag
from amyloid_yolo_paper_amd.datasets import ListDataset, default_transform
from oracle.ingest_oracle import ingest

# (h, w, S): square, wide, tall, and an S that is not a multiple of 4 (the geometries the rule was prototyped on)
GEOMETRIES = [(96, 96, 64), (90, 150, 96), (150, 90, 70), (64, 48, 33)]


def rand_img(seed, h, w):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


# ---- the reference itself -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,S", GEOMETRIES)
def test_reference_identity_is_the_ingest_oracle(h, w, S):
    img = rand_img(h * 7 + w, h, w)
    got = ar.augment(img, S, ar.record(h, w))
    assert got.tobytes() == ingest(img, S).numpy().tobytes()


@pytest.mark.slow
def test_reference_identity_is_the_ingest_oracle_at_tile_scale():
    img = rand_img(5, 1536, 1536)
    assert ar.augment(img, 1024, ar.record(1536, 1536)).tobytes() == ingest(img, 1024).numpy().tobytes()


def test_identity_table_is_the_reference_identity_record():
    t = ag.identity_params([(90, 150), (64, 48)])
    for i, (h, w) in enumerate([(90, 150), (64, 48)]):
        got, want = ar.from_row(t.dev[i]), ar.record(h, w)
        for k in want:
            assert np.array_equal(got[k], want[k]), k
    assert t.dev["src_offset"].tolist() == [0, 90 * 150 * 3]


def test_reference_operations_do_something():
    """flip mirrors the ingest; a dropped pixel is `bright`; sharpen leaves a flat image alone"""
    h, w, S = 96, 96, 64
    img = rand_img(3, h, w)
    base = ar.augment(img, S, ar.record(h, w))
    assert np.array_equal(ar.augment(img, S, ar.record(h, w, flip=1)), ingest(img[:, ::-1], S).numpy())
    all_dropped = ar.augment(img, S, ar.record(h, w, drop_threshold=2 ** 32 - 1, bright=51.0))
    assert (all_dropped == np.float32(51.0) / np.float32(255.0)).all()
    frac = (ar.drop_hash(256, 1234) < np.uint32(0.01 * 2 ** 32)).mean()
    assert 0.007 < frac < 0.013                                   # the hash drops about p of the pixels
    flat = np.full((h, w, 3), 100, np.uint8)
    inner = ar.augment(flat, S, ar.record(h, w, sharpen_alpha=0.2))
    assert (inner == np.float32(100) / np.float32(255)).all()
    assert not np.array_equal(ar.augment(img, S, ar.record(h, w, sharpen_alpha=0.2)), base)


# ---- ABI mirror -----------------------------------------------------------------------------------------------------------------
def test_record_mirrors_agree():
    assert ag.AUG_DTYPE.itemsize == ctypes.sizeof(_lib.AugParams) == 96
    for name, _ in _lib.AugParams._fields_:
        assert ag.AUG_DTYPE.fields[name][1] == getattr(_lib.AugParams, name).offset, name
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "amyloid_yolo.h")).read()
    body = text[text.index("typedef struct ay_aug_params {"):text.index("} ay_aug_params;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"(\w+)(?:\[\d+\])?\s*[;,]", body)
    assert declared == [n for n, _ in _lib.AugParams._fields_]      # the header declares the fields in the mirrors' order


# ---- sampler --------------------------------------------------------------------------------------------------------------------
SIZES = [(96, 96), (90, 150), (150, 90), (1536, 1536)]


def test_sampler_is_reproducible_per_seed_and_rank():
    a = ag.DeviceAugmenter(11, rank=0).rng
    b = ag.DeviceAugmenter(11, rank=0).rng
    c = ag.DeviceAugmenter(11, rank=1).rng
    ta, tb, tc = (ag.sample_params(r, SIZES) for r in (a, b, c))
    assert ta.dev.tobytes() == tb.dev.tobytes() and np.array_equal(ta.A, tb.A)
    assert ta.dev.tobytes() != tc.dev.tobytes()
    assert ag.sample_params(a, SIZES).dev.tobytes() != ta.dev.tobytes()      # the stream moves on


def test_sampler_values_lie_in_their_ranges():
    g = ag.AugmentRanges()
    rng = np.random.default_rng(2)
    flips = []
    for _ in range(50):
        t = ag.sample_params(rng, SIZES, g)
        for i, (h, w) in enumerate(SIZES):
            A, r = t.A[i], t.dev[i]
            deg = math.degrees(math.atan2(A[1, 0], A[0, 0]))
            assert abs(deg) <= g.rotate + 1e-9 and abs(A[0, 0] - A[1, 1]) < 1e-15 and abs(A[0, 1] + A[1, 0]) < 1e-15
            assert abs(A[0, 2]) <= g.translate * w and abs(A[1, 2]) <= g.translate * h
            assert abs(float(r["bright"])) <= g.brightness
            assert 0.0 <= float(r["sharpen_alpha"]) <= np.float32(g.sharpen)
            assert 0 <= int(r["drop_threshold"]) <= math.floor(g.dropout * 2 ** 32)
            assert int(r["flip"]) in (0, 1) and (int(r["h"]), int(r["w"])) == (h, w)
            M = r["color"].astype(np.float64).reshape(3, 3)
            assert np.allclose(M @ M.T, np.eye(3), atol=1e-6) and np.allclose(M @ np.ones(3), np.ones(3), atol=1e-6)   # grey axis fixed
            hue = math.degrees(math.acos(min(1.0, (np.trace(M) - 1) / 2)))
            assert hue <= g.hue * ag.HUE_UNIT_DEGREES + 1e-3
            flips.append(int(r["flip"]))
    assert 0.35 < np.mean(flips) < 0.65


def test_inverse_is_the_fp32_rounding_of_the_float64_inverse():
    t = ag.sample_params(np.random.default_rng(4), SIZES)
    for i in range(len(SIZES)):
        A3 = np.vstack([t.A[i], [0, 0, 1]])
        want = np.linalg.inv(A3)[:2].astype(np.float32).ravel()
        assert t.dev[i]["inv"].tobytes() == want.tobytes()
        assert np.allclose(np.vstack([t.dev[i]["inv"].reshape(2, 3), [0, 0, 1]]).astype(np.float64) @ A3, np.eye(3), atol=1e-4)
    p = 0.0037
    t = ag.make_table([(8, 8)], drop_p=[p])
    assert int(t.dev[0]["drop_threshold"]) == math.floor(p * 2 ** 32)


@pytest.mark.parametrize("field", ["rotate", "translate", "brightness", "hue", "dropout", "sharpen", "fliplr"])
def test_a_switched_off_range_yields_the_identity_value(field):
    g = ag.AugmentRanges(**{field: 0.0})
    ident = ag.identity_params(SIZES)
    for seed in range(5):
        t = ag.sample_params(np.random.default_rng(seed), SIZES, g)
        full = ag.sample_params(np.random.default_rng(seed), SIZES)
        for i in range(len(SIZES)):
            r, f, e = t.dev[i], full.dev[i], ident.dev[i]
            if field == "rotate":
                assert t.A[i][0, 0] == 1.0 and t.A[i][0, 1] == 0.0 and t.A[i][1, 0] == 0.0 and t.A[i][1, 1] == 1.0
                assert np.array_equal(r["inv"][[0, 1, 3, 4]], e["inv"][[0, 1, 3, 4]])
            elif field == "translate":
                assert t.A[i][0, 2] == 0.0 and t.A[i][1, 2] == 0.0 and r["inv"][2] == 0.0 and r["inv"][5] == 0.0
            else:
                key = {"brightness": "bright", "hue": "color", "dropout": "drop_threshold", "sharpen": "sharpen_alpha", "fliplr": "flip"}[field]
                assert np.array_equal(r[key], e[key])
                assert np.array_equal(r["inv"], f["inv"])             # the other draws are what they were
    everything_off = ag.sample_params(np.random.default_rng(0), SIZES, ag.OFF)
    ident.dev["drop_seed"] = everything_off.dev["drop_seed"]           # (the seed is drawn but never used)
    assert everything_off.dev.tobytes() == ident.dev.tobytes()


# ---- labels, closed form --------------------------------------------------------------------------------------------------------
def rec(A=None, flip=0):
    return ag.make_table([(1, 1)], A=None if A is None else [A], flip=[flip])[0]


BOX = np.array([[2.0, 0.30, 0.40, 0.20, 0.10]])


def test_labels_flip_only():
    got = ag.transform_labels(BOX, 200, 200, rec(flip=1))
    assert np.allclose(got, [[2.0, 0.70, 0.40, 0.20, 0.10]], atol=1e-12)


def test_labels_translation_only():
    got = ag.transform_labels(BOX, 200, 200, rec(ag.forward_matrix(0.0, 20.0, -10.0)))
    assert np.allclose(got, [[2.0, 0.40, 0.35, 0.20, 0.10]], atol=1e-12)


def test_labels_quarter_turn_swaps_width_and_height():
    got = ag.transform_labels(BOX, 200, 200, rec(ag.forward_matrix(90.0, 0.0, 0.0)))
    # (x, y) - c -> (-(y - c), x - c): cx' = 1 - cy, cy' = cx
    assert np.allclose(got, [[2.0, 0.60, 0.30, 0.10, 0.20]], atol=1e-12)


def test_labels_box_outside_is_dropped_and_half_outside_is_clipped():
    two = np.array([[0.0, 0.30, 0.40, 0.20, 0.10], [1.0, 0.80, 0.50, 0.20, 0.20]])
    got = ag.transform_labels(two, 200, 200, rec(ag.forward_matrix(0.0, 40.0, 0.0)))       # +0.2 in x
    # box 0 moves to cx .5; box 1 spans [.9, 1.1] -> clipped to [.9, 1]
    assert np.allclose(got, [[0.0, 0.50, 0.40, 0.20, 0.10], [1.0, 0.95, 0.50, 0.10, 0.20]], atol=1e-12)
    got = ag.transform_labels(two, 200, 200, rec(ag.forward_matrix(0.0, 70.0, 0.0)))       # +0.35: box 1 spans [1.05, 1.25]
    assert got.shape == (1, 5) and got[0, 0] == 0.0
    assert ag.transform_labels(np.zeros((0, 5)), 200, 200, rec()).shape == (0, 5)


@pytest.mark.parametrize("h,w", [(90, 150), (150, 90), (101, 60)])
def test_labels_identity_on_a_non_square_tile_is_default_transform(h, w):
    boxes = np.array([[1.0, 0.3, 0.4, 0.2, 0.1], [0.0, 0.7, 0.6, 0.25, 0.3]])
    _, want = default_transform(np.zeros((h, w, 3), np.uint8), boxes)
    got = ag.transform_labels(boxes, h, w, rec())
    assert np.allclose(got, want[:, 1:].numpy().astype(np.float64), atol=1e-6)
    assert got.dtype == np.float64
    # and moved: against the corner-by-corner restatement
    r = rec(ag.forward_matrix(17.0, 0.1 * w, -0.05 * h), flip=1)
    assert np.allclose(ag.transform_labels(boxes, h, w, r), ar.labels(boxes, h, w, r.A, 1), atol=1e-12)


def test_labels_against_the_restatement_over_random_records():
    rng = np.random.default_rng(9)
    for _ in range(40):
        h, w = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        n = int(rng.integers(0, 6))
        boxes = np.concatenate([rng.integers(0, 3, (n, 1)).astype(np.float64), rng.uniform(0.1, 0.9, (n, 2)), rng.uniform(0.02, 0.3, (n, 2))], 1)
        t = ag.sample_params(rng, [(h, w)])
        got = ag.transform_labels(boxes, h, w, t[0])
        want = ar.labels(boxes, h, w, t.A[0], t[0].flip)
        assert got.shape == want.shape and np.allclose(got, want, atol=1e-12)
        if len(got):
            assert (got[:, 1:] >= 0).all() and (got[:, 1:] <= 1).all()


# ---- device entry without a device ----------------------------------------------------------------------------------------------
def test_augment_ingest_without_gpu_raises():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.AyError):
        ag.augment_ingest_device([rand_img(0, 8, 8)], ag.identity_params([(8, 8)]), 8)


# ---- raw loader -----------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def tile_list(tmp_path):
    (tmp_path / "images").mkdir()
    (tmp_path / "labels").mkdir()
    paths, imgs, labels = [], [], []
    for i, (h, w, n) in enumerate([(40, 40, 2), (30, 50, 0), (50, 30, 1)]):
        img = rand_img(100 + i, h, w)
        p = str(tmp_path / "images" / f"t{i}.png")
        Image.fromarray(img).save(p)
        lab = np.random.default_rng(i).uniform(0.2, 0.6, (n, 5))
        lab[:, 0] = i
        np.savetxt(str(tmp_path / "labels" / f"t{i}.txt"), lab)
        paths.append(p), imgs.append(img), labels.append(lab.reshape(-1, 5))
    paths.append(str(tmp_path / "images" / "missing.png"))           # unreadable: dropped by the collate step
    lst = tmp_path / "train.txt"
    lst.write_text("\n".join(paths) + "\n")
    return str(lst), paths, imgs, labels


def test_raw_loader_hands_out_bytes_and_label_rows(tile_list):
    lst, paths, imgs, labels = tile_list
    ds = ListDataset(lst, img_size=64, multiscale=False, raw_u8=True)
    with pytest.warns(UserWarning):
        items = [ds[i] for i in range(len(ds))]
    assert items[3] is None
    for i in range(3):
        p, tile, boxes = items[i]
        assert p == paths[i] and tile.dtype == torch.uint8 and np.array_equal(tile.numpy(), imgs[i])
        assert boxes.shape == (len(labels[i]), 5) and np.allclose(boxes.numpy(), labels[i])
    got_paths, tiles, boxes, size = ds.collate_fn(items)
    assert got_paths == tuple(paths[:3]) and size == 64 and len(tiles) == len(boxes) == 3
    assert all(np.array_equal(t.numpy(), im) for t, im in zip(tiles, imgs))
    # the size comes from the unchanged schedule
    ms = ListDataset(lst, img_size=416, multiscale=True, raw_u8=True)
    sizes = {ms.collate_fn(items)[3] for _ in range(40)}
    assert sizes <= set(range(320, 513, 32)) and len(sizes) > 1


def test_default_loader_is_what_it_was(tile_list):
    lst, paths, imgs, labels = tile_list
    ds = ListDataset(lst, img_size=64, multiscale=False)
    assert ds.raw_u8 is False
    with pytest.warns(UserWarning):
        items = [ds[i] for i in range(len(ds))]
    got_paths, batch, targets = ds.collate_fn(items)
    assert got_paths == tuple(paths[:3]) and batch.shape == (3, 3, 64, 64) and batch.dtype == torch.float32
    for i in range(3):
        assert torch.equal(batch[i], ingest(imgs[i], 64))
        _, want = default_transform(imgs[i], labels[i])
        assert torch.equal(targets[targets[:, 0] == i][:, 1:], want[:, 1:])
