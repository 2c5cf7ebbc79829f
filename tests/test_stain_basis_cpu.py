"""Stain basis estimation without a GPU: the bounds THE BASIS RULE (include/amyloid_yolo.h) states, the floor of its division, the
host half of wsi.estimate_basis (wsi.basis_plane, wsi.basis_vectors, wsi.StainEstimate) against tests/stain_basis_reference.py on the
reference's own device passes, recovery of known stain vectors on synthetic slides, the guard and the assignment, the remix tables of
wsi.stain_tables / wsi.StainMap, and that normalising through each slide's own basis brings two slides closer than the fixed basis
does.  The device passes themselves are tested in tests/test_gpu_stain_basis.py."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import stain_basis_reference as br
import stain_reference as sref
from amyloid_yolo_paper_amd import _lib, wsi
from amyloid_yolo_paper_amd.wsi import H_DAB, StainBasis, StainEstimate, StainMap, StainStats

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRUE = (((0.60, 0.74, 0.30), (0.35, 0.60, 0.72)), ((0.55, 0.76, 0.34), (0.20, 0.50, 0.84)))
HAND_PLANE = (np.array([700, -650, 300], np.int32), np.array([-600, 250, 760], np.int32))     # p1 <= 0 and p2 < 0 both occur


@functools.lru_cache(maxsize=None)
def slide(vectors, share, seed=5, strength=(1.0, 1.0)):
    s = br.synthetic_slide(512, 768, vectors[0], vectors[1], share, seed, strength)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def passes(vectors, share, beta=0.15):
    """the reference's two device passes on a synthetic slide -> (moments, hist)"""
    s, bq = slide(vectors, share), br.beta_q(beta)
    m = br.moments(s, 1, 220, bq)
    eq1, eq2, _ = br.plane(m)
    return m, br.direction_hist(s, 1, 220, bq, eq1, eq2)


def product(vectors, share, alpha=1.0, prior=H_DAB, max_angle="half"):
    """the product's host half on the reference's passes"""
    m, h = passes(vectors, share)
    return StainEstimate(m, h, alpha, br.beta_q(), prior, wsi._check_basis_args(0.15, alpha, prior, max_angle)[2])


# ---- 1. the rule's bounds ----------------------------------------------------------------------------------------------------------------
def test_integer_od_table():
    t = br.odq()
    assert t[255] == 0 and t[0] == 2466 == br.OD_MAX and (np.diff(t) <= 0).all()
    assert list(wsi.basis_tables().odq) == t.tolist()
    assert bytes(wsi.basis_tables()) == t.astype(np.int32).tobytes()
    assert br.beta_q(0.15) == 154 and br.beta_q(2.4) <= br.OD_MAX


def test_int32_bounds_of_the_rule():
    assert 2466 ** 2 == 6081156
    assert 16 * 2466 ** 2 < 2 ** 31                                  # an item of 16 pixels fits int32
    assert 128 * 16 * 2466 ** 2 > 2 ** 32                            # a lane's 128 items of a work unit do not: 64-bit lane sums
    assert 2466 * 1024 * 3 * 256 == 1939341312 < 2 ** 31            # |256 p2| at the corner of the allowed planes
    assert 2466 * 1025 * 3 * 256 < 2 ** 31 < 2466 * 1134 * 3 * 256   # the refusal of |eq_c| > 1024 has room; 1134 would not
    corner = np.full((1, 3), 2466, np.int64)
    for signs in ((1, 1, 1), (-1, -1, -1), (1, -1, 1)):
        eq2 = np.array(signs) * 1024
        assert abs(int(256 * (corner @ eq2)[0])) < 2 ** 31
    assert 2 * 2466 * 1024 * 3 < 2 ** 31                             # p1 + |p2|


@pytest.mark.parametrize("which", ["estimated plane", "hand-made plane"])
def test_direction_bin_range_over_every_pixel(which):
    """k in -256 .. 255 for all 256^3 bytes: direction_bins asserts the range and the 2^31 bound; here every bin of both halves is hit"""
    eq1, eq2 = br.plane(passes(TRUE[0], 0.20)[0])[:2] if which == "estimated plane" else HAND_PLANE
    t = br.odq()
    g, b = np.meshgrid(t, t, indexing="ij")
    seen, outside = np.zeros(512, bool), 0
    for r in range(256):
        o = np.stack([np.full(g.size, t[r]), g.ravel(), b.ravel()], 1)
        k, out = br.direction_bins(o, eq1, eq2)
        seen[np.unique(k) + 256] = True
        outside += out
    assert seen[256:].any() and seen[:256].any()
    if which == "hand-made plane":
        assert outside > 1 and seen[0]                               # p1 <= 0 beyond the white pixel; k == -256 is reached
    else:
        assert outside == 1                                          # the white pixel alone: p1 == 0


def test_the_division_is_a_floor():
    eq1, eq2 = HAND_PLANE
    o = np.array([[1000, 500, 200]], np.int64)
    p1, p2 = int((o @ eq1.astype(np.int64))[0]), int((o @ eq2.astype(np.int64))[0])
    assert p1 > 0 and p2 < 0 and (256 * p2) % (p1 - p2) != 0
    k, _ = br.direction_bins(o, eq1, eq2)
    trunc = -((256 * -p2) // (p1 - p2))                              # C's division rounds towards zero
    assert int(k[0]) == (256 * p2) // (p1 - p2) == trunc - 1 == -math.ceil(256 * -p2 / (p1 - p2))
    up = np.array([[200, 500, 1000]], np.int64)                      # p2 > 0: floor and truncation agree
    q1, q2 = int((up @ eq1.astype(np.int64))[0]), int((up @ eq2.astype(np.int64))[0])
    assert q1 > 0 and q2 > 0 and int(br.direction_bins(up, eq1, eq2)[0][0]) == (256 * q2) // (q1 + q2)


# ---- 2. the host half against the reference, and recovery --------------------------------------------------------------------------------
@pytest.mark.parametrize("share", [0.05, 0.20])
@pytest.mark.parametrize("true", TRUE, ids=["vectors A", "vectors B"])
def test_recovery_on_synthetic_slides(true, share):
    M = sref.basis(*true)
    m, h = passes(true, share)
    assert m[0] == 384 * 576 and 0 < m[1] < m[0] and h[513] == m[1] == h[:513].sum()
    for alpha in (1.0, 0.1):
        want = br.vectors(h, *br.plane(m)[:2], alpha)
        got = product(true, share, alpha)
        assert np.array_equal(got.plane[0], br.plane(m)[0]) and np.array_equal(got.plane[1], br.plane(m)[1])
        assert got.eigenvalues == tuple(br.plane(m)[2]) and got.eigenvalues[0] >= got.eigenvalues[1] > 0
        assert np.array_equal(got.vectors, want["vectors"]) and got.angle_to_prior == pytest.approx(want["angle_to_prior"], rel=1e-9)
        assert got.fell_back == want["fell_back"] == (False, False)
        assert np.array_equal(got.basis.M, br.basis_of(want["vectors"])) and np.array_equal(got.basis.M[:2], got.vectors)
        assert (got.n_tissue, got.n_selected, got.outside, got.alpha, got.beta) == (m[0], m[1], h[512], alpha, 154 / 1024)
        for s in (0, 1):
            err, prior = br.angle(got.vectors[s], M[s]), br.angle(H_DAB.M[s], M[s])
            print(f"share {share} alpha {alpha} stain {s}: {err:.2f} degrees off, the prior {prior:.2f}")
            assert err < prior                                       # closer to the truth than the fixed basis: no constant


def test_true_vectors_equal_to_the_prior_do_not_fall_back():
    for share in (0.05, 0.20):
        for alpha in (1.0, 0.1):
            got = product((sref.HEMATOXYLIN, sref.DAB), share, alpha)
            assert got.fell_back == (False, False) and max(got.angle_to_prior) < br.half_angle()


def test_guard_catches_the_sparse_dab_slide():
    """0.4 % DAB with alpha = 1: the extreme on the DAB side is not DAB (the limit the docstring states)"""
    true = (sref.HEMATOXYLIN, sref.DAB)
    got = product(true, 0.004)
    assert 18.5 < br.half_angle() < 18.7
    assert got.fell_back == (False, True) and got.angle_to_prior[1] > br.half_angle()
    assert np.array_equal(got.basis.M[1], H_DAB.M[1]) and not np.array_equal(got.basis.M[0], H_DAB.M[0])
    raw = product(true, 0.004, max_angle=None)                       # without the guard: the raw vector
    m, h = passes(true, 0.004)
    assert raw.fell_back == (False, False) and np.array_equal(raw.vectors, br.vectors(h, *br.plane(m)[:2], 1.0, max_angle=None)["raw"])
    assert raw.angle_to_prior == got.angle_to_prior and np.array_equal(raw.vectors[0], got.vectors[0])
    low = product(true, 0.004, alpha=0.1)                            # the caller lowers alpha
    print(f"0.4 % DAB: alpha 1 lands {raw.angle_to_prior[1]:.1f} degrees off, alpha 0.1 {low.angle_to_prior[1]:.1f}")
    assert low.fell_back == (False, False) and low.angle_to_prior[1] < raw.angle_to_prior[1]


def test_assignment_follows_the_prior():
    swapped = StainBasis(H_DAB.M[1], H_DAB.M[0])
    a, b = product(TRUE[0], 0.20), product(TRUE[0], 0.20, prior=swapped)
    assert np.array_equal(a.vectors[0], b.vectors[1]) and np.array_equal(a.vectors[1], b.vectors[0])
    assert a.angle_to_prior == pytest.approx(b.angle_to_prior[::-1], rel=1e-9) and b.fell_back == (False, False)


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_raise_before_any_launch():
    r = slide(TRUE[0], 0.20)
    for kw in ({"alpha": 0.0}, {"alpha": 50.0}, {"alpha": -1.0}, {"alpha": math.nan}, {"beta": -0.01}, {"beta": 2.41}, {"beta": math.nan},
               {"prior": "H_DAB"}, {"prior": H_DAB.M}, {"max_angle": 0.0}, {"max_angle": 90.5}, {"max_angle": math.nan}, {"max_angle": True},
               {"bg_level": 257}, {"probe_stride": 0}):
        with pytest.raises(ValueError):
            wsi.estimate_basis(r, **kw)
    with pytest.raises(ValueError):
        wsi.estimate_basis(r.astype(np.float32))
    assert wsi._check_basis_args(0.15, 1.0, H_DAB, "half") == (154, 1.0, pytest.approx(br.half_angle(), rel=1e-12))
    assert wsi._check_basis_args(2.4, 49.9, H_DAB, None) == (2458, 49.9, None)
    assert wsi._check_basis_args(0.0, 0.1, H_DAB, 90) == (0, 0.1, 90.0)


def test_slides_without_a_plane_are_refused():
    glass = np.full((32, 48, 3), 240, np.uint8)                      # no tissue, no selected pixel
    pale = np.full((32, 48, 3), 200, np.uint8)                       # tissue, nothing reaches beta
    one = np.empty((32, 48, 3), np.uint8)
    one[:] = (150, 90, 60)                                           # selected, one colour: no plane
    for r, n_t, n_s in ((glass, 0, 0), (pale, 32 * 48, 0), (one, 32 * 48, 32 * 48)):
        m = br.moments(r, 1, 220, 154)
        assert (m[0], m[1]) == (n_t, n_s)
        with pytest.raises(ValueError):
            br.plane(m)
        with pytest.raises(ValueError):
            wsi.basis_plane(m)
        with pytest.raises(ValueError):
            StainEstimate(m, np.zeros(514, np.int64), 1.0, 154, H_DAB, None)
    with pytest.raises(ValueError):
        wsi.basis_vectors(np.zeros(512, np.int64), (700, -650, 300), (-600, 250, 760))


def test_without_a_device_the_library_error_is_raised():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.AyError):
        wsi.estimate_basis(slide(TRUE[0], 0.20))


# ---- 4. remix ------------------------------------------------------------------------------------------------------------------------------
def hist_of(a, b):
    h = np.zeros((2, 512), np.int64)
    for row, d in ((0, a), (1, b)):
        for k, v in d.items():
            h[row, k] = v
    return h


def test_remix_tables():
    b, other = StainBasis(*TRUE[0]), StainBasis(*TRUE[1])
    g = (1.3, 0.7)
    assert bytes(wsi.stain_tables(b, g)) == bytes(wsi.stain_tables(b, g, target_basis=b)) == bytes(wsi.stain_tables(b, g, None))
    got, want = wsi.stain_tables(b, g, target_basis=other), br.remix_tables(b.M, g, other.M)
    exact = np.linalg.inv(b.M) @ np.diag([1.3, 0.7, 1.0]) @ other.M                       # the float64 product, rounded once
    assert np.asarray(got.A, np.float32).tobytes() == exact.reshape(-1).astype(np.float32).tobytes() == want["A"].tobytes()
    assert bytes(got) == b"".join(want[k].tobytes() for k in ("od", "D", "A", "T"))
    assert np.asarray(got.D, np.float32).tobytes() == sref.tables(g, b.M)["D"].tobytes()  # D stays the source's
    assert np.asarray(got.A, np.float32).tobytes() != np.asarray(wsi.stain_tables(b, g).A, np.float32).tobytes()


def test_stain_map_remix():
    b, other = StainBasis(*TRUE[0]), StainBasis(*TRUE[1])
    s = StainStats(hist_of({63: 10}, {31: 10}), 10, b)               # strengths (1.0, 0.5)
    t = StainStats(hist_of({127: 10}, {15: 10}), 10, other)          # strengths (2.0, 0.25)
    with pytest.raises(ValueError, match="source and target statistics were made on different bases"):
        StainMap(s, t)                                               # remix=False: as before
    with pytest.raises(ValueError):
        StainMap(s, (1.0, 1.0), target_basis=other)                  # target_basis needs remix=True
    with pytest.raises(ValueError):
        StainMap(s, (1.0, 1.0), remix=True, target_basis=other.M)
    with pytest.raises(ValueError):
        StainMap(s, t, remix=True, target_basis=b)                   # not the target statistics' basis
    m = StainMap(s, t, remix=True)
    assert m.gains == (2.0, 0.5) and m.basis == b and m.target_basis == other and m.target == (2.0, 0.25)
    assert bytes(m.tables) == bytes(wsi.stain_tables(b, (2.0, 0.5), other))
    pair = StainMap(s, (2.0, 0.25), remix=True, target_basis=other)
    assert bytes(pair.tables) == bytes(m.tables) and pair.target_basis == other
    same = StainStats(t.hist, 10, b)
    plain = StainMap(s, same)
    assert plain.target_basis == b and StainMap.identity(b).target_basis == b
    for again in (StainMap(s, same, remix=True), StainMap(s, (2.0, 0.25), remix=True), StainMap(s, (2.0, 0.25), remix=True, target_basis=b)):
        assert bytes(again.tables) == bytes(plain.tables) and again.gains == plain.gains and again.target_basis == b
    assert bytes(StainMap(s, (1.3, 0.35)).tables) == b"".join(sref.tables((1.3, 0.7), b.M)[k].tobytes() for k in ("od", "D", "A", "T"))


# ---- 5. normalisation through each slide's own basis -------------------------------------------------------------------------------------
def write_gap(values):
    """the three figures into profiles/stain_basis.txt, next to whatever scripts/bench_stain_basis.py wrote there"""
    path = os.path.join(REPO, "profiles", "stain_basis.txt")
    kept = [ln for ln in (open(path).read().splitlines() if os.path.exists(path) else []) if not ln.startswith("normalisation gap")]
    lines = [f"normalisation gap, mean |byte difference| to slide A over the tissue: {name} {v:.4f}" for name, v in values]
    try:
        with open(path, "w") as f:
            f.write("\n".join(kept + lines) + "\n")
    except OSError:
        pass                                                         # a read-only checkout: the figures are printed


def test_normalisation_closes_the_gap():
    """slide B: the concentration maps of slide A, other vectors, other strengths.  B mapped to A through each slide's own estimated
    basis (estimate -> statistics -> remix map -> apply, all by the restatements) is closer to A than raw B, and closer than B mapped on
    the fixed H_DAB basis.  The assertion is the ordering."""
    A, B = slide(TRUE[0], 0.20), slide(TRUE[1], 0.20, strength=(0.8, 1.25))
    y0, y1, x0, x1 = br.concentration_maps(512, 768, 0.20, 5)[2]
    gap = lambda img: float(np.abs(img[y0:y1, x0:x1].astype(np.int64) - A[y0:y1, x0:x1].astype(np.int64)).mean())

    def strengths(r, M):
        h = sref.hist(r, 1, 220, sref.tables(M=M))
        return sref.strength(h[:1024].reshape(2, 512), int(h[1024]), 99.0)

    fixed = sref.apply(B, 1, sref.tables(sref.gains(strengths(B, br.H_DAB), strengths(A, br.H_DAB))))
    ea, eb = br.estimate(A), br.estimate(B)
    assert ea["fell_back"] == eb["fell_back"] == (False, False)
    g = sref.gains(strengths(B, eb["M"]), strengths(A, ea["M"]))
    remixed = sref.to_u8(sref.map_pixels(B, br.remix_tables(eb["M"], g, ea["M"])))
    values = (("raw slide B", gap(B)), ("H_DAB map", gap(fixed)), ("estimated bases, remix map", gap(remixed)))
    for name, v in values:
        print(f"{name}: {v:.4f}")
    write_gap(values)
    assert values[2][1] < values[1][1] and values[2][1] < values[0][1]
    # the product's map from the same statistics has the restatement's tables
    sa = StainStats(sref.hist(A, 1, 220, sref.tables(M=ea["M"]))[:1024].reshape(2, 512), 384 * 576, StainBasis(*ea["vectors"]))
    sb = StainStats(sref.hist(B, 1, 220, sref.tables(M=eb["M"]))[:1024].reshape(2, 512), 384 * 576, StainBasis(*eb["vectors"]))
    m = StainMap(sb, sa, remix=True)
    assert m.gains == g and bytes(m.tables) == b"".join(br.remix_tables(eb["M"], g, ea["M"])[k].tobytes() for k in ("od", "D", "A", "T"))
