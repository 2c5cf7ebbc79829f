"""The conditions tests/test_gpu_small_kernels.py rests on, asserted on tests/small_kernels_reference.py alone (no GPU, nothing
compiled): the rounding sweeps really are round-to-nearest-even on torch-CPU, every case has a finite E (its bar is printed), the
extreme logits fall into the classes the GPU test treats, every match case exercises the mechanism it names, and the 0.5-IoU boxes
give 0.5f."""
import numpy as np
import pytest
import torch

import small_kernels_reference as skr
from oracle import boxes_oracle as bo

F32, F64 = np.float32, np.float64


def _torch_bits(u32, tdt):
    return torch.from_numpy(np.asarray(u32, np.uint32).view(np.int32).copy()).view(torch.float32).to(tdt).view(torch.int16).numpy().view(np.uint16)


# ------------------------------------------------------------------------------------------------ rounding sweeps
def test_bf16_sweep_is_round_to_nearest_even_on_torch_cpu():
    u = skr.bf16_sweep()
    assert u.size == 393216 and np.unique(u).size == u.size
    got, want = _torch_bits(u, torch.bfloat16), skr.bf16_rne_bits(u)
    nan = skr.is_nan32(u)
    assert np.array_equal(got[~nan], want[~nan])
    assert bool(((got[nan] & 0x7FFF) > 0x7F80).all())                     # NaNs stay NaN
    # the sweep holds ties in both directions, values just beside a tie, and carries into the exponent and into infinity
    tie = (u & 0xFFFF) == 0x8000
    assert np.array_equal(want[tie & ~nan] & 1, np.zeros(int((tie & ~nan).sum()), np.uint16))
    assert int(((want & 0x7FFF) == 0x7F80).sum() - ((u & 0x7FFFFFFF) == 0x7F800000).sum()) > 0   # finite values that round to infinity


def test_f16_sweep_is_round_to_nearest_even_on_torch_cpu():
    u = skr.f16_sweep()
    assert u.size == 190464 and not skr.is_nan32(u).any()
    got, want = _torch_bits(u, torch.float16), skr.f16_rne_bits(u)
    assert np.array_equal(got, want)
    assert int(((want & 0x7FFF) == 0x7C00).sum()) == 4                     # 65520 and its upper neighbour, both signs
    assert int(((want & 0x7C00) == 0).sum()) > 6000                        # the subnormal range and zero
    # every midpoint is a tie: it goes to the even neighbour, the values beside it to their own side
    mid = u.view(F32)[1::3][:0x7C00]
    assert np.array_equal(want[1::3][:0x7C00] & 1, np.zeros(0x7C00, np.uint16))
    assert np.array_equal(want[0::3][:0x7C00], np.arange(0x7C00, dtype=np.uint16)) and mid.size == 0x7C00
    assert np.array_equal(want[2::3][:0x7C00], np.arange(1, 0x7C01, dtype=np.uint16))
    # the device rule differs from torch in exactly the four saturating values
    dev = skr.half_bits_device_rule(u, got)
    diff = np.flatnonzero(dev != got)
    assert diff.size == 4 and set(dev[diff].tolist()) == {0x7BFF, 0xFBFF}
    # random values and NaN / infinity through the integer rule too
    r = skr.rng(3).normal(0, 1, 100000).astype(F32) * np.exp2(skr.rng(4).integers(-30, 20, 100000)).astype(F32)
    assert np.array_equal(_torch_bits(r.view(np.uint32), torch.float16), skr.f16_rne_bits(r.view(np.uint32)))
    inf = np.asarray([np.inf, -np.inf], F32).view(np.uint32)
    assert skr.f16_rne_bits(inf).tolist() == [0x7C00, 0xFC00] and np.array_equal(skr.half_bits_device_rule(inf, skr.f16_rne_bits(inf)), skr.f16_rne_bits(inf))


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("case", skr.DECODE_CASES, ids=skr.decode_id)
def test_decode_cases_have_finite_E(case):
    A, C, G, B, img = case
    head, anchors = skr.decode_head(case), skr.anchors_of(A)
    ref, twin = skr.decode_f64(head, anchors, C, img), skr.decode_twin(head, anchors, C, img)
    assert ref.shape == twin.shape == (B, A * G * G, 5 + C) and np.isfinite(ref).all() and np.isfinite(twin).all()
    for name, E in skr.decode_errors(twin, ref, A, G, img).items():
        print("decode %-22s %-4s E %9.2e  bar %9.2e" % (skr.decode_id(case), name, E, skr.bar(E)))
        assert np.isfinite(E) and E < 2.0 ** -20                           # a few ulp of float32, as measured: 2.6 ulp at sigma = 3
    if float(img) / G == int(img / G):                                     # the oracle's decode is this twin (its anchors go through Python floats)
        assert np.array_equal(twin, bo.decode(head, anchors, C, img)[0])


def test_blocked_head_holds_the_head_and_nan_pads():
    head = skr.decode_head((3, 2, 8, 1, 256))
    hb = skr.blocked_head(head)
    assert hb.shape == (1, 2, 8, 8, 16)
    back = hb.transpose(0, 1, 4, 2, 3).reshape(1, 32, 8, 8)
    assert np.array_equal(back[:, :21], head) and np.isnan(back[:, 21:]).all()


def test_extreme_table_classes():
    """the float64 classes of the planted logits: what the GPU test asserts of each rests on these"""
    A, C, G, B, img = skr.EXTREME_CASE
    base, planted, plan = skr.extreme_head()
    assert len(plan) == (5 + C) * len(skr.EXTREME) <= A * G * G and len({p[0] for p in plan}) == len(plan)
    assert int((base.view(np.uint32) != planted.view(np.uint32)).sum()) == len(plan)
    cls = {(k, v if v == v else "nan", np.signbit(v)): c for _, k, v, c, _ in skr.extreme_classes(plan, skr.anchors_of(A), img, G)}
    key = lambda k, v: (k, float(F32(v)), bool(np.signbit(F32(v))))
    for k in (2, 3):                                                       # w, h
        assert [cls[key(k, v)] for v in (87.0, 88.5, 89.0, 104.0, np.inf)] == ["inf"] * 5    # exp(87) = 6.1e37; x anchor >= 10 is beyond FLT_MAX
        assert [cls[key(k, v)] for v in (-88.5, -89.0, -104.0, -np.inf)] == ["tiny"] * 4
        assert [cls[key(k, v)] for v in (0.0, -0.0, 1e-40, -1e-40, -87.0)] == ["normal"] * 5
        assert cls[(k, "nan", False)] == "nan"
    for k in (0, 1, 4, 5, 6):                                              # sigmoids
        assert [cls[key(k, v)] for v in (87.0, 88.5, 89.0, 104.0, np.inf)] == ["one"] * 5
        assert [cls[key(k, v)] for v in (-104.0, -np.inf)] == ["zero"] * 2
        assert [cls[key(k, v)] for v in (-88.5, -89.0)] == ["tiny"] * 2
        assert [cls[key(k, v)] for v in (0.0, -0.0, 1e-40, -1e-40, -87.0)] == ["normal"] * 5
        assert cls[(k, "nan", False)] == "nan"
    # the twin itself: non-finite only where planted so, and the unplanted slots of every row are the base decode
    anchors = skr.anchors_of(A)
    t0, t1 = skr.decode_twin(base, anchors, C, img), skr.decode_twin(planted, anchors, C, img)
    mask = np.ones(t0.shape, bool)
    for cell, k, _ in plan:
        mask[0, cell, k] = False
    assert np.array_equal(t0[mask], t1[mask]) and np.isfinite(t0).all()


def test_fused_extreme_plan_covers_every_channel_and_value():
    A, C, G, B, img = skr.FUSED_EXTREME_CASE
    K = 5 + C
    base = skr.rng(91).normal(0, 2, A * K).astype(F32)
    seen = set()
    for j in range(len(skr.EXTREME)):
        for k in range(K):
            logits, plan = skr.fused_extreme_logits(base, A, K, G, j, k)
            assert int((logits.view(np.uint32) != base.view(np.uint32)).sum()) == A and len(plan) == A * G * G
            seen |= {(cell // (G * G), kk, repr(v)) for cell, kk, v in plan}
            assert {c for *_, c, _ in skr.extreme_classes(plan, skr.anchors_of(A), img, G)} <= {"nan", "inf", "tiny", "one", "zero", "normal"}
    assert len(seen) == A * K * len(skr.EXTREME)


# ------------------------------------------------------------------------------------------------ box math
def test_half_iou_boxes_give_exactly_half():
    a, b = skr.HALF_IOU_PAIR
    v = bo.bbox_iou([a], [b])
    assert v.dtype == F32 and v[0] == F32(0.5) and float(skr.iou_f64([a], [b])[0]) == 50.0 / (100.0 + 1e-16)
    below = bo.bbox_iou([skr.BELOW_HALF_IOU_PAIR[0]], [skr.BELOW_HALF_IOU_PAIR[1]])
    assert F32(0.5) - F32(1e-6) < below[0] < F32(0.5)


def test_box_classes_and_giou_E():
    cls = skr.box_classes()
    for name, (a, b) in cls.items():
        assert a.dtype == b.dtype == F32 and a.shape == b.shape and a.shape[1] == 4
        twin, ref = skr.giou_twin(a, b), skr.giou_f64(a, b)
        assert np.isfinite(twin).all() and np.isfinite(ref).all()
        E = float(np.abs(twin.astype(F64) - ref).max())                    # scale 1: GIoU lies in [-1, 1]
        print("giou %-16s E %9.2e  bar %9.2e" % (name, E, skr.bar(E)))
        assert np.isfinite(E)
        Ei = float(np.abs(skr.iou_twin(a, b).astype(F64) - skr.iou_f64(a, b)).max())
        assert Ei < 1e-5
    assert (skr.iou_twin(*cls["touching"]) > 0).all() and (skr.iou_twin(*cls["disjoint"]) == 0).all()
    w = np.minimum(cls["touching"][0][:, 2], cls["touching"][1][:, 2]) - np.maximum(cls["touching"][0][:, 0], cls["touching"][1][:, 0]) + 1
    assert (w == 1).all()                                                  # inter width 1 under the +1 rule
    assert (skr.giou_twin(*cls["identical"]) == 1).all()
    # two zero-area boxes: the 1e-16 terms decide (0 / 1e-16 - 0 / 1e-16 = 0 at one point; -1 + ... between two distinct points)
    assert (skr.giou_twin(*cls["zero_same_point"]) == 0).all()
    a, b = cls["zero_both"]
    both = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]) == 0) & ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) == 0)
    assert both.all() and (skr.giou_twin(a, b) <= 0).all()
    assert float(cls["slide_2^20"][0].max()) > 2.0 ** 20 and float(cls["slide_2^17"][0].max()) > 2.0 ** 17


def test_xywh_round_trip_inputs_are_float32():
    a, _ = skr.all_boxes()
    c = skr.to_cxcywh(a)
    assert c.dtype == F32 and np.isfinite(skr.xywh2xyxy_twin(c)).all()


# ------------------------------------------------------------------------------------------------ match
@pytest.mark.parametrize("name", sorted(skr.match_cases()))
def test_match_cases_are_not_idle(name):
    c = skr.match_cases()[name]
    tp, overflow, ev = skr.match_batch(c["rows"], c["count"], c["targets"], c["thr"])
    print("match %-14s tp %d of %d rows, events %s" % (name, int(tp.sum()), int(np.minimum(c["count"], c["rows"].shape[1]).sum()), ev))
    assert overflow == 0
    for need in c["needs"]:
        assert ev[need] >= 1, (name, need, ev)
    # the instrumented walk is the oracle's
    B, max_det = c["rows"].shape[:2]
    outs = [c["rows"][b, :min(int(c["count"][b]), max_det)] for b in range(B)]
    ref = bo.get_batch_statistics([o if len(o) else None for o in outs], c["targets"], c["thr"])
    present = [b for b in range(B) if len(outs[b])]
    assert len(ref) == len(present)
    for b, m in zip(present, ref):
        assert np.array_equal(m[0], tp[b, :len(outs[b])]), (name, b)
    if name not in ("empty_sides",):
        assert tp.sum() >= 1                                               # something matches
    if name == "absent_label":
        assert tp[0].tolist() == [0, 0, 0, 0, 1, 1, 1, 1]                  # label 9 claims nothing at IoU 1: the same boxes match afterwards
    if name == "early_stop":
        assert tp[0].tolist() == [1, 1, 1, 0, 0, 0, 0, 0, 0]
    if name == "duplicates":
        assert tp[0].tolist() == [1, 0, 0, 0, 0, 1, 1]                     # the first of four equal targets wins, every time
    if name == "threshold":
        assert tp[0].tolist() == [0, 1, 0, 0]
    if name == "nan_box":
        assert tp[0].tolist() == [1, 0, 0, 1, 1, 1, 1, 0]
    if name == "count_clamp":
        assert int(c["count"][0]) > max_det and tp[1, 5:].sum() == 0
    if name == "empty_sides":
        assert tp[0].sum() == 0 and tp[1].sum() == 0 and tp[2].sum() >= 1 and (c["targets"][:, 0] >= B).sum() == 24


@pytest.mark.parametrize("n", [2048, 2049])
def test_match_cap_cases(n):
    c = skr.cap_case(n)
    tp, overflow, ev = skr.match_batch(c["rows"], c["count"], c["targets"], c["thr"])
    assert overflow == int(n > skr.MAX_T) and int(tp.sum()) == skr.MAX_T
    if n > skr.MAX_T:                                                      # the detection of the dropped target is the one row without a TP, unless the early stop came first
        lost = np.flatnonzero(tp[0, :n] == 0)
        assert lost.size == 1


# ------------------------------------------------------------------------------------------------ BatchNorm, fold_bn
@pytest.mark.parametrize("kind", ["random", "cancel", "const"])
@pytest.mark.parametrize("shape", skr.BN_SHAPES, ids=skr.bn_id)
def test_bn_cases_have_finite_E(shape, kind):
    z, gamma, beta, rm, rv, dy = skr.bn_inputs(shape, kind)
    for leaky in (0, 1):
        for mom in skr.BN_MOMENTA:
            ref = skr.bn_fwd_f64(z, gamma, beta, rm, rv, mom, skr.BN_EPS, leaky)
            twin = skr.bn_fwd_twin(z, gamma, beta, rm, rv, mom, skr.BN_EPS, leaky)
            for k in ("y", "save_mean", "save_invstd", "running_mean", "running_var"):
                E = skr.channel_errors(twin[k], ref[k], ref["scale"][k])
                assert np.isfinite(E).all(), (k, E)
                if mom == 0.1:
                    print("bn %-18s %-6s leaky %d %-12s E %9.2e  bar %9.2e" % (skr.bn_id(shape), kind, leaky, k, E.max(), skr.bar(E.max())))
            assert np.array_equal(twin["y"], skr.bn_apply_twin(z, twin["save_mean"], twin["save_invstd"], gamma, beta, leaky))
            if shape[0] * shape[2] == 1:                                   # n = 1: the biased variance (0) goes into running_var
                assert np.array_equal(twin["running_var"], (F32(1) - F32(mom)) * rv + F32(mom) * F32(0))
            if kind == "const":
                assert np.array_equal(twin["save_invstd"], np.full(shape[1], F32(1.0 / np.sqrt(F64(F32(skr.BN_EPS)))), F32))
            if kind == "cancel" and shape[0] * shape[2] > 1000:            # the variance survives the mean of 1e4: relative to float64
                assert skr.channel_errors(twin["save_invstd"], ref["save_invstd"], ref["save_invstd"]).max() < 1e-6
        twin = skr.bn_fwd_twin(z, gamma, beta, rm, rv, 0.1, skr.BN_EPS, leaky)
        rb = skr.bn_bwd_f64(dy, twin["y"], z, gamma, twin["save_mean"], twin["save_invstd"], leaky)
        tb = skr.bn_bwd_twin(dy, twin["y"], z, gamma, twin["save_mean"], twin["save_invstd"], leaky)
        for k in ("dz", "dgamma", "dbeta"):
            E = skr.channel_errors(tb[k], rb[k], rb["scale"][k])
            assert np.isfinite(E).all(), (k, E)
            print("bn %-18s %-6s leaky %d %-12s E %9.2e  bar %9.2e" % (skr.bn_id(shape), kind, leaky, k, E.max(), skr.bar(E.max())))


def test_bn_zero_y_case_reaches_the_mask_edge():
    for shape in ((1, 5, 256), (4, 33, 64 * 64)):
        z, gamma, beta, rm, rv, dy = skr.bn_inputs(shape, "zero_y")
        twin = skr.bn_fwd_twin(z, gamma, beta, rm, rv, 0.1, skr.BN_EPS, 1)
        assert (twin["save_mean"] == 0).all() and (beta == 0).all()
        zero = z == 0
        assert zero.mean() == 0.5 and (twin["y"][zero] == 0).all() and (twin["y"][~zero] != 0).all()
        # with the slope of y > 0 at those pixels the gradient would differ far beyond the bar
        rb = skr.bn_bwd_f64(dy, twin["y"], z, gamma, twin["save_mean"], twin["save_invstd"], 1)
        wrong = skr.bn_bwd_f64(dy, np.where(zero, F32(1), twin["y"]), z, gamma, twin["save_mean"], twin["save_invstd"], 1)
        assert skr.channel_errors(wrong["dz"], rb["dz"], rb["scale"]["dz"]).min() > 1e-3


def test_fold_bn_twin_forms():
    r = skr.rng(2)
    n = 257
    g, b, m, v, bias = (r.normal(0, 1, n).astype(F32) for _ in range(5))
    v = np.abs(v)
    s, t = skr.fold_bn_twin(g, b, m, v, None, 1e-5, n, n + 300)
    assert s.shape == (n + 300,) and not s[n:].any() and not t[n:].any() and not np.signbit(s[n:]).any()
    ref = g.astype(F64) / np.sqrt(v.astype(F64) + F64(F32(1e-5)))
    assert np.abs(s[:n] - ref).max() <= 2.0 ** -22 * np.abs(ref).max()
    s, t = skr.fold_bn_twin(None, None, None, None, bias, 0.0, n, n)
    assert (s == 1).all() and np.array_equal(t, bias)
    s, t = skr.fold_bn_twin(None, None, None, None, None, 0.0, n, 288)
    assert (s[:n] == 1).all() and not t.any() and not s[n:].any()


# ------------------------------------------------------------------------------------------------ layout, plumbing
def test_blocked_round_trip_and_plumbing_twins():
    for shape in skr.LAYOUT_SHAPES:
        x = skr.rng(sum(shape)).normal(0, 1, shape).astype(F32)
        xb = skr.to_blocked(x)
        assert xb.shape == (shape[0], (shape[1] + 15) // 16, shape[2], shape[3], 16)
        assert np.array_equal(skr.from_blocked(xb, shape[1]), x)
        if shape[1] % 16:
            assert not xb[:, -1, :, :, shape[1] % 16:].any()
    src = skr.rng(1).normal(0, 1, (3, 4, 3, 5)).astype(F32)
    out = skr.copy_channels_twin(src, np.full((3, 9, 6, 10), 7, F32), 2, 1)
    assert np.array_equal(out[:, 2:6, 1::2, 1::2], src) and (out[:, :2] == 7).all() and (out[:, 6:] == 7).all()
    acc = skr.slice_accumulate_twin(out, np.zeros_like(src), 2, 1)
    assert np.array_equal(acc, 4 * src)
    s1 = np.arange(2 * 1 * 3 * 5 * 16, dtype=np.uint16).reshape(2, 1, 3, 5, 16)
    cat = skr.concat_upsample_twin(s1, 1, None)
    assert cat.shape == (2, 1, 6, 10, 16) and np.array_equal(cat[:, :, 1::2, 0::2], s1)
