"""CPU: the conditions tests/test_gpu_yolo_loss.py rests on, asserted on the reference (tests/yolo_loss_reference.py) alone -- its
values against the float32 path the suite already trusts and against the GIoU known answers, the margins that make integer
comparisons of counts legitimate, the edges `edges` claims to have, and that the cases can tell each deliberate error from the truth."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import yolo_loss_reference as R
from oracle import boxes_oracle as bo
from oracle.darknet_oracle import giou_cxcywh

F32 = np.float32
BOX_LOSSES = ["mse", "giou"]


def _float32_path(c, box_loss):
    """loss and d loss / d head exactly as test_yolo_loss_kernel_duplicates_and_grad / test_yolo_giou_loss_kernel_vs_autograd
    compose them: oracle decode + build_targets, torch float32 autograd with mean reductions"""
    B, A, Cc, G = c.B, c.A, c.C, c.G
    tg = R.filter_dropped(c.targets, B, Cc, G)
    h = torch.from_numpy(c.head).clone().requires_grad_(True)
    p = h.view(B, A, 5 + Cc, G, G).permute(0, 1, 3, 4, 2)
    sx, sy, w, hh = torch.sigmoid(p[..., 0]), torch.sigmoid(p[..., 1]), p[..., 2], p[..., 3]
    conf, cls = torch.sigmoid(p[..., 4]), torch.sigmoid(p[..., 5:])
    _, boxes, aux = bo.decode(c.head, c.anchors, Cc, c.img_dim)
    bt = bo.build_targets(boxes, aux["cls"], tg, aux["scaled_anchors"], c.ignore_thres)
    iou_scores, class_mask, obj, noobj, tx, ty, tw, th, tcls, tconf = [torch.from_numpy(np.ascontiguousarray(v)) for v in bt]
    if box_loss == "mse":
        box = F.mse_loss(sx[obj], tx[obj]) + F.mse_loss(sy[obj], ty[obj]) + F.mse_loss(w[obj], tw[obj]) + F.mse_loss(hh[obj], th[obj])
    else:
        sa = torch.from_numpy(np.asarray(aux["scaled_anchors"], F32))
        gi = torch.arange(G, dtype=torch.float32).view(1, 1, 1, G).expand(B, A, G, G)[obj]
        gj = torch.arange(G, dtype=torch.float32).view(1, 1, G, 1).expand(B, A, G, G)[obj]
        aw, ah = sa[:, 0].view(1, A, 1, 1).expand(B, A, G, G)[obj], sa[:, 1].view(1, A, 1, 1).expand(B, A, G, G)[obj]
        pb = torch.stack((sx[obj] + gi, sy[obj] + gj, torch.exp(w[obj]) * aw, torch.exp(hh[obj]) * ah), 1)
        tb = torch.stack((tx[obj] + gi, ty[obj] + gj, torch.exp(tw[obj]) * aw, torch.exp(th[obj]) * ah), 1)
        box = (1.0 - giou_cxcywh(pb, tb)).mean()
    loss = (box + F.binary_cross_entropy(conf[obj], tconf[obj]) + 100 * F.binary_cross_entropy(conf[noobj], tconf[noobj])
            + F.binary_cross_entropy(cls[obj], tcls[obj]))
    loss.backward()
    return float(loss.detach()), h.grad.numpy()


@pytest.mark.parametrize("box_loss", BOX_LOSSES)
@pytest.mark.parametrize("name", ["parts16", "edges", "one_wg"])
def test_reference_agrees_with_the_float32_path(name, box_loss):
    """float64 sums and gradient against the float32 path of today's tests, to 1e-5 (of the loss, of the largest gradient)"""
    c, asg, ref, _, _ = R.reference(name, box_loss)
    want, g = _float32_path(c, box_loss)
    s = ref.sums
    got = (s[0] + s[1] + s[2] + s[3]) / s[7] + s[4] / s[7] + 100 * s[5] / s[8] + s[6] / (s[7] * c.C)
    assert abs(got - want) <= 1e-5 * abs(want)
    assert abs(ref.loss - want) <= 1e-5 * abs(want)
    assert np.abs(ref.dhead - g).max() <= 1e-5 * np.abs(g).max()


def test_reference_giou_agrees_with_the_known_answers(golden_dir):
    """every vector of tests/golden/giou_kat.json as the one object cell of a head: boxes scaled by 2^-7 (GIoU does not change) into
    cell (5, 5) of a 16 x 16 grid with one 1 x 1 anchor; slot 0 of the float64 sums is 1 - GIoU"""
    doc = json.load(open(os.path.join(golden_dir, "giou_kat.json")))
    s, off, G = 2.0 ** -7, 5 + 2.0 ** -8, 16
    logit = lambda v: np.log(v / (1 - v))
    for k in doc["cases"]:
        (x1, y1, x2, y2), (X1, Y1, X2, Y2) = k["box1"], k["box2"]
        head = np.zeros((1, 6, G, G), F32)
        head[0, :4, 5, 5] = [logit((x1 + x2) / 2 * s + off - 5), logit((y1 + y2) / 2 * s + off - 5), np.log((x2 - x1) * s), np.log((y2 - y1) * s)]
        tg = np.array([[0, 0, ((X1 + X2) / 2 * s + off) / G, ((Y1 + Y2) / 2 * s + off) / G, (X2 - X1) * s / G, (Y2 - Y1) * s / G]], F32)
        c = R.Case(k["name"], 1, 1, 1, G, [(8, 8)], head, tg)
        asg = R.assign(c)
        assert asg.obj[0, 0, 5, 5] and asg.obj.sum() == 1
        ref = R.loss_reference(c, asg, "giou")
        assert abs(ref.sums[0] - (1 - k["giou"][0] / k["giou"][1])) <= 2e-6, k["name"]
        assert ref.sums[1] == ref.sums[2] == ref.sums[3] == 0


def test_cases_reach_the_paths_they_name():
    wg = {n: R.case(n).workgroups for n in R.CASES}
    assert wg["stride"] == 1024 and R.case("stride").cells == 294912
    assert (R.case("stride").cells - 1024 * 256) // 256 == 128          # workgroups that take a second sweep
    assert (len(R.case("stride").targets) + 255) // 256 == 3            # yolo_targets_pass1 workgroups
    assert wg["cap_ragged"] == 1020 and R.case("cap_ragged").cells % 256 != 0 and (1020 + 15) // 16 == 64 and 1020 % 64 != 0
    assert (wg["parts17"], wg["parts16"], wg["parts33"], wg["one_wg"]) == (17, 16, 33, 1)
    assert R.case("one_wg").cells < 256 and R.case("empty").targets.shape == (0, 6)
    for n in R.CASES:
        c = R.case(n)
        assert c.head.dtype == F32 and c.targets.dtype == F32 and c.img_dim == 8 * c.G
        assert np.abs(c.head.reshape(c.B, c.A, 5 + c.C, c.G, c.G)[:, :, 2:4]).max() <= 8


@pytest.mark.parametrize("name", ["stride", "cap_ragged", "parts17", "parts16", "parts33", "saturated"])
def test_targets_meet_the_hard_cases(name):
    """every anchor is some target's best; some cell holds two targets (multi-hot where there is more than one class)"""
    c = R.case(name)
    asg = R.assign(c)
    assert sorted(set(asg.ious.argmax(0).tolist())) == list(range(c.A))
    assert asg.obj.sum() < len(asg.tg)
    if c.C > 1:
        assert (asg.tcls.sum(-1) > 1).any()


@pytest.mark.parametrize("name", R.CASES)
def test_decisions_keep_their_margins(name):
    """no float32 decision within 1e-4 of its threshold, so one ulp between the device's expf and NumPy's cannot change a count;
    in `edges` the wh_iou values that are not exactly on the threshold keep the margin too"""
    c = R.case(name)
    m = R.decision_margins(c, R.assign(c))
    assert m["wh_iou_off_thres" if name == "edges" else "wh_iou"] > 1e-4
    assert m["anchor_gap_off_tie" if name == "edges" else "anchor_gap"] > 1e-4      # the best-anchor argmax itself
    assert m["conf"] > 1e-4 and m["iou"] > 1e-4 and m["cls_top2"] > 1e-4, m


def test_filter_dropped_is_the_kernels_rule():
    keep = np.array([[0, 0, .5, .5, .1, .1], [1, 2, 0., 0., .1, .1], [1, 2, 1 - 2.0 ** -10, 1 - 2.0 ** -10, .1, .1]], F32)
    drop = np.array([[2, 0, .5, .5, .1, .1], [-1, 0, .5, .5, .1, .1], [0, 3, .5, .5, .1, .1], [0, -1, .5, .5, .1, .1],
                     [0, 0, 1., .5, .1, .1], [0, 0, .5, 1., .1, .1], [0, 0, -1.5, .5, .1, .1]], F32)
    np.testing.assert_array_equal(R.filter_dropped(np.concatenate([drop[:3], keep, drop[3:]]), 2, 3, 16), keep)
    assert len(R.filter_dropped(np.zeros((0, 6), F32), 2, 3, 16)) == 0
    with pytest.raises(IndexError):        # what the reference does with such a row
        bo.build_targets(np.zeros((2, 3, 16, 16, 4), F32), np.zeros((2, 3, 16, 16, 3), F32), drop[:1], np.ones((3, 2), F32), 0.5)


def test_edges_has_its_edges():
    c = R.case("edges")
    asg = R.assign(c)
    tg, G = asg.tg, c.G
    sa = asg.sa
    np.testing.assert_array_equal(sa, np.array([(2, 2), (2, 2), (4, 2), (1, 1)], F32))
    # dropped rows: dropped by filter_dropped and by nothing else
    np.testing.assert_array_equal(tg, R.edges_targets(dropped=False))
    assert len(c.targets) == len(tg) + 4
    gone = [r for r in c.targets.tolist() if r not in tg.tolist()]
    assert sorted((r[0] == c.B, r[1] == c.C, r[2] == 1.0, r[3] == 1.0) for r in gone) == sorted(
        [(True, False, False, False), (False, True, False, False), (False, False, True, False), (False, False, False, True)])
    # anchor tie, bit for bit; anchor 0 is the object cell
    assert asg.ious[0, 0] == asg.ious[1, 0] == F32(1.0) and asg.ious[:, 0].argmax() == 0
    assert asg.obj[0, 0, 4, 3] and not asg.obj[0, 1, 4, 3]
    # wh_iou == 0.5 in float32 against anchors 0, 1, 3: anchor 0 is best, 1 and 3 stay no-object at 0.5 and are cleared at 0.4999
    assert asg.ious[0, 1] == asg.ious[1, 1] == asg.ious[3, 1] == F32(0.5) and asg.ious[2, 1] < F32(0.5)
    assert asg.obj[0, 0, 2, 8] and asg.noobj[0, 1, 2, 8] and asg.noobj[0, 3, 2, 8] and asg.noobj[0, 2, 2, 8]
    low = R.assign(c, 0.4999)
    assert not low.noobj[0, 1, 2, 8] and not low.noobj[0, 3, 2, 8] and low.noobj[0, 2, 2, 8]
    assert low.noobj.sum() < asg.noobj.sum()
    # cell and image edges
    tx, ty = asg.bt[4], asg.bt[5]
    assert asg.obj[1, 3, 7, 5] and tx[1, 3, 7, 5] == 0.0
    assert asg.obj[1, 3, 3, 0] and tx[1, 3, 3, 0] == 0.0
    assert asg.obj[1, 3, 9, G - 1] and tx[1, 3, 9, G - 1] == F32(1 - 2.0 ** -6)
    assert asg.obj[0, 3, 9, 6] and ty[0, 3, 9, 6] == 0.0
    assert asg.obj[0, 3, 0, 13] and ty[0, 3, 0, 13] == 0.0
    assert asg.obj[0, 3, G - 1, 1] and ty[0, 3, G - 1, 1] == F32(1 - 2.0 ** -6)
    # 64 rows in one (image, anchor, cell): last row wins, tcls all ones, class_mask from the last row's label
    b, a, gj, gi = R.EDGE_CELL
    gi_all, gj_all = (tg[:, 2] * F32(G)).astype(int), (tg[:, 3] * F32(G)).astype(int)
    rows = np.nonzero((tg[:, 0] == b) & (gi_all == gi) & (gj_all == gj) & (asg.ious.argmax(0) == a))[0]
    assert len(rows) == 64 and asg.win[b, a, gj, gi] == rows[-1]
    assert asg.tcls[b, a, gj, gi].tolist() == [1.0, 1.0, 1.0]
    assert sorted(set(tg[rows, 1].tolist())) == [0.0, 1.0, 2.0]
    assert asg.class_mask[b, a, gj, gi] == float(asg.cls[b, a, gj, gi].argmax() == int(tg[rows[-1], 1]))
    assert asg.bt[6][b, a, gj, gi] == np.log(tg[rows[-1], 4] * F32(G) / sa[a, 0] + F32(1e-16), dtype=F32)
    # two targets, one cell, different best anchors
    assert asg.obj[1, 2, 12, 12] and asg.obj[1, 3, 12, 12]
    assert asg.obj.sum() == 11


def test_saturated_logits_cannot_change_side():
    c = R.case("saturated")
    asg = R.assign(c)
    h = c.head.reshape(c.B, c.A, 5 + c.C, c.G, c.G)
    planted = np.zeros(h.shape, bool)
    kinds = set()
    for idx in c.planted:
        planted[idx] = True
        x = F32(h[idx])
        assert abs(x) >= 30
        with np.errstate(over="ignore"):
            p = F32(1) / (F32(1) + np.exp(-x, dtype=F32))
        assert p == 0 or p == 1 or (F32(1) - p) * p < 1e-12
        b, a, ch, gj, gi = idx
        kinds.add(("obj" if asg.obj[b, a, gj, gi] else "noobj" if asg.noobj[b, a, gj, gi] else "ignored", "conf" if ch == 4 else "cls",
                   float(x), float(asg.tcls[b, a, gj, gi, ch - 5]) if ch > 4 else None))
    assert len(c.planted) == 16
    for v in R.PLANTED:
        assert ("obj", "conf", v, None) in kinds and ("noobj", "conf", v, None) in kinds
        assert any(k[:3] == ("obj", "cls", v) for k in kinds)
    assert {k[3] for k in kinds if k[1] == "cls"} == {0.0, 1.0}        # both target values meet a saturated class logit
    rest = np.abs(h[~planted])
    assert not ((rest >= 14) & (rest <= 25)).any() and rest.max() < 14
    # the twin (torch float32 autograd) has exact zeros at the planted logits that saturate to 0 or 1, and the -100 clamps
    _, _, ref, _, _ = R.reference("saturated")
    d = ref.dhead.reshape(h.shape)
    zeros = [idx for idx in c.planted if h[idx] == 30 or abs(h[idx]) == 104]
    assert len(zeros) == 12 and all(d[idx] == 0.0 for idx in zeros)
    assert all(d[idx] != 0.0 for idx in c.planted if h[idx] == -30)
    plain = R.unplanted(c)
    base = R.loss_reference(plain, R.assign(plain), "mse", torch.float32)
    assert ref.sums[5] - base.sums[5] > 190 and ref.sums[4] - base.sums[4] > 120      # 100 + 100 (+30, +104); 100 + 30 (-104, -30)


def _differs(mut, ref, Eg, Es):
    """does `mut` miss the device bars around `ref`?"""
    if any(mut.sums[k] != ref.sums[k] for k in R.COUNT_SLOTS):
        return True
    es = R.sum_errors(mut.sums, ref)
    if any(es[n] > R.bar(Es[n]) for n in es):
        return True
    eg, stray = R.grad_errors(mut.dhead, ref)
    return stray > 0 or any(eg[n] > R.bar(Eg[n]) for n in eg)


@pytest.mark.parametrize("box_loss", BOX_LOSSES)
@pytest.mark.parametrize("name,mutant", [("edges", "ge_thres"), ("edges", "first_writer"), ("stride", "first_writer"),
                                         ("edges", "last_max_anchor"), ("edges", "one_hot"), ("stride", "one_hot"),
                                         ("edges", "no_100"), ("stride", "no_100"), ("empty", "no_100")])
def test_cases_tell_each_mutant_from_the_truth(name, mutant, box_loss):
    c, asg, ref, Eg, Es = R.reference(name, box_loss)
    if mutant == "no_100":
        mut = R.loss_reference(c, asg, box_loss, noobj_factor=1.0)
    else:
        mut = R.loss_reference(c, R.assign(c, mutant=mutant), box_loss)
    assert _differs(mut, ref, Eg, Es)
    assert not _differs(ref, ref, Eg, Es)


def test_twin_stays_within_its_own_bar():
    """the float32 twin is inside the bar it sets (trivially 4x), and the bars are tight: no class above 1e-4 of its scale"""
    for name in R.CASES:
        for box_loss in (BOX_LOSSES if name != "saturated" else ["mse"]):
            _, _, _, Eg, Es = R.reference(name, box_loss)
            assert max(Eg.values()) < 1e-4 and max(Es.values()) < 1e-5, (name, box_loss, Eg, Es)


def test_kernel_tree_sum_is_a_sum():
    rng = np.random.Generator(np.random.PCG64(3))
    for n in (1, 169, 4332, 261075, 294912):
        x = rng.integers(-8, 9, n).astype(F32)          # exact in float32 in any order
        assert R.kernel_tree_sum(x) == float(x.sum(dtype=np.float64))
