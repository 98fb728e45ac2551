"""CPU checks of ``detect_refs.py``: each reference is tied to ``oracle/detection.py`` on ordinary inputs, the lattice claim
(every fp32 width, area, intersection and union of lattice boxes is exact in any order) is checked itself together with the
exact-tie counts that keep the NMS sweep from being vacuous, and a non-transitive suppression chain is checked by hand."""
from fractions import Fraction

import numpy as np
import torch

import detect_refs as DR
from oracle import detection as OD

NMS_SIZES = (63, 64, 65, 127, 128, 129, 700, 4097)


def test_lattice_is_exact_in_fp32_and_holds_exact_ties():
    rng = np.random.RandomState(0)
    b = DR.lattice_boxes(rng, 700)
    q = DR.quarter_units(b)
    assert q.min() >= 0 and q.max() <= 256
    sides = np.concatenate([q[:, 2] - q[:, 0], q[:, 3] - q[:, 1]])
    assert sides.min() == 0 and sides.max() <= 64 and (sides == 0).sum() >= 5
    inter, union = DR.lattice_inter_union(b, b)
    assert inter.max() <= 8192 and union.max() <= 8192
    f = np.float32
    w, h = f(b[:, 2] - b[:, 0]), f(b[:, 3] - b[:, 1])
    area = f(w * h)
    iw = np.maximum(np.minimum(b[:, None, 2], b[None, :, 2]) - np.maximum(b[:, None, 0], b[None, :, 0]), f(0))
    ih = np.maximum(np.minimum(b[:, None, 3], b[None, :, 3]) - np.maximum(b[:, None, 1], b[None, :, 1]), f(0))
    i32 = f(iw * ih)
    assert i32.dtype == np.float32
    assert np.array_equal(i32.astype(np.float64) * 16, inter.astype(np.float64))
    for u32 in (f(f(area[:, None] + area[None, :]) - i32), f(area[:, None] + f(area[None, :] - i32)),
                f(f(area[:, None] - i32) + area[None, :])):                      # three summation orders
        assert np.array_equal(u32.astype(np.float64) * 16, union.astype(np.float64))
    # with the class offset of batched_nms (idx <= 12) the boxes stay on the lattice and the sides do not change
    off = f(12) * f(b.max() + f(1))
    assert np.array_equal(DR.quarter_units(b + off)[:, 2:] - DR.quarter_units(b + off)[:, :2], q[:, 2:] - q[:, :2])
    # the ties: at every size of the sweep, and the thresholds 0.3 / 0.7 land on the planted 3/10 and 7/10
    for n in NMS_SIZES:
        bb = DR.lattice_boxes(np.random.RandomState(n), n)
        DR.nms_mask_ref(bb, 0.5)                                            # asserts MIN_TIES itself
        DR.nms_mask_ref(bb, 0.25)
        if n <= 700:
            assert DR.exact_tie_count(bb, 0.5) >= DR.MIN_TIES and DR.exact_tie_count(bb, 0.25) >= DR.MIN_TIES, n
            assert DR.exact_tie_count(bb, 0.3) >= 2 and DR.exact_tie_count(bb, 0.7) >= 2, n
    assert np.float32(3) / np.float32(10) == np.float32(0.3) and np.float32(7) / np.float32(10) == np.float32(0.7)
    # an input without ties is refused
    try:
        DR.nms_mask_ref(DR.CHAIN, 0.5)
    except AssertionError:
        pass
    else:
        raise AssertionError("nms_mask_ref accepted an input without ties at the threshold")
    # a tie is not above the threshold, and the table is symmetric
    table = DR.nms_mask_ref(b, 0.5)
    inter, union = DR.lattice_inter_union(b, b)
    assert not table[(2 * inter == union) & (union > 0)].any() and np.array_equal(table, table.T)


def test_greedy_nms_ref_equals_the_oracle():
    for seed, n in enumerate((1, 2, 65, 300, 700)):
        rng = np.random.RandomState(10 + seed)
        b = DR.lattice_boxes(rng, n, plant=seed % 2 == 0)
        scores = torch.linspace(1.0, 0.0, n)
        for thr in (0.5, 0.25, 0.3, 0.7, 0.0, 1.0, -1.0):
            ref = OD.nms(torch.from_numpy(b), scores, thr)
            keep = DR.greedy_nms_ref(b, thr)
            assert np.array_equal(np.nonzero(keep)[0], ref.numpy()), (n, thr)
            full = np.nonzero(keep)[0]
            for mk in (1, len(full), len(full) + 3, max(len(full) // 2, 1)):
                assert np.array_equal(np.nonzero(DR.greedy_nms_ref(b, thr, mk))[0], full[:mk]), (n, thr, mk)
            # the scan agrees with the bit table it would be built from
            table = DR.nms_mask_ref(b, thr, require_ties=False)
            supp = np.zeros(n, bool)
            for i in range(n):
                if not supp[i]:
                    supp[i + 1:] |= table[i, i + 1:]
            assert np.array_equal(~supp, keep)


def test_non_transitive_chain_by_hand():
    inter, union = DR.lattice_inter_union(DR.CHAIN, DR.CHAIN)
    assert Fraction(int(inter[0, 1]), int(union[0, 1])) == Fraction(1, 3) == Fraction(int(inter[1, 2]), int(union[1, 2]))
    assert inter[0, 2] == 0
    for thr in (0.0, 0.25, 0.3):
        assert DR.greedy_nms_ref(DR.CHAIN, thr).tolist() == [True, False, True]
    assert DR.greedy_nms_ref(DR.CHAIN, 0.5).tolist() == [True, True, True]
    assert DR.greedy_nms_ref(DR.CHAIN, -1.0).tolist() == [True, False, False]      # 0 > -1: even a touching box goes


def test_batched_nms_ref_equals_the_oracle():
    rng = np.random.RandomState(3)
    n = 600
    b = DR.lattice_boxes(rng, n)
    scores = rng.permutation(n).astype(np.float32) / n
    cls = rng.randint(0, 13, n)
    valid = rng.rand(n) > 0.2
    for thr, top_n in ((0.5, 100), (0.25, 37), (0.3, 1000)):
        ref = OD.batched_nms(torch.from_numpy(b[valid]), torch.from_numpy(scores[valid]), torch.from_numpy(cls[valid]), thr)[:top_n]
        ref = np.nonzero(valid)[0][ref.numpy()]
        got = DR.batched_nms_ref(b, scores, cls, valid, thr, top_n)
        assert np.array_equal(got, ref), thr
    assert DR.batched_nms_ref(b, scores, cls, np.zeros(n, bool), 0.5, 10).size == 0


def test_decode_ref_close_to_the_oracle():
    rng = np.random.RandomState(4)
    worst = 0.0
    for ncls, weights, clip in ((1, (1., 1., 1., 1.), (97.5, 130.25)), (14, (10., 10., 5., 5.), None), (2, (10., 10., 5., 5.), (400., 416.))):
        n = 257
        xy = rng.uniform(-20, 380, (n, 2))
        wh = rng.uniform(0, 150, (n, 2))
        boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        deltas = (rng.normal(0, 1, (n, ncls * 4)) * 2).astype(np.float32)
        deltas[::9, 2::4] = 40.0                                              # clamped
        ref, bound = DR.decode_ref(deltas, boxes, weights, clip)
        o = OD.decode_boxes(torch.from_numpy(deltas), torch.from_numpy(boxes), weights)
        if clip is not None:
            o = OD.clip_boxes(o.view(n, ncls, 4), clip).view(n, -1)
        err = np.abs(o.double().numpy() - ref)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), float((err / bound).max())
    print(f"decode: fp32 oracle error / bound = {worst:.3f}")
    # the clamp: exactly at it, above it, +inf and NaN give the clamped size; far below it a zero-size box at the centre
    box = np.array([[10., 20., 30., 60.]], np.float32)
    for dz, size in ((DR.XFORM_CLIP, 62.5 * 20), (1e4, 62.5 * 20), (np.inf, 62.5 * 20), (np.nan, 62.5 * 20), (-1e4, 0.0)):
        ref, _ = DR.decode_ref(np.array([[0., 0., dz, 0.]], np.float32), box, (1., 1., 1., 1.))
        assert abs((ref[0, 2] - ref[0, 0]) - size) <= 1e-4 * max(size, 1.0) and ref[0, 3] - ref[0, 1] == 40.0


def test_sigmoid_and_mask_select_ref():
    x = np.array([0., 1.5, -3.25, 88., -88., 104., -104., np.inf, -np.inf], np.float32)
    ref, bound = DR.sigmoid_ref(x)
    assert np.allclose(ref, torch.sigmoid(torch.from_numpy(x).double()).numpy(), rtol=1e-15, atol=0)
    assert ref[0] == 0.5 and ref[7] == 1.0 and ref[8] == 0.0 and (bound >= DR.FLT_MIN).all()
    rng = np.random.RandomState(5)
    k, ncls = 6, 14
    logits = torch.from_numpy(rng.normal(0, 2, (k, ncls, 28, 28)).astype(np.float32))
    labels = torch.tensor([1, 13, 0, 5, 5, 7])
    sub = logits.view(k, ncls, 14, 2, 14, 2).permute(0, 2, 4, 3, 5, 1).reshape(k, 14, 14, 4 * ncls).contiguous()
    want = OD.maskrcnn_inference(logits.double(), [labels])[0].numpy()
    got, _ = DR.sigmoid_ref(DR.mask_select_ref(sub.numpy(), labels.numpy()))
    assert np.allclose(got, want, rtol=1e-6, atol=0)


def test_round_f32_rounds_as_numpy():
    rng = np.random.RandomState(6)
    vals = np.concatenate([rng.normal(0, 1, 300) * 10.0 ** rng.randint(-44, 30, 300), [0.0, 1.0, 2.0 ** -149, 2.0 ** -150, 3 * 2.0 ** -150,
                           1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, -(1 + 2.0 ** -24)]])
    for v in vals:
        assert DR._round_f32(Fraction(float(v))) == float(np.float32(v)), v
    # a tie that float64 cannot see: 1 + 2^-24 + 2^-80 rounds up, 1 + 2^-24 - 2^-80 down
    assert DR._round_f32(1 + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 80)) == 1 + 2.0 ** -23
    assert DR._round_f32(1 + Fraction(1, 2 ** 24) - Fraction(1, 2 ** 80)) == 1.0


def test_paste_ref_close_to_the_oracle():
    rng = np.random.RandomState(7)
    bx = np.array([[10.2, 12.7, 59.9, 80.1], [-15.5, -4.2, 30.0, 44.0], [100., 50., 180.5, 119.9], [0., 0., 191.9, 127.9],
                   [150.3, 100.1, 230.0, 160.0], [40.5, 40.5, 41.2, 41.0], [5., 90., 120., 131.], [60., 70., 20., 30.],
                   [-300., -300., -200., -250.], [-50., -50., 400., 300.], [33., 44., 33., 44.]], np.float32)
    k = bx.shape[0]
    masks = rng.rand(k, 1, 28, 28).astype(np.float32)
    hw = (128, 192)
    ref, bound = DR.paste_ref(masks, bx, hw)
    o = OD.paste_masks_in_image(torch.from_numpy(masks), torch.from_numpy(bx), hw).double().numpy()
    # the oracle's interpolate forms a position as fl(fl(s (r + .5)) - .5), one fp32 step (<= 2^-19 below 32) from the fused form:
    # each axis moves a weight by that much, a value by that much times the map's range (<= 1 here); its own fp32
    # interpolation adds the bound once more
    err = np.abs(o - ref)
    assert (err <= 2 * bound + 2.0 ** -18).all(), float(err.max())
    for i in range(k):
        inside = DR.paste_inside(bx[i], hw)
        assert (ref[i, 0][~inside] == 0).all() and (o[i, 0][~inside] == 0).all()
        assert (bound[i, 0][~inside] == 0).all()
    assert ref[7].max() == 0 and ref[8].max() == 0 and ref[0].max() > 0.5          # inverted, outside; an ordinary one is not empty
    # solid maps: away from the zero border of the padded map the value is exactly 1
    ref1, _ = DR.paste_ref(np.ones((1, 1, 28, 28), np.float32), np.array([[-50., -50., 400., 300.]], np.float32), hw)
    assert ref1.min() == 1.0 and ref1.max() == 1.0
    ref1, _ = DR.paste_ref(np.ones((1, 1, 28, 28), np.float32), np.array([[10., 10., 37., 37.]], np.float32), (64, 40))
    x0, y0, x1, y1, bw, bh, sx, sy = DR.paste_box_ref(np.array([10., 10., 37., 37.], np.float32))
    assert (x0, y0, x1, y1, bw, bh) == (9, 9, 37, 37, 29, 29)
    assert int((ref1 > 0).sum()) == 29 * 29 and int((ref1 > 0.5).sum()) == 27 * 27


def test_rpn_topk_ref_equals_a_stable_sort_and_pins_the_special_values():
    rng = np.random.RandomState(8)
    for n, k in ((1, 1), (1025, 1024), (5000, 1000), (3073, 700)):
        x = rng.normal(0, 3, n).astype(np.float32)
        if n == 5000:
            x = np.round(x * 2) / 2                                           # heavy ties
        x[x == 0] = 0.5                                                      # -0-free
        want = torch.argsort(torch.from_numpy(x), descending=True, stable=True)[:k].numpy()
        assert np.array_equal(DR.rpn_topk_ref(x, k), want), n
    x = np.array([np.nan, -0.0, 0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 0.0], np.float32)
    assert DR.rpn_topk_ref(x, 9).tolist() == [3, 6, 1, 2, 8, 7, 0, 4, 5]


def test_box_iou_ref_exact_and_float_forms_agree():
    rng = np.random.RandomState(9)
    a, b = DR.lattice_boxes(rng, 40), DR.lattice_boxes(rng, 33)
    a[3] = a[3][[2, 1, 0, 3]]                                                # inverted in x: negative area, no clamping
    exact, none = DR.box_iou_ref(a, b)
    assert none is None and exact.dtype == np.float32
    f = torch.from_numpy
    ta, tb = f(a), f(b)
    area_a = (ta[:, 2] - ta[:, 0]) * (ta[:, 3] - ta[:, 1])
    area_b = (tb[:, 2] - tb[:, 0]) * (tb[:, 3] - tb[:, 1])
    wh = (torch.min(ta[:, None, 2:], tb[None, :, 2:]) - torch.max(ta[:, None, :2], tb[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    tv = (inter / (area_a[:, None] + area_b[None, :] - inter)).numpy()      # torchvision's box_iou, fp32
    assert np.array_equal(exact, tv, equal_nan=True)
    assert np.isnan(exact).any() or (DR.quarter_units(a)[:, 2] != DR.quarter_units(a)[:, 0]).all()
    fa = (a + np.float32(0.001)).astype(np.float32)                         # off the lattice: the float64 form
    approx, bound = DR.box_iou_ref(fa, b)
    assert bound is not None and approx.dtype == np.float64
    ok = np.isfinite(exact) & np.isfinite(approx)
    assert np.abs(approx - exact)[ok].max() < 1e-2
