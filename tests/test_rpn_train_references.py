"""CPU: hand-derivable known answers for the restatement of the RPN's training branch (``rpn_train_refs.py``), which the
GPU tests then use as their reference; plus the parts of the feature that can be seen without a GPU (the ABI entry points,
the constructor surface, the frozen-backbone rule)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import rpn_train_refs as PR
import roi_train_refs as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("seam_rpn_match_f32", "seam_rpn_sample_f32", "seam_rpn_gather_patches_f32", "seam_rpn_loss_fwd_bwd_f32")


# ------------------------------------------------------------------------------ matcher
def test_anchor_identical_to_a_gt_box_is_foreground():
    anchors = torch.tensor([[10., 10., 50., 50.], [200., 200., 240., 240.]])
    gt = torch.tensor([[10., 10., 50., 50.]])
    labels, matched = PR.match(anchors, gt)
    assert float(RR.box_iou_f32(gt, anchors)[0, 0]) == 1.0
    assert labels.tolist() == [1, 0] and matched.tolist() == [0, 0]


def test_iou_exactly_half_is_ignored():
    gt = torch.tensor([[0., 0., 10., 10.]])
    anchors = torch.tensor([[0., 0., 10., 10.],       # 1.0: foreground, and the GT box's best anchor
                            [0., 0., 10., 5.],        # 50 / 100 = 0.5: between 0.3 and 0.7
                            [0., 0., 10., 2.],        # 0.2: background
                            [0., 0., 10., 7.],        # 0.7 exactly: foreground (not < 0.7)
                            [0., 0., 10., 3.]])       # 0.3 exactly: ignored (not < 0.3)
    q = RR.box_iou_f32(gt, anchors)[0]
    # the thresholds are compared in fp32, where 70 / 100 and 30 / 100 round to the same values as 0.7 and 0.3
    assert float(q[1]) == 0.5 and bool(q[3] == torch.tensor(0.7)) and bool(q[4] == torch.tensor(0.3))
    labels, matched = PR.match(anchors, gt)
    assert labels.tolist() == [1, -1, 0, 1, -1]
    assert matched.tolist() == [0, 0, 0, 0, 0]


def test_two_gt_boxes_tying_take_the_first():
    gt = torch.tensor([[0., 0., 10., 10.], [0., 0., 10., 10.], [100., 100., 120., 120.]])
    anchors = torch.tensor([[0., 0., 10., 10.], [100., 100., 120., 120.]])
    labels, matched = PR.match(anchors, gt)
    assert labels.tolist() == [1, 1] and matched.tolist() == [0, 2]


def test_low_quality_rule_restores_an_anchor_to_its_own_argmax():
    gt = torch.tensor([[0., 0., 10., 10.], [0., 0., 4., 3.]])
    anchors = torch.tensor([[0., 0., 10., 10.],       # GT 0: 1.0;          GT 1: 12 / 100 = 0.12
                            [0., 0., 10., 6.],        # GT 0: 60/100 = 0.6; GT 1: 12 / 60 = 0.2, GT 1's largest IoU
                            [300., 300., 320., 320.]])
    q = RR.box_iou_f32(gt, anchors)
    assert float(q[0, 0]) == 1.0 and bool(q[0, 1] == torch.tensor(0.6)) and float(q[1, 1]) > float(q[1, 0]) > 0.0
    # without GT 1 the middle anchor sits in the ignored band
    labels, matched = PR.match(anchors, gt[:1])
    assert labels.tolist() == [1, -1, 0] and matched.tolist() == [0, 0, 0]
    # GT 1's best anchor is the middle one: the rule makes it foreground -- matched to its OWN argmax, GT 0, not to GT 1
    labels, matched = PR.match(anchors, gt)
    assert labels.tolist() == [1, 1, 0] and matched.tolist() == [0, 0, 0]
    # with the GT boxes swapped the same anchor is matched to index 1
    labels, matched = PR.match(anchors, gt[[1, 0]])
    assert labels.tolist() == [1, 1, 0] and matched.tolist() == [1, 1, 0]


def test_gt_box_overlapping_nothing_turns_the_whole_image_foreground():
    anchors, _ = PR.anchor_grid(256, 320)
    gt = torch.tensor([[100., 100., 160., 180.], [5000., 5000., 5100., 5100.]])
    labels, matched = PR.match(anchors, gt)
    assert anchors.shape[0] == 20460 and int((labels == 1).sum()) == 20460
    assert set(matched.tolist()) == {0}                # every IoU with GT 1 is 0: the first maximum is GT 0 everywhere
    s = PR.assign_and_sample(anchors, gt, torch.rand(anchors.shape[0], generator=torch.Generator().manual_seed(0)))
    assert len(s["idx"]) == 128 and bool((s["labels"] == 1).all())


def test_image_without_gt_is_all_background_with_zero_targets():
    anchors, _ = PR.anchor_grid(256, 320)
    s = PR.assign_and_sample(anchors, torch.zeros((0, 4)), torch.rand(anchors.shape[0], generator=torch.Generator().manual_seed(1)))
    assert int((s["labels_all"] != 0).sum()) == 0 and len(s["idx"]) == 256
    assert bool((s["labels"] == 0).all()) and float(s["targets"].abs().max()) == 0.0


# ------------------------------------------------------------------------------ sampler, encode
def test_num_pos_num_neg_at_the_cap():
    assert PR.num_pos_neg(500, 10000) == (128, 128)
    assert PR.num_pos_neg(128, 10000) == (128, 128)
    assert PR.num_pos_neg(127, 10000) == (127, 129)
    assert PR.num_pos_neg(0, 10000) == (0, 256)
    assert PR.num_pos_neg(300, 50) == (128, 50)
    assert PR.num_pos_neg(3, 7) == (3, 7)
    labels = torch.cat([torch.ones(200, dtype=torch.int64), torch.zeros(400, dtype=torch.int64), -torch.ones(50, dtype=torch.int64)])
    keys = torch.rand(650, generator=torch.Generator().manual_seed(2))
    idx = PR.sample_by_keys(labels, keys)
    assert len(idx) == 256 and int((labels[idx] == 1).sum()) == 128 and int((labels[idx] == 0).sum()) == 128
    assert bool((idx[1:] > idx[:-1]).all())
    # the kept positives are the 128 smallest keys among the positives
    assert set(idx[labels[idx] == 1].tolist()) == set(torch.argsort(keys[:200], stable=True)[:128].tolist())
    # all keys equal: the lower index wins
    idx = PR.sample_by_keys(labels, torch.full((650,), 0.5))
    assert idx.tolist() == list(range(128)) + list(range(200, 328))


def test_encode_unit_weights_known_answer():
    anchors = torch.tensor([[0., 0., 10., 20.]])
    gt = torch.tensor([[5., 10., 25., 50.]])              # centre (15, 30), size (20, 40); anchor centre (5, 10), size (10, 20)
    t = PR.encode(gt, anchors)[0]
    assert t[:2].tolist() == [1.0, 1.0]
    assert abs(float(t[2]) - 0.6931471805599453) < 1e-7 and abs(float(t[3]) - 0.6931471805599453) < 1e-7


# ------------------------------------------------------------------------------ losses
def test_losses_against_torch_functional():
    g = torch.Generator().manual_seed(3)
    s = 300
    obj = torch.randn(s, generator=g, dtype=torch.float64) * 3
    dlt = torch.randn((s, 4), generator=g, dtype=torch.float64) * 0.3
    labels = (torch.rand(s, generator=g) < 0.4).to(torch.int64)
    tgt = torch.randn((s, 4), generator=g, dtype=torch.float64) * 0.3
    lo, lb = PR.rpn_losses(obj, dlt, labels, tgt)
    pos = labels == 1
    assert abs(float(lo) - float(F.binary_cross_entropy_with_logits(obj, labels.double()))) < 1e-15
    ref = F.smooth_l1_loss(dlt[pos], tgt[pos], beta=1 / 9, reduction="sum") / s
    assert abs(float(lb) - float(ref)) < 1e-12
    # one hand-computed row: x = 0, y = 1 -> log 2; |d| = 1 on one delta -> 1 - 1/18, the three others exact
    lo, lb = PR.rpn_losses(torch.zeros(1, dtype=torch.float64), torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64),
                           torch.ones(1, dtype=torch.int64), torch.zeros((1, 4), dtype=torch.float64))
    assert abs(float(lo) - 0.6931471805599453) < 1e-15 and abs(float(lb) - (1 - 1 / 18)) < 1e-15


def test_dense_head_order_is_level_y_x_anchor():
    torch.manual_seed(0)
    P = {"conv.weight": torch.zeros(4, 4, 3, 3), "conv.bias": torch.ones(4), "cls_logits.weight": torch.zeros(3, 4, 1, 1),
         "cls_logits.bias": torch.tensor([1., 2., 3.]), "bbox_pred.weight": torch.zeros(12, 4, 1, 1),
         "bbox_pred.bias": torch.arange(12.)}
    obj, dlt = PR.dense_head([torch.zeros(1, 4, 2, 2), torch.zeros(1, 4, 1, 1)], P)
    assert obj.shape == (1, 15) and obj[0, :6].tolist() == [1., 2., 3., 1., 2., 3.]
    assert dlt.shape == (1, 15, 4) and dlt[0, 1].tolist() == [4., 5., 6., 7.] and dlt[0, 12].tolist() == [0., 1., 2., 3.]


# ------------------------------------------------------------------------------ the feature, as far as a CPU sees it
def test_entry_points_are_declared_and_bound():
    from seam_match_rcnn_amd import _native
    txt = open(os.path.join(ROOT, "include", "seam_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", txt), f"{name} is not declared in include/seam_hip.h"
        assert name in _native.SIGNATURES, f"{name} is not bound in _native.SIGNATURES"


def test_rpn_keeps_the_training_knobs():
    from seam_match_rcnn_amd.models import detection as det
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params
    rpn = det.RegionProposalNetwork()
    assert (rpn.pre_nms_top_n_train, rpn.post_nms_top_n_train) == (2000, 2000)
    assert (rpn.batch_size_per_image, rpn.positive_fraction, rpn.fg_iou_thresh, rpn.bg_iou_thresh) == (256, 0.5, 0.7, 0.3)
    assert rpn.sample_generator is None
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14, **params)
    assert (m.rpn.pre_nms_top_n_train, m.rpn.post_nms_top_n_train) == (2000, 8000)
    assert (m.rpn.pre_nms_top_n, m.rpn.post_nms_top_n) == (1000, 4000)
    assert "rpn_pre_nms_top_n_train" not in m._ignored_kwargs and "rpn_post_nms_top_n_train" not in m._ignored_kwargs


def test_training_forward_needs_a_frozen_backbone_and_targets():
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14).train()
    targets = [dict(boxes=torch.tensor([[4., 4., 20., 20.]]), labels=torch.ones(1, dtype=torch.int64))]
    with pytest.raises(NotImplementedError, match="backbone"):       # raised before any tensor reaches a device
        m([torch.zeros(3, 32, 32)], targets)
    with pytest.raises(NotImplementedError):                          # without targets: the inference-only message, as before
        m([torch.zeros(3, 32, 32)])


def test_mask_resize_is_torch_nearest():
    from seam_match_rcnn_amd.models.matchrcnn import resize_masks_nearest
    g = torch.Generator().manual_seed(4)
    for (hi, wi, ho, wo) in ((600, 800, 800, 1066), (750, 1101, 800, 1174), (123, 77, 256, 160), (64, 64, 64, 64)):
        m = (torch.rand((2, hi, wi), generator=g) < 0.5).to(torch.uint8)
        out = resize_masks_nearest(m, (ho, wo))
        assert out.dtype == torch.uint8
        assert torch.equal(out, F.interpolate(m[:, None].float(), size=(ho, wo))[:, 0].byte())
