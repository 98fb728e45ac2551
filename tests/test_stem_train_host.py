"""CPU: the switch of stem training (``ResNet50Body.train_stem`` and the ``train_stem`` keyword of the two constructors that take
it) and ``detection.stem_s2d_grad_to_oihw``, the map of the stem's space-to-depth weight gradient back onto the 7x7 taps.

``pack`` below is the forward packing written out from its formula, tap by tap, not taken from the code under test:
``w'[k, (dy*2+dx)*3 + c, r', s'] = w[k, c, 2r'+dy-1, 2s'+dx-1]``, zero where the 7x7 kernel has no tap (index -1)."""
import pytest
import torch

from seam_match_rcnn_amd.models import detection as det


def pack(w):
    k = w.shape[0]
    ws = torch.zeros((k, 12, 4, 4), dtype=w.dtype)
    for dy in range(2):
        for dx in range(2):
            for c in range(3):
                for r in range(4):
                    for s in range(4):
                        i, j = 2 * r + dy - 1, 2 * s + dx - 1
                        if i >= 0 and j >= 0:
                            ws[:, (dy * 2 + dx) * 3 + c, r, s] = w[:, c, i, j]
    return ws


def padded_slots():
    """[12,4,4] mask of the slots that hold the padded tap -1."""
    m = torch.zeros((12, 4, 4), dtype=torch.bool)
    for dy in range(2):
        for dx in range(2):
            for r in range(4):
                for s in range(4):
                    if 2 * r + dy - 1 < 0 or 2 * s + dx - 1 < 0:
                        m[(dy * 2 + dx) * 3:(dy * 2 + dx) * 3 + 3, r, s] = True
    return m


def test_the_attribute_defaults_to_false_and_the_keyword_sets_it():
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    assert det.ResNet50Body().train_stem is False
    assert det.resnet_fpn_backbone("resnet50", False).body.train_stem is False
    assert det.resnet_fpn_backbone("resnet50", False, trainable_layers=5).body.train_stem is False
    b = det.resnet_fpn_backbone("resnet50", False, trainable_layers=5, train_stem=True)
    assert b.body.train_stem is True and b.body.conv1.weight.requires_grad
    b = det.resnet_fpn_backbone("resnet50", False, trainable_layers=3, train_stem=True)       # the switch freezes and unfreezes nothing
    assert b.body.train_stem is True and not b.body.conv1.weight.requires_grad
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    assert m.backbone.body.train_stem is False
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14, trainable_backbone_layers=5, train_stem=True)
    assert m.backbone.body.train_stem is True and m.backbone.body.conv1.weight.requires_grad
    assert "train_stem" not in m.state_dict()


def test_the_packing_written_out_here_is_the_bodys():
    """``pack`` against the forward's own expression (models/detection.py, ``ResNet50Body.packed``), restated."""
    import torch.nn.functional as F
    w = torch.randn((64, 3, 7, 7), generator=torch.Generator().manual_seed(1))
    w8 = F.pad(w, (1, 0, 1, 0))
    assert torch.equal(pack(w), w8.view(64, 3, 4, 2, 4, 2).permute(0, 3, 5, 1, 2, 4).reshape(64, 12, 4, 4))
    assert int(padded_slots().sum()) == 12 * 16 - 3 * 49


def test_unpack_is_the_exact_inverse_of_the_forward_packing():
    w = torch.randn((64, 3, 7, 7), generator=torch.Generator().manual_seed(2))
    back = det.stem_s2d_grad_to_oihw(pack(w))
    assert back.shape == w.shape and back.is_contiguous() and torch.equal(back, w)


def test_unpack_is_the_adjoint_of_the_packing():
    g = torch.Generator().manual_seed(3)
    w = torch.randn((64, 3, 7, 7), generator=g, dtype=torch.float64)
    gs = torch.randn((64, 12, 4, 4), generator=g, dtype=torch.float64)
    lhs, rhs = float((pack(w) * gs).sum()), float((w * det.stem_s2d_grad_to_oihw(gs)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(pack(w).norm() * gs.norm())
    # ... and autograd's own adjoint of the packing, element by element
    wr = w.clone().requires_grad_(True)
    pack(wr).backward(gs)
    assert torch.equal(wr.grad, det.stem_s2d_grad_to_oihw(gs))


def test_every_slot_of_the_padded_tap_is_ignored():
    g = torch.Generator().manual_seed(4)
    gs = torch.randn((64, 12, 4, 4), generator=g)
    want = det.stem_s2d_grad_to_oihw(gs)
    pad = padded_slots()
    for fill in (float("nan"), float("inf"), 1e30):
        poisoned = gs.clone()
        poisoned[:, pad] = fill
        assert torch.equal(det.stem_s2d_grad_to_oihw(poisoned), want)
    only_pad = torch.zeros_like(gs)
    only_pad[:, pad] = 1.0
    assert not bool(det.stem_s2d_grad_to_oihw(only_pad).any())
    # every one of the 147 taps comes from exactly one slot: an indicator in a real slot lands on exactly one tap
    ones = torch.zeros((1, 12, 4, 4))
    ones[0, ~pad] = 1.0
    assert torch.equal(det.stem_s2d_grad_to_oihw(ones), torch.ones((1, 3, 7, 7)))


def test_a_wrong_shape_is_a_value_error():
    with pytest.raises(ValueError):
        det.stem_s2d_grad_to_oihw(torch.zeros((64, 3, 7, 7)))
