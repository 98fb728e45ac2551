"""CPU: torchvision's ``trainable_layers`` rule on ``det.resnet_fpn_backbone`` and the two model constructors that pass it on.

torchvision (``resnet_fpn_backbone`` / ``_resnet_fpn_extractor``): ``layers_to_train = ['layer4', 'layer3', 'layer2', 'layer1',
'conv1'][:trainable_layers]`` and every parameter of the body whose name starts with none of them is frozen.  The body's
FrozenBatchNorm2d are buffers, so its parameters are the 53 conv weights; the FPN is not touched.  The expected sets below are
written out by hand, not derived from the rule under test."""
import pytest

from seam_match_rcnn_amd.models import detection as det

# trainable top-level children of the body for each value of the keyword
EXPECTED = {
    0: set(),
    1: {"layer4"},
    2: {"layer4", "layer3"},
    3: {"layer4", "layer3", "layer2"},
    4: {"layer4", "layer3", "layer2", "layer1"},
    5: {"layer4", "layer3", "layer2", "layer1", "conv1"},
}
ALL = EXPECTED[5]


def body_names(backbone):
    return {n: p.requires_grad for n, p in backbone.body.named_parameters()}


@pytest.mark.parametrize("n", sorted(EXPECTED))
def test_trainable_layers_freezes_torchvisions_set(n):
    b = det.resnet_fpn_backbone("resnet50", False, trainable_layers=n)
    names = body_names(b)
    assert len(names) == 53 and {k.split(".")[0] for k in names} == ALL
    for k, rg in names.items():
        assert rg == (k.split(".")[0] in EXPECTED[n]), (n, k)
    assert names["conv1.weight"] == (n == 5)
    assert names["layer2.0.downsample.0.weight"] == (n >= 3) and names["layer1.2.conv3.weight"] == (n >= 4)
    fpn = dict(b.fpn.named_parameters())
    assert len(fpn) == 16 and all(p.requires_grad for p in fpn.values())


def test_none_leaves_everything_trainable():
    for b in (det.resnet_fpn_backbone("resnet50", False), det.resnet_fpn_backbone("resnet50", False, trainable_layers=None)):
        assert all(body_names(b).values()) and all(p.requires_grad for p in b.fpn.parameters())


@pytest.mark.parametrize("bad", [6, -1, 2.5, "3", True])
def test_anything_else_is_a_value_error(bad):
    with pytest.raises(ValueError):
        det.resnet_fpn_backbone("resnet50", False, trainable_layers=bad)


def test_the_model_constructors_pass_the_keyword_on():
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    for ctor in (matchrcnn_resnet50_fpn, videomatchrcnn_resnet50_fpn):
        m = ctor(pretrained_backbone=False, num_classes=14, trainable_backbone_layers=3)
        names = body_names(m.backbone)
        assert {k.split(".")[0] for k, rg in names.items() if rg} == EXPECTED[3], ctor.__name__
        assert all(p.requires_grad for p in m.backbone.fpn.parameters()) and all(p.requires_grad for p in m.rpn.parameters())
        m = ctor(pretrained_backbone=False, num_classes=14)
        assert all(body_names(m.backbone).values()), ctor.__name__
        with pytest.raises(ValueError):
            ctor(pretrained_backbone=False, num_classes=14, trainable_backbone_layers=6)
