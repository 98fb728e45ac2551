"""GPU: the split classes c2 / fpn3 / rpn3 / mask3 in the model (models/detection.py) -- two 128 x 160 images through body + FPN +
RPN head, and the mask head on 8 ROIs, with ``ops.W24SX_MIN_BLOCKS`` at 0 so that maps of this size take the route.  With the classes removed, or SEAM_W24SX off, the launches are the fp32 kernels'; with them
on, the outputs stay within the model-level tolerance of the split tests (1e-5 of each output's largest value,
tests/test_gpu_stem_sxpc_model.py); an optimizer step leaves every ``u24x`` twin at the bytes of a fresh pack; a training-mode
module and a grad-enabled call keep the exact kernels."""
import contextlib

import numpy as np
import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
NEW = frozenset({"c2", "fpn3", "rpn3", "mask3"})


def normal(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def build():
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models import detection as det
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items()}
    sub = lambda p: {k[len(p):]: v for k, v in sd.items() if k.startswith(p)}
    m = torch.nn.Module()
    m.backbone = torch.nn.Module()
    m.backbone.body, m.backbone.fpn = det.ResNet50Body(), det.FeaturePyramidNetwork()
    m.rpn = torch.nn.Module()
    m.rpn.head = det.RPNHead()
    m.mask_head = det.MaskRCNNHeads(256, (256, 256, 256, 256))
    m.backbone.body.load_state_dict(sub("backbone.body."))
    m.backbone.fpn.load_state_dict(sub("backbone.fpn."))
    m.rpn.head.load_state_dict(sub("rpn.head."))
    m.mask_head.load_state_dict(sub("roi_heads.mask_head."))
    return m.to(DEV).eval()


_M = {}


def model():
    if not _M:
        _M["m"] = build()
        for p in _M["m"].parameters():
            p.requires_grad_(False)
    return _M["m"]


def run(m):
    """-> (outputs, CONV_TRACE names)"""
    from seam_match_rcnn_amd import ops
    x = normal(3, (2, 128, 160, 4))
    x[..., 3] = 0
    rois = torch.relu(normal(4, (8, 14, 14, 256))).to(DEV)
    ops.CONV_TRACE = []
    try:
        feats = m.backbone.body(x.to(DEV))
        pyr = m.backbone.fpn(feats)
        rpn = m.rpn.head.fused(list(pyr.values()))
        mask = m.mask_head(rois)
        torch.cuda.synchronize()
        return list(feats) + list(pyr.values()) + list(rpn) + [mask], [t[0] for t in ops.CONV_TRACE]
    finally:
        ops.CONV_TRACE = None


@contextlib.contextmanager
def knobs():
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    saved = det.SPLIT_CLASSES, ops.W24SX, ops.W24SX_MIN_BLOCKS
    try:
        ops.W24SX_MIN_BLOCKS = 0          # these maps are far below the rule's 128 blocks per image: every other rule decides here
        yield det, ops
    finally:
        det.SPLIT_CLASSES, ops.W24SX, ops.W24SX_MIN_BLOCKS = saved


def test_switches_restore_the_fp32_launches_and_the_route_stays_in_tolerance():
    m = model()
    with knobs() as (det, ops), torch.no_grad():
        det.SPLIT_CLASSES = det.SPLIT_CLASSES | NEW
        on, names_on = run(m)
        assert names_on.count("conv3x3_wino24sx") >= 4, names_on
        det.SPLIT_CLASSES = det.SPLIT_CLASSES - NEW
        off, names_off = run(m)
        det.SPLIT_CLASSES = det.SPLIT_CLASSES | NEW
        ops.W24SX = False
        off2, names_off2 = run(m)
        ops.W24SX = True
        assert "conv3x3_wino24sx" not in names_off and names_off == names_off2
        assert all(torch.equal(a, b) for a, b in zip(off, off2))
        # every launch that moved was an F(2x4,3x3) launch of the fp32 kernels, and nothing else changed
        assert len(names_on) == len(names_off)
        for a, b in zip(names_on, names_off):
            assert a == b or (a == "conv3x3_wino24sx" and b.startswith("conv3x3_wino24")), (a, b)
        for i, (a, b) in enumerate(zip(on, off)):
            d, s = float((a - b).abs().max()), float(b.abs().max())
            print(f"output {i} {tuple(b.shape)}: |on - off| / max {d / s:.3e}")
        for i, (a, b) in enumerate(zip(on, off)):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()), i
        # a training-mode module and a grad-enabled call do not take the route
        m.train()
        _, names = run(m)
        m.eval()
        assert "conv3x3_wino24sx" not in names
    with knobs() as (det, ops), torch.enable_grad():
        det.SPLIT_CLASSES = det.SPLIT_CLASSES | NEW
        _, names = run(m)
        assert "conv3x3_wino24sx" not in names


def test_after_an_sgd_step_every_twin_equals_a_fresh_pack():
    from seam_match_rcnn_amd.optim import SGD
    with knobs() as (det, ops):
        det.SPLIT_CLASSES = det.SPLIT_CLASSES | NEW
        m = build()
        body, fpn, head = m.backbone.body, m.backbone.fpn, m.rpn.head
        train = [body.layer2[1].conv2.weight, body.layer3[2].conv2.weight, fpn.layer_blocks[0].weight, fpn.layer_blocks[3].weight, head.conv.weight]
        for p in m.parameters():
            p.requires_grad_(any(p is t for t in train))
        opt = SGD(train, lr=0.05, momentum=0.9, model=m)

        def twins(mm):
            b, f, h = mm.backbone.body, mm.backbone.fpn, mm.rpn.head
            b.packed(); f.packed(); h.packed()
            return [b._pk[(2, 1)]["c2w"], b._pk[(3, 2)]["c2w"], f._out_twins[0], f._out_twins[3], h._conv_twin]

        mine = twins(m)
        before = [t.u24x.clone() for t in mine]
        for i, p in enumerate(train):
            p.grad = normal(20 + i, tuple(p.shape)).to(DEV) * 0.1
        opt.step()
        assert opt.plan.refreshes == 1 and opt.plan.rebuilds == 0
        after = twins(m)
        assert all(a is b for a, b in zip(mine, after)) and not any(torch.equal(t.u24x, o) for t, o in zip(after, before))
        fresh = build()
        for dst, src in ((fresh.backbone.body, body), (fresh.backbone.fpn, fpn), (fresh.rpn.head, head)):
            dst.load_state_dict(src.state_dict())
        for t, f in zip(after, twins(fresh)):
            assert torch.equal(t.u24x, f.u24x) and torch.equal(t.w, f.w) and torch.equal(t.shift, f.shift)
