"""GPU: training the FPN -- ``autograd.FPNFunction`` alone, ``matchrcnn_resnet50_fpn`` with ``backbone.body`` frozen and
``backbone.fpn`` trainable, and the RoI heads / the RPN called directly on feature maps that require a gradient.

References are float64 torch autograd on the CPU through ``oracle.detection.fpn`` / ``oracle.detection.roi_align`` and the
head and loss restatements of ``roi_train_refs.py`` / ``rpn_train_refs.py`` (``fpn_train_refs.py`` chains them).  The device's
body features and the device's sampled rows are constants of the reference: the samplers are exact given the same keys
(tests/test_gpu_roi_train.py, tests/test_gpu_rpn_train.py), so the reference redraws the keys from the same seeds.

Bound: the project's rule for a gradient tensor behind a chain of fp32 GEMMs and ReLUs (``_compare`` of
tests/test_gpu_roi_train.py, restated as ``fpn_train_refs.compare_grads``): relative Frobenius error <= 2e-3, largest error
<= 2e-2 of the reference's largest element.
"""
import numpy as np
import pytest
import torch

import fpn_train_refs as FR
import rpn_train_refs as PR
from oracle import detection as OD

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NCLS = 14
ROI_BATCH = 64
SIX = ["loss_classifier", "loss_box_reg", "loss_mask", "loss_match", "loss_objectness", "loss_rpn_box_reg"]


def nchw64(t):
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


# ------------------------------------------------------------------------------ FPNFunction alone
def test_fpn_function_alone_vs_float64():
    from seam_match_rcnn_amd.models import detection as det
    torch.manual_seed(3)
    chans, hws = (32, 64, 96, 128), [(25, 21), (13, 11), (7, 6), (4, 3)]
    fpn = det.FeaturePyramidNetwork(in_channels=chans, out_channels=64).to(DEV)
    g = torch.Generator().manual_seed(4)
    feats = [torch.randn((2, h, w, c), generator=g).to(DEV).requires_grad_(True) for c, (h, w) in zip(chans, hws)]
    with torch.no_grad():
        plain = fpn([f.detach() for f in feats])
    taped = fpn.forward_taped(feats)
    assert list(taped) == ["0", "1", "2", "3", "pool"] and tuple(taped["pool"].shape) == (2, 2, 2, 64)
    assert all(torch.equal(taped[k], plain[k]) for k in plain)                   # the same launches, the same bits
    ups = {k: torch.randn(tuple(v.shape), generator=g) for k, v in taped.items()}

    def grads_of():
        fpn.zero_grad(set_to_none=True)
        for f in feats:
            f.grad = None
        out = fpn.forward_taped(feats)
        sum((out[k] * ups[k].to(DEV)).sum() for k in out).backward()
        got = {k: p.grad.detach().clone() for k, p in fpn.named_parameters()}
        got.update({f"C{i + 2}": f.grad.detach().clone() for i, f in enumerate(feats)})
        return got
    got, again = grads_of(), grads_of()
    assert len(got) == 20 and all(torch.equal(got[k], again[k]) for k in got)
    P = {"backbone.fpn." + k: p.detach().cpu().double().requires_grad_(True) for k, p in fpn.named_parameters()}
    f64 = [nchw64(f).requires_grad_(True) for f in feats]
    ref = OD.fpn(f64, P)
    for k in plain:
        assert float((nchw64(plain[k]) - ref[k].detach()).abs().max()) <= 1e-4 * float(ref[k].detach().abs().max()), k
    sum((ref[k] * ups[k].double().permute(0, 3, 1, 2)).sum() for k in ref).backward()
    want = {k[len("backbone.fpn."):]: p.grad for k, p in P.items()}
    want.update({f"C{i + 2}": f.grad.permute(0, 2, 3, 1) for i, f in enumerate(f64)})
    FR.compare_grads(got, want, sorted(want))
    # without the pool's gradient and with an unused output: the missing gradients count as zeros
    fpn.zero_grad(set_to_none=True)
    out = fpn.forward_taped([f.detach() for f in feats])
    (out["1"] * ups["1"].to(DEV)).sum().backward()
    assert float(fpn.layer_blocks[0].weight.grad.abs().max()) == 0 and float(fpn.inner_blocks[0].weight.grad.abs().max()) == 0
    assert float(fpn.layer_blocks[1].weight.grad.abs().max()) > 0 and float(fpn.inner_blocks[3].weight.grad.abs().max()) > 0


# ------------------------------------------------------------------------------ the whole model
def make_model(fpn_trainable):
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS, min_size=256, max_size=320, **params)
    sd = synth.detector_state(5, NCLS)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    for p in m.backbone.body.parameters():
        p.requires_grad_(False)
    for p in m.backbone.fpn.parameters():
        p.requires_grad_(fpn_trainable)
    # 64 RoI samples per image (16 positives at most): the float64 reference differentiates RoIAlign ROI by ROI
    m.roi_heads.batch_size_per_image = ROI_BATCH
    return m.to(DEV).train()


def make_model_batch(seed=0):
    """The 256 x 320 two-image batch of tests/test_gpu_rpn_train.py::make_model_batch."""
    import seam_match_rcnn_amd.synth as synth
    g = torch.Generator().manual_seed(seed)
    images, targets = [], []
    for i, (h, w) in enumerate(((200, 250), (192, 240))):
        images.append(torch.from_numpy(synth.frames(50 + i, 1, h, w)[0]).to(DEV))
        ng = 2 + i
        gt = PR.random_gt(g, ng, h, w, 30, 120)
        masks = torch.zeros((ng, h, w), dtype=torch.uint8)
        for j, b in enumerate(gt.round().to(torch.int64).tolist()):
            masks[j, b[1]:b[3], b[0]:b[2]] = 1
        targets.append(dict(boxes=gt.to(DEV), labels=torch.randint(1, NCLS, (ng,), generator=g).to(DEV), masks=masks.to(DEV),
                            pair_ids=torch.randint(0, 3, (ng,), generator=g), styles=torch.randint(1, 3, (ng,), generator=g),
                            sources=torch.tensor([i])))
    return images, targets


def run_model(m, images, targets, capture=None):
    m.rpn.sample_generator = torch.Generator(device=DEV).manual_seed(1)
    m.roi_heads.sample_generator = torch.Generator(device=DEV).manual_seed(2)
    m.zero_grad(set_to_none=True)
    hooks = []
    if capture is not None:
        hooks.append(m.backbone.body.register_forward_hook(lambda mod, a, out: capture.__setitem__("body", [o.detach() for o in out])))
        hooks.append(m.rpn.register_forward_pre_hook(lambda mod, a, kw: capture.__setitem__("rpn", (a, kw)), with_kwargs=True))
        hooks.append(m.roi_heads.register_forward_pre_hook(lambda mod, a: capture.__setitem__("roi", a)))
    losses = m(images, targets)
    for h in hooks:
        h.remove()
    assert list(losses) == SIX
    sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in losses.items()}, grads


@pytest.fixture(scope="module")
def runs():
    images, targets = make_model_batch()
    frozen = run_model(make_model(False), images, targets)
    m = make_model(True)
    cap = {}
    first = run_model(m, images, targets, cap)
    second = run_model(m, images, targets)
    return dict(images=images, targets=targets, frozen=frozen, first=first, second=second, cap=cap, model=m)


def test_model_losses_and_head_gradients_equal_the_frozen_run(runs):
    (fl, fg), (l1, g1) = runs["frozen"], runs["first"]
    for k in SIX:
        print(k, float(l1[k]))
        assert torch.equal(l1[k], fl[k]) or (bool(torch.isnan(l1[k])) and bool(torch.isnan(fl[k]))), k
    assert all(bool(torch.isfinite(l1[k])) for k in SIX if k != "loss_match")
    fpn_keys = [k for k in g1 if k.startswith("backbone.fpn.")]
    assert len(fpn_keys) == 16 and not any(k.startswith("backbone.") for k in fg)
    for k in fpn_keys:
        assert bool(torch.isfinite(g1[k]).all()) and float(g1[k].abs().max()) > 0, k
    assert not any(k.startswith("backbone.body.") for k in g1)
    assert set(g1) - set(fpn_keys) == set(fg) and len(fg) > 30
    for k in fg:
        assert torch.equal(g1[k], fg[k]), k


def test_model_second_run_is_bit_identical(runs):
    (l1, g1), (l2, g2) = runs["first"], runs["second"]
    assert g1.keys() == g2.keys()
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    assert all(torch.equal(l1[k], l2[k]) or bool(torch.isnan(l1[k])) for k in SIX)


def test_model_fpn_gradients_vs_float64(runs):
    m, cap, (l1, g1) = runs["model"], runs["cap"], runs["first"]
    (feats, sizes, padded), kw = cap["rpn"]
    _, proposals, sizes2, tg = cap["roi"]
    assert list(sizes2) == list(sizes)
    n = len(sizes)
    # the keys, redrawn from the seeds of run_model
    anchors, _ = PR.anchor_grid(*padded)
    rpn_keys = torch.rand((n, anchors.shape[0]), generator=torch.Generator(device=DEV).manual_seed(1), device=DEV).cpu()
    props = [p.detach().cpu() for p in proposals]
    tcpu = [{k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in t.items()} for t in tg]
    pmax = max(len(p) + len(t["boxes"]) for p, t in zip(props, tcpu))
    roi_keys = torch.rand((n, pmax), generator=torch.Generator(device=DEV).manual_seed(2), device=DEV).cpu()
    P = {k: p.detach().cpu().double().requires_grad_(k.startswith("backbone.fpn.")) for k, p in m.named_parameters()
         if not k.startswith("backbone.body.")}
    f = OD.fpn([nchw64(c) for c in cap["body"]], P)
    for k in f:                                                                    # the oracle's pyramid is the device's
        assert float((nchw64(feats[k]) - f[k].detach()).abs().max()) <= 1e-3 * float(f[k].detach().abs().max()), k
    Prpn = {k[len("rpn.head."):]: v for k, v in P.items() if k.startswith("rpn.head.")}
    Proi = {k[len("roi_heads."):]: v for k, v in P.items() if k.startswith("roi_heads.")}
    losses = FR.rpn_losses64(Prpn, list(f.values()), padded, [t["boxes"] for t in tcpu], rpn_keys)
    losses.update(FR.roi_losses64(Proi, [f[k] for k in "0123"], props, tcpu, list(sizes), roi_keys,
                                  m.roi_heads.match_predictor.linear[1].eps, ROI_BATCH, ROI_BATCH // 4))
    for k in SIX:
        a, b = float(l1[k]), float(losses[k])
        print(f"{k}: device {a!r} float64 {b!r}")
        assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-4 * abs(b) + 1e-6, k
    sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
    keys = sorted(k for k in P if k.startswith("backbone.fpn."))
    assert len(keys) == 16
    FR.compare_grads(g1, {k: P[k].grad for k in keys}, keys)


def test_model_sgd_step_refreshes_the_packed_fpn_weights(runs):
    images, targets = runs["images"], runs["targets"]
    m = make_model(True)
    with torch.no_grad():
        feats0 = [o.clone() for o in m.eval().extract_features(images)[0].values()]
        before = m(images)
    m.train()
    run_model(m, images, targets)
    torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.01).step()
    fresh = make_model(True)
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        feats1 = list(m.eval().extract_features(images)[0].values())
        after, want = m(images), fresh.eval()(images)
    assert all(not torch.equal(a, b) for a, b in zip(feats0, feats1))              # the pyramid moved with its weights ...
    assert len(before) != len(after) or any(a[k].shape != b[k].shape or not torch.equal(a[k], b[k])
                                            for a, b in zip(before, after) for k in a)
    assert len(after) == len(want)                                                 # ... and is what a fresh model computes
    for a, b in zip(after, want):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_body_must_be_frozen():
    m = make_model(True)
    next(m.backbone.body.parameters()).requires_grad_(True)
    images, targets = make_model_batch()
    with pytest.raises(NotImplementedError, match="backbone"):
        m(images, targets)


# ------------------------------------------------------------------------------ the modules on maps that require a gradient
def test_rpn_on_leaf_maps_vs_float64():
    from seam_match_rcnn_amd.models import detection as det
    H, W = 128, 160
    torch.manual_seed(1)
    rpn = det.RegionProposalNetwork().to(DEV).train()
    g = torch.Generator().manual_seed(8)
    _, hws = PR.anchor_grid(H, W)
    feats = {k: (torch.randn((2, h, w, 256), generator=g) * 0.5).to(DEV).requires_grad_(True)
             for k, (h, w) in zip(["0", "1", "2", "3", "pool"], hws)}
    gts = [PR.random_gt(g, k, H, W, 20, 100) for k in (2, 3)]
    targets = [dict(boxes=b.to(DEV)) for b in gts]

    def run():
        rpn.sample_generator = torch.Generator(device=DEV).manual_seed(5)
        for f in feats.values():
            f.grad = None
        losses = rpn.training_losses(feats, (H, W), targets)
        sum(losses.values()).backward()
        return {k: f.grad.detach().clone() for k, f in feats.items()}
    got, again = run(), run()
    assert all(torch.equal(got[k], again[k]) for k in got)
    anchors, _ = PR.anchor_grid(H, W)
    keys = torch.rand((2, anchors.shape[0]), generator=torch.Generator(device=DEV).manual_seed(5), device=DEV).cpu()
    P = {k: p.detach().cpu().double() for k, p in rpn.head.named_parameters()}
    f64 = {k: nchw64(f).requires_grad_(True) for k, f in feats.items()}
    sum(FR.rpn_losses64(P, list(f64.values()), (H, W), gts, keys).values()).backward()
    want = {k: (torch.zeros_like(f) if f.grad is None else f.grad).permute(0, 2, 3, 1) for k, f in f64.items()}     # None: a level no ROI uses
    assert sum(float(w.abs().max()) > 0 for w in want.values()) >= 2
    FR.compare_grads(got, want, list(f64))


def test_roi_heads_on_leaf_maps_vs_float64():
    from seam_match_rcnn_amd.models.matchrcnn import NewRoIHeads
    H, W = 128, 160
    torch.manual_seed(2)
    h = NewRoIHeads(NCLS).to(DEV).train()
    g = torch.Generator().manual_seed(9)
    feats = {str(l): (torch.randn((2, H // s, W // s, 256), generator=g) * 0.5).to(DEV).requires_grad_(True)
             for l, s in zip(range(4), (4, 8, 16, 32))}
    props, targets = [], []
    for i in range(2):
        ng = 2 + i
        gt = PR.random_gt(g, ng, H, W, 20, 100)
        masks = torch.zeros((ng, H, W), dtype=torch.uint8)
        for j, b in enumerate(gt.round().to(torch.int64).tolist()):
            masks[j, b[1]:b[3], b[0]:b[2]] = 1
        jit = gt[torch.randint(0, ng, (8,), generator=g)] + (torch.rand((8, 4), generator=g) - 0.5) * 8
        props.append(torch.cat([PR.random_gt(g, 40, H, W, 8, 120), jit]))
        targets.append(dict(boxes=gt, labels=torch.randint(1, NCLS, (ng,), generator=g), masks=masks,
                            pair_ids=torch.randint(0, 3, (ng,), generator=g), styles=torch.randint(1, 3, (ng,), generator=g),
                            sources=torch.tensor([i])))
    dev_t = [{k: v.to(DEV) if k in ("boxes", "labels", "masks") else v for k, v in t.items()} for t in targets]
    shapes = [(H, W)] * 2

    def run():
        h.sample_generator = torch.Generator(device=DEV).manual_seed(6)
        for f in feats.values():
            f.grad = None
        _, losses = h(feats, [p.to(DEV) for p in props], shapes, dev_t)
        sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
        return {k: f.grad.detach().clone() for k, f in feats.items()}
    got, again = run(), run()
    assert all(torch.equal(got[k], again[k]) for k in got)
    pmax = max(len(p) + len(t["boxes"]) for p, t in zip(props, targets))
    keys = torch.rand((2, pmax), generator=torch.Generator(device=DEV).manual_seed(6), device=DEV).cpu()
    P = {k: p.detach().cpu().double() for k, p in h.named_parameters()}
    f64 = {k: nchw64(f).requires_grad_(True) for k, f in feats.items()}
    losses = FR.roi_losses64(P, [f64[k] for k in "0123"], props, targets, shapes, keys, h.match_predictor.linear[1].eps)
    sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
    want = {k: (torch.zeros_like(f) if f.grad is None else f.grad).permute(0, 2, 3, 1) for k, f in f64.items()}     # None: a level no ROI uses
    assert sum(float(w.abs().max()) > 0 for w in want.values()) >= 2
    FR.compare_grads(got, want, list(f64))
