"""GPU: the training branch of ``NewRoIHeads`` (ref models/matchrcnn.py:333-472) -- proposal sampling, the box / mask /
match losses and the head gradients -- against the CPU restatement of ``roi_train_refs.py`` (itself checked against the
reference's own code by ``test_roi_train_references.py``) and float64 autograd.

Bounds.  Sampling is exact: given the same keys the sampled indices, labels and matched GT boxes are identical (box_iou
runs in fp32 in the same expression order on both sides).  The regression targets: dx, dy are the same IEEE operations;
dw, dh take one logf (device, <= 2 ulp) where the CPU takes torch.log, so each target is within 4 ulp of the restatement.
Losses and logits gradients are compared with float64 on the same fp32 inputs: a loss is a mean of n terms summed in
fp32, so its relative error is below n * 2^-24 (plus the few ulp of exp/log per term); gradients per element within
4 ulp of their magnitude plus 2^-24 / n.  Head gradients chain fp32 GEMMs with reductions of length L <= 12544 (fc6):
each gradient tensor is within 2e-3 of float64 in relative Frobenius norm (L * 2^-24 ~ 7.5e-4, doubled for the chain).
A pre-activation within rounding of zero can take the other side of a ReLU in fp32 than in float64, which moves single
elements further, so the elementwise bound is 2e-2 of the tensor's largest element.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_train_refs as RR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64 = torch.float64
ULP = 2.0 ** -23


def _ulp_close(a, b, n_ulp):
    a, b = a.double(), b.double()
    return bool(((a - b).abs() <= n_ulp * ULP * b.abs() + 1e-30).all())


def rand_boxes(g, n, H, W, lo=4.0, hi=300.0):
    xy = torch.rand((n, 2), generator=g) * torch.tensor([W * 0.9, H * 0.9])
    wh = lo + torch.rand((n, 2), generator=g) * (hi - lo)
    b = torch.cat([xy, xy + wh], 1)
    b[:, 2] = b[:, 2].clamp(max=W)
    b[:, 3] = b[:, 3].clamp(max=H)
    b[:, 2:] = torch.max(b[:, 2:], b[:, :2] + 1)
    return b


def near(g, boxes, k, jit=0.1):
    src = boxes[torch.randint(0, len(boxes), (k,), generator=g)]
    wh = (src[:, 2:] - src[:, :2]).repeat(1, 2)
    out = src + (torch.rand((k, 4), generator=g) - 0.5) * jit * wh
    out[:, 2:] = torch.max(out[:, 2:], out[:, :2] + 1)
    return out


# ------------------------------------------------------------------------------ sampler
def _run_sampler(props, gts, gls, keys, batch=512, pos_max=128):
    from seam_match_rcnn_amd import ops
    from torch.nn.utils.rnn import pad_sequence
    cands = [torch.cat([p, g]) for p, g in zip(props, gts)]
    cand = pad_sequence(cands, batch_first=True).to(DEV)
    keyp = pad_sequence(keys, batch_first=True).to(DEV)
    out = ops.roi_sample(cand, torch.tensor([len(c) for c in cands], dtype=torch.int32, device=DEV), keyp,
                         pad_sequence(gts, batch_first=True).to(DEV), pad_sequence(gls, batch_first=True).to(DEV),
                         torch.tensor([len(g) for g in gts], dtype=torch.int32, device=DEV), batch, pos_max)
    return [t.cpu() for t in out]


def _check_sampler(props, gts, gls, keys, batch=512, pos_max=128):
    idx, labels, matched, boxes, targets, count = _run_sampler(props, gts, gls, keys, batch, pos_max)
    again = _run_sampler(props, gts, gls, keys, batch, pos_max)
    assert all(torch.equal(a, b) for a, b in zip((idx, labels, matched, boxes, targets, count), again))
    ref = RR.select_training_samples(props, gts, gls, keys, batch, pos_max)
    for i, r in enumerate(ref):
        c = int(count[i, 0])
        assert c == len(r["idx"]) and int(count[i, 1]) == int((r["labels"] > 0).sum())
        assert torch.equal(idx[i, :c], r["idx"])
        assert torch.equal(labels[i, :c], r["labels"])
        assert torch.equal(matched[i, :c], r["matched"])
        assert torch.equal(boxes[i, :c], r["boxes"])
        assert _ulp_close(targets[i, :c], r["targets"], 4), (targets[i, :c] - r["targets"]).abs().max()
        assert (idx[i, c:] == -1).all() and (targets[i, c:] == 0).all()
    return ref


@pytest.mark.parametrize("n_gt,n_prop,n_near", [(1, 300, 20), (6, 1000, 400), (3, 50, 2), (2, 8000, 600)])
def test_sampler_matches_restatement(n_gt, n_prop, n_near):
    g = torch.Generator().manual_seed(n_gt * 100 + n_prop)
    props, gts, gls, keys = [], [], [], []
    for i in range(3):
        gt = rand_boxes(g, n_gt, 600, 800, 40, 300)
        p = torch.cat([rand_boxes(g, n_prop - n_near, 600, 800), near(g, gt, n_near)])
        props.append(p)
        gts.append(gt)
        gls.append(torch.randint(1, 14, (n_gt,), generator=g))
        keys.append(torch.rand(n_prop + n_gt, generator=g))
    ref = _check_sampler(props, gts, gls, keys)
    npos = [int((r["labels"] > 0).sum()) for r in ref]
    if n_near >= 400:
        assert max(npos) == 128            # more than 128 positives available: capped
    if n_near <= 20:
        assert min(npos) < 128


def test_sampler_iou_exactly_half_and_ties():
    gt = torch.tensor([[0., 0., 10., 10.], [0., 0., 10., 10.], [100., 100., 120., 140.]])
    gl = torch.tensor([2, 7, 5])
    p = torch.tensor([[0., 0., 10., 5.],            # 50 / 100 = 0.5 exactly: foreground
                      [0., 0., 20., 10.],           # 100 / 200 = 0.5
                      [0., 0., 10., 4.9],           # below
                      [100., 100., 120., 120.],     # 400 / 800 = 0.5 with GT 2
                      [300., 300., 310., 310.]])
    keys = torch.full((8,), 0.5)                                            # all keys tie: lower index first
    ref = _check_sampler([p], [gt], [gl], [keys], batch=4, pos_max=3)
    assert ref[0]["idx"].tolist() == [0, 1, 2, 3]
    assert ref[0]["labels"].tolist() == [2, 2, 0, 5]                        # IoU 0.5 is foreground; GT 0 / GT 1 tie: the first
    assert float(RR.box_iou_f32(gt, p)[0, 0]) == 0.5
    keys = torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0.25, 0.25, 0.25])        # the appended GT boxes have the smallest keys
    ref = _check_sampler([p], [gt], [gl], [keys], batch=6, pos_max=3)
    assert ref[0]["idx"].tolist() == [2, 4, 5, 6, 7] and ref[0]["labels"].tolist() == [0, 0, 2, 2, 5]


def test_sampler_refuses_too_many_candidates():
    from seam_match_rcnn_amd import ops
    z = torch.zeros((1, 16385, 4), device=DEV)
    with pytest.raises(ValueError, match="capacity"):
        ops.roi_sample(z, torch.tensor([16385], dtype=torch.int32, device=DEV), torch.zeros((1, 16385), device=DEV),
                       torch.zeros((1, 1, 4), device=DEV), torch.ones((1, 1), dtype=torch.int64, device=DEV),
                       torch.ones(1, dtype=torch.int32, device=DEV))


# ------------------------------------------------------------------------------ losses
def test_fastrcnn_loss_and_gradients_vs_float64():
    from seam_match_rcnn_amd import ops
    g = torch.Generator().manual_seed(3)
    for r, ncls in ((1, 14), (300, 14), (4096, 14), (77, 91)):
        cl = torch.randn((r, ncls), generator=g) * 3
        br = torch.randn((r, 4 * ncls), generator=g) * 0.3
        lab = torch.randint(0, ncls, (r,), generator=g)
        lab[torch.rand(r, generator=g) < 0.6] = 0
        tg = torch.randn((r, 4), generator=g) * 0.3
        loss, dcl, dbr = ops.fastrcnn_loss_fwd_bwd(cl.to(DEV), br.to(DEV), lab.to(DEV), tg.to(DEV))
        c64, b64 = cl.double().requires_grad_(True), br.double().requires_grad_(True)
        l1, l2 = RR.fastrcnn_loss(c64, b64, lab, tg.double())
        (gc,) = torch.autograd.grad(l1, c64)
        gb = torch.autograd.grad(l2, b64)[0] if (lab > 0).any() else torch.zeros_like(b64)
        loss = loss.cpu().double()
        assert abs(float(loss[0] - l1)) <= 4 * r * 2 ** -24 * float(l1) + 1e-7
        assert abs(float(loss[1] - l2)) <= 4 * r * 2 ** -24 * float(l2) + 1e-7
        assert float((dcl.cpu().double() - gc).abs().max()) <= 8 * ULP * float(gc.abs().max()) + 2 ** -24 / r
        assert float((dbr.cpu().double() - gb).abs().max()) <= 8 * ULP * max(float(gb.abs().max()), 1.0 / r)


def _mask_case(g, p, ncls, H, W, big=False):
    masks = (torch.rand((3, H, W), generator=g) < 0.5).to(torch.uint8)
    masks[:, H // 4: 3 * H // 4, W // 4: 3 * W // 4] = 1
    rois = rand_boxes(g, p, H, W, 2.0, 900.0 if big else 200.0)
    if big:
        rois[0] = torch.tensor([0.0, 0.0, float(W), float(H)])
    matched = torch.randint(0, 3, (p,), generator=g)
    labels = torch.randint(1, ncls, (p,), generator=g)
    logits = torch.randn((p, 14, 14, 4 * ncls), generator=g) * 2
    return masks, rois, matched, labels, logits


def test_mask_loss_and_gradient_vs_float64():
    from seam_match_rcnn_amd import ops
    g = torch.Generator().manual_seed(5)
    for p, ncls, H, W, big in ((1, 14, 64, 80, False), (40, 14, 300, 400, False), (6, 3, 820, 1000, True)):
        masks, rois, matched, labels, logits = _mask_case(g, p, ncls, H, W, big)
        off = matched.to(torch.int64) * H * W
        hw = torch.tensor([[H, W]] * p, dtype=torch.int32)
        loss, dl = ops.mask_loss_fwd_bwd(logits.to(DEV), labels.to(DEV), rois.to(DEV), masks.reshape(-1).to(DEV),
                                         off.to(DEV), hw.to(DEV))
        loss2, dl2 = ops.mask_loss_fwd_bwd(logits.to(DEV), labels.to(DEV), rois.to(DEV), masks.reshape(-1).to(DEV),
                                           off.to(DEV), hw.to(DEV))
        assert torch.equal(loss, loss2) and torch.equal(dl, dl2)
        t28 = torch.from_numpy(RR.project_masks(masks.numpy(), rois.numpy(), matched.numpy()))
        l64 = logits.double().requires_grad_(True)
        ref = RR.maskrcnn_loss(l64, labels, t28)
        (gref,) = torch.autograd.grad(ref, l64)
        n = p * 784
        # targets: within RR.target_error of the float64 ones
        terr = RR.target_error(rois.numpy(), H, W)
        assert abs(float(loss.cpu()) - float(ref)) <= 8 * n * 2 ** -24 * float(ref) + terr * float(l64.abs().mean()) \
            + 1e-6, (float(loss), float(ref))
        assert float((dl.cpu().double() - gref).abs().max()) <= (terr + 16 * ULP) / n
        assert int((dl.cpu() != 0).sum()) <= n


# ------------------------------------------------------------------------------ heads, end to end
NCLS = 14


def make_heads(seed=0):
    from seam_match_rcnn_amd.models.matchrcnn import NewRoIHeads
    torch.manual_seed(seed)
    h = NewRoIHeads(NCLS)
    with torch.no_grad():
        for m in (h.mask_head, h.mask_predictor, h.match_predictor):
            for p in m.parameters():
                if p.dim() > 1:
                    p.mul_(1.5)
    return h.to(DEV).train()


def make_batch(seed, n_img=8, n_prop=2000, H=512, W=640, shop=(0, 1, 0, 1, 0, 1, 1, 0), n_near=4):
    g = torch.Generator().manual_seed(seed)
    feats = {str(l): (torch.randn((n_img, H // s, W // s, 256), generator=g) * 0.5).to(DEV)
             for l, s in zip(range(4), (4, 8, 16, 32))}
    props, targets = [], []
    for i in range(n_img):
        ng = 1 + (i * 5 + seed) % 4
        gt = rand_boxes(g, ng, H, W, 30, 300)
        masks = torch.zeros((ng, H, W), dtype=torch.uint8)
        for j, b in enumerate(gt.round().to(torch.int64).tolist()):
            masks[j, b[1]:b[3], b[0]:b[2]] = (torch.rand((b[3] - b[1], b[2] - b[0]), generator=g) < 0.8).to(torch.uint8)
        props.append(torch.cat([rand_boxes(g, n_prop - n_near * ng, H, W), near(g, gt, n_near * ng, 0.3)]).to(DEV))
        targets.append(dict(boxes=gt.to(DEV), labels=torch.randint(1, NCLS, (ng,), generator=g).to(DEV), masks=masks.to(DEV),
                            pair_ids=torch.randint(0, 3, (ng,), generator=g), styles=torch.randint(0, 3, (ng,), generator=g),
                            sources=torch.tensor([shop[i % len(shop)]])))
    return feats, props, [(H, W)] * n_img, targets


def run_heads(h, feats, props, shapes, targets, seed):
    h.sample_generator = torch.Generator(device=DEV).manual_seed(seed)
    h.zero_grad(set_to_none=True)
    res, losses = h(feats, props, shapes, targets)
    assert res == [] and list(losses) == ["loss_classifier", "loss_box_reg", "loss_mask", "loss_match"]
    assert all(v.dim() == 0 and v.dtype == torch.float32 and v.is_cuda for v in losses.values())
    sum(losses.values()).backward()           # a NaN loss_match contributes zero gradients, as in the reference
    grads = {k: p.grad.detach().clone() for k, p in h.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in losses.items()}, grads


TRAINED = ["box_head.fc6", "box_head.fc7", "box_predictor.cls_score", "box_predictor.bbox_pred"] + \
    [f"mask_head.mask_fcn{i}" for i in range(1, 5)] + ["mask_predictor.conv5_mask", "mask_predictor.mask_fcn_logits"]


def restate(h, feats, props, shapes, targets, seed):
    """float64 CPU restatement of the whole training branch on the device's RoIAlign outputs -> (losses, grads)."""
    n = len(props)
    pmax = max(len(p) + len(t["boxes"]) for p, t in zip(props, targets))
    keys = torch.rand((n, pmax), generator=torch.Generator(device=DEV).manual_seed(seed), device=DEV).cpu()
    samp = RR.select_training_samples([p.cpu() for p in props], [t["boxes"].cpu() for t in targets],
                                      [t["labels"].cpu() for t in targets], list(keys))
    P = {k: p.detach().cpu().double().requires_grad_(True) for k, p in h.named_parameters()}
    with torch.no_grad():
        bx = h.box_roi_pool(feats, [s["boxes"].to(DEV) for s in samp], shapes).cpu().double()
    x = bx.permute(0, 3, 1, 2).reshape(bx.shape[0], -1)
    x = F.relu(F.linear(x, P["box_head.fc6.weight"], P["box_head.fc6.bias"]))
    x = F.relu(F.linear(x, P["box_head.fc7.weight"], P["box_head.fc7.bias"]))
    cl = F.linear(x, P["box_predictor.cls_score.weight"], P["box_predictor.cls_score.bias"])
    br = F.linear(x, P["box_predictor.bbox_pred.weight"], P["box_predictor.bbox_pred.bias"])
    lab = torch.cat([s["labels"] for s in samp])
    l_cls, l_box = RR.fastrcnn_loss(cl, br, lab, torch.cat([s["targets"] for s in samp]).double())
    pos = [torch.nonzero(s["labels"] > 0).view(-1) for s in samp]
    pboxes = [s["boxes"][p] for s, p in zip(samp, pos)]
    with torch.no_grad():
        mr = h.mask_roi_pool(feats, [b.to(DEV) for b in pboxes], shapes).cpu().double().permute(0, 3, 1, 2)
    y = mr
    for i in range(1, 5):
        y = F.relu(F.conv2d(y, P[f"mask_head.mask_fcn{i}.weight"], P[f"mask_head.mask_fcn{i}.bias"], padding=1))
    y = F.relu(F.conv_transpose2d(y, P["mask_predictor.conv5_mask.weight"], P["mask_predictor.conv5_mask.bias"], stride=2))
    y = F.conv2d(y, P["mask_predictor.mask_fcn_logits.weight"], P["mask_predictor.mask_fcn_logits.bias"])
    plab = torch.cat([s["labels"][p] for s, p in zip(samp, pos)])
    t28 = np.concatenate([RR.project_masks(t["masks"].cpu().numpy(), b.numpy(), s["matched"][p].numpy())
                          for t, b, s, p in zip(targets, pboxes, samp, pos)])
    l_mask = F.binary_cross_entropy_with_logits(y[torch.arange(len(plab)), plab], torch.from_numpy(t28))
    kp, km, rows = RR.filter_proposals(pboxes, [t["boxes"].cpu() for t in targets], [s["matched"][p] for s, p in zip(samp, pos)])
    off = np.cumsum([0] + [len(p) for p in pos[:-1]])
    sel = torch.cat([r + int(o) for r, o in zip(rows, off)])
    types = torch.cat([torch.full((len(p),), int(int(t["sources"][0]) == 1), dtype=torch.int32) for p, t in zip(kp, targets)])
    z = mr[sel]
    for i in (0, 2, 4, 6):
        z = F.relu(F.conv2d(z, P[f"match_predictor.conv_seq.{i}.weight"], P[f"match_predictor.conv_seq.{i}.bias"]))
    z = F.relu(F.avg_pool2d(z, 6)).flatten(1)
    z = F.linear(z, P["match_predictor.linear.0.weight"], P["match_predictor.linear.0.bias"])
    z = F.batch_norm(z, None, None, P["match_predictor.linear.1.weight"], P["match_predictor.linear.1.bias"], True, 0.0,
                     h.match_predictor.linear[1].eps)
    x5 = F.linear((z[types == 0][:, None] - z[types == 1][None]) ** 2, P["match_predictor.last.weight"],
                  P["match_predictor.last.bias"])
    l_match = RR.match_loss(x5, [t["pair_ids"] for t in targets], [t["styles"] for t in targets], types, km)
    losses = dict(loss_classifier=l_cls, loss_box_reg=l_box, loss_mask=l_mask, loss_match=l_match)
    sum(losses.values()).backward()
    return {k: v.detach() for k, v in losses.items()}, {k: p.grad for k, p in P.items() if p.grad is not None}


def _compare(losses, grads, rl, rg, tol=2e-3):
    for k in rl:
        a, b = float(losses[k]), float(rl[k])
        if np.isnan(b):
            assert np.isnan(a), k
        else:
            assert abs(a - b) <= 1e-4 * abs(b) + 1e-6, (k, a, b)
    for k, gref in rg.items():
        if float(gref.abs().max()) == 0.0:
            continue
        d = grads[k].cpu().double() - gref
        w = rg.get(k[:-4] + "weight") if k.endswith(".bias") else None
        if w is not None and float(gref.abs().max()) < 1e-6 * float(w.abs().max()):
            # exactly zero in exact arithmetic (the Linear bias in front of BatchNorm1d on batch statistics; the BatchNorm
            # shift, which the translation-invariant (a - b)^2 pairs cannot see): what is left on both sides is rounding
            assert float(d.abs().max()) <= 1e-4 * float(w.abs().max()), k
            continue
        fro = float(d.norm() / gref.norm())
        err = float(d.abs().max())
        assert fro <= tol, (k, fro)
        assert err <= 10 * tol * float(gref.abs().max()) + 1e-9, (k, err, float(gref.abs().max()))


def test_head_gradients_vs_float64_small():
    h = make_heads(1)
    feats, props, shapes, targets = make_batch(11, n_img=2, n_prop=120, shop=(0, 1))
    losses, grads = run_heads(h, feats, props, shapes, targets, seed=5)
    for name in TRAINED:
        assert f"{name}.weight" in grads and f"{name}.bias" in grads, name
    assert all(k in grads for k, _ in h.match_predictor.named_parameters(prefix="match_predictor"))
    rl, rg = restate(make_heads(1), feats, props, shapes, targets, seed=5)
    _compare(losses, grads, rl, rg)


def test_end_to_end_df2_batch_matches_restatement_and_is_bit_identical():
    h = make_heads(2)
    feats, props, shapes, targets = make_batch(21)
    losses, grads = run_heads(h, feats, props, shapes, targets, seed=9)
    losses2, grads2 = run_heads(h, feats, props, shapes, targets, seed=9)
    assert all(torch.equal(losses[k], losses2[k]) for k in losses)
    assert grads.keys() == grads2.keys() and all(torch.equal(grads[k], grads2[k]) for k in grads)
    rl, rg = restate(make_heads(2), feats, props, shapes, targets, seed=9)
    _compare(losses, grads, rl, rg)
    # the padded proposal form that detect() accepts gives the same result
    pmax = max(len(p) for p in props)
    padded = torch.zeros((len(props), pmax, 4), device=DEV)
    for i, p in enumerate(props):
        padded[i, :len(p)] = p
    losses3, grads3 = run_heads(h, feats, (padded, torch.tensor([len(p) for p in props], device=DEV)), shapes, targets, seed=9)
    assert all(torch.equal(losses[k], losses3[k]) for k in losses)


def test_five_sgd_steps_lower_the_loss():
    h = make_heads(3)
    feats, props, shapes, targets = make_batch(31, n_img=4, n_prop=500, shop=(0, 1))
    opt = torch.optim.SGD(h.parameters(), lr=0.01, momentum=0.9)
    totals = []
    for _ in range(6):
        h.sample_generator = torch.Generator(device=DEV).manual_seed(4)
        opt.zero_grad()
        _, losses = h(feats, props, shapes, targets)
        total = sum(losses.values())
        totals.append(float(total))
        if len(totals) <= 5:
            total.backward()
            opt.step()
    assert all(np.isfinite(totals)) and totals[-1] < totals[0], totals


def test_no_gt_raises_and_street_only_gives_the_reference_nan():
    h = make_heads(4)
    feats, props, shapes, targets = make_batch(41, n_img=2, n_prop=100, shop=(0, 0))
    losses, grads = run_heads(h, feats, props, shapes, targets, seed=1)
    assert torch.isnan(losses["loss_match"]) and all(torch.isfinite(losses[k]) for k in ("loss_classifier", "loss_box_reg",
                                                                                           "loss_mask"))
    assert float(grads["match_predictor.last.weight"].abs().max()) == 0.0
    bad = [dict(t) for t in targets]
    bad[1]["boxes"] = torch.zeros((0, 4), device=DEV)
    bad[1]["labels"] = torch.zeros((0,), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="No ground-truth boxes"):
        h(feats, props, shapes, bad)


def test_training_is_fp32_only_and_model_forward_still_raises():
    from seam_match_rcnn_amd.models import detection as det
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    h = make_heads(5)
    feats, props, shapes, targets = make_batch(51, n_img=2, n_prop=50)
    det.set_compute_dtype(h, torch.float16)
    with pytest.raises(NotImplementedError, match="fp32"):
        h(feats, props, shapes, targets)
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS).train()
    with pytest.raises(NotImplementedError):
        m([torch.zeros(3, 32, 32)])
