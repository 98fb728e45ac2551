"""Float64 references of the FPN-training adjoints (``csrc/seam_fpn_train.hip``) and the fixtures their tests share.

The three small adjoints -- RoIAlign backward, the RPN window scatter, the top-down merge backward -- are restated as EXPLICIT
scatters in float64.  One pass returns, per output element, the sum, the sum of the absolute contributions ``A`` and the number
of non-zero contributions ``T``: every weight is non-negative, so any fp32 evaluation order of the same terms stays within
``(T + c) * 2^-24 * A`` of the float64 sum (c covers the roundings of forming a weight and of the final scale).

Sample positions, validity, clamps and bilinear fractions of RoIAlign come from ``oracle.detection._axis_samples`` -- fp32, the
operation sequence of torchvision -- and ``hy = 1 - ly`` is taken in fp32 as well (what the oracle and the kernels do); only the
products and sums are float64.  ``test_fpn_train_references.py`` ties this scatter to torch autograd of ``oracle.detection.roi_align``.
"""
import math

import numpy as np
import torch

from oracle import detection as OD

U = 2.0 ** -24          # unit roundoff of fp32

# the pyramid of the RoIAlign tests: a 80 x 96 image
IMG_HW = (80, 96)
ROI_HWS = [(20, 24), (10, 12), (5, 6), (3, 3)]
ROI_SCALES = [0.25, 0.125, 0.0625, 0.03125]
K_MIN = 2


BOUNDARY_STEPS = (-16, -12, -8, -1, 0, 1)      # fp32 steps away from 112 / 224 / 448; LevelMapper's + 1e-6 puts the boundary ~10 below


def _step(v, j):
    v = np.float32(v)
    for _ in range(abs(j)):
        v = np.nextafter(v, np.float32(np.inf if j > 0 else -np.inf))
    return float(v)


def roi_set(image1: str = "some"):
    """About 40 ROIs [K,5] fp32 on the 80 x 96 image (two images).  ``image1``: "some" -- image 1 owns ROIs of levels 0..2
    only (none of level 3); "none" -- every ROI belongs to image 0.  Rows 11..28 are the level-boundary squares."""
    rois = [
        [0, 500., 500., 520., 520.],            # far outside: every sample skipped
        [0, -10., 20., 15., 50.],               # over the left edge
        [0, 30., -12., 60., 14.],               # over the top edge
        [0, 80., 20., 110., 60.],               # over the right edge
        [0, 20., 65., 50., 95.],                # over the bottom edge
        [0, -30., -30., 2., 3.],                # a corner: samples between -1 and 0 are clamped, those below -1 skipped
        [0, 40.2, 30.3, 40.9, 31.1],            # smaller than a pixel of level 0: the extent clamp
        [0, 0., 0., 96., 80.],                  # the whole map
        [0, 12., 9., 47., 38.],
        [0, 12., 9., 47., 38.],                 # an exact duplicate
        [0, 94., 78., 96., 80.],                # the last pixel: row / column collapse
    ]
    # level boundaries: squares with sqrt(area) at 112 / 224 / 448 and at fp32 neighbours on both sides of the boundary
    for s in (112., 224., 448.):
        for j in BOUNDARY_STEPS:
            rois.append([0, 0., 0., _step(s, j), _step(s, j)])
    if image1 == "some":
        rois.append([1, 0., 0., _step(112., -8), _step(112., -8)])
        rois.append([1, 0., 0., _step(224., -12), _step(224., -12)])
    g = torch.Generator().manual_seed(1234)
    for i in range(12):
        cx, cy = float(torch.rand((), generator=g)) * 96, float(torch.rand((), generator=g)) * 80
        w, h = 2 + float(torch.rand((), generator=g)) * 60, 2 + float(torch.rand((), generator=g)) * 50
        rois.append([i % 2 if image1 == "some" else 0, cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2])
    if image1 == "some":
        rois.append([1, 12., 9., 47., 38.])     # the duplicate's box once more, in the other image
    return torch.tensor(rois, dtype=torch.float32)


def explicit_levels(k: int, image1_no_level3: torch.Tensor):
    """Given levels that spread the ROIs over all four maps (image 1 still gets no level 3)."""
    lv = torch.arange(k, dtype=torch.int64) % 4
    return torch.where(image1_no_level3 & (lv == 3), torch.zeros_like(lv), lv).to(torch.int32)


def _axis_table(start, extent, pooled, sr, size):
    """W [size, pooled] float64 (summed weights of a bin's samples on a pixel) and the count of non-zero terms."""
    valid, lo, hi, frac = OD._axis_samples(start, extent, pooled, sr, size)
    hw = (1.0 - frac).double().numpy()            # fp32 subtraction, as on the device
    lw = frac.double().numpy()
    wt, ct = np.zeros((size, pooled)), np.zeros((size, pooled))
    for g in range(pooled * sr):
        if not bool(valid[g]):
            continue
        p = g // sr
        for idx, w in ((int(lo[g]), hw[g]), (int(hi[g]), lw[g])):
            wt[idx, p] += w
            ct[idx, p] += 1.0 if w != 0.0 else 0.0
    return wt, ct


def roi_align_bwd_scatter(dout, rois, levels, hws, scales, sr, n_images):
    """dout float64 [K,P,P,C] (NHWC), rois fp32 [K,5], levels int [K] -> per level (sum, A, T), float64 [N,H,W,C] each."""
    dout = dout.double().numpy()
    k, p = dout.shape[0], dout.shape[1]
    res = [[np.zeros((n_images, h, w, dout.shape[3])) for _ in range(3)] for h, w in hws]
    for i in range(k):
        b = float(rois[i, 0])
        l = int(levels[i])
        if not (math.isfinite(b) and 0 <= b < n_images) or not 0 <= l < 4:
            continue
        b = int(b)
        h, w = hws[l]
        x1, y1, x2, y2 = (rois[i, j].to(torch.float32) * scales[l] for j in (1, 2, 3, 4))
        wy, cy = _axis_table(y1, torch.clamp(y2 - y1, min=1.0), p, sr, h)
        wx, cx = _axis_table(x1, torch.clamp(x2 - x1, min=1.0), p, sr, w)
        s, a, t = res[l]
        s[b] += np.einsum("yp,xq,pqc->yxc", wy, wx, dout[i]) / (sr * sr)
        a[b] += np.einsum("yp,xq,pqc->yxc", wy, wx, np.abs(dout[i])) / (sr * sr)
        t[b] += np.einsum("yp,xq->yx", cy, cx)[:, :, None]
    return [tuple(torch.from_numpy(v) for v in r) for r in res]


def roi_align_bwd_autograd(dout, rois, levels, hws, scales, sr, n_images):
    """The same gradient by torch autograd of ``oracle.detection.roi_align`` in float64 -> per level [N,H,W,C]."""
    k, p, c = dout.shape[0], dout.shape[1], dout.shape[3]
    outs = []
    for l, (h, w) in enumerate(hws):
        f = torch.zeros((n_images, c, h, w), dtype=torch.float64, requires_grad=True)
        sel = torch.nonzero(torch.as_tensor(levels).to(torch.int64) == l).squeeze(1)
        if sel.numel():
            o = OD.roi_align(f, rois[sel], scales[l], p, sr)
            o.backward(dout[sel].double().permute(0, 3, 1, 2))
            outs.append(f.grad.permute(0, 2, 3, 1).contiguous())
        else:
            outs.append(torch.zeros((n_images, h, w, c), dtype=torch.float64))
    return outs


# ------------------------------------------------------------------------------ RPN windows
SCATTER_HWS = [(6, 7), (3, 4), (2, 2)]


def scatter_rows():
    """37 rows (image, level, y, x) on the three maps above, two images."""
    rows = [
        [0, 0, 0, 0], [0, 0, 0, 6], [0, 0, 5, 0], [0, 0, 5, 6],      # the four corners: the padding taps are dropped
        [0, 0, 2, 3], [0, 0, 2, 3], [0, 0, 2, 3],                    # one pixel three times (three anchor slots)
        [0, 0, 2, 4], [0, 0, 3, 5],                                  # horizontally and diagonally adjacent
        [0, 7, 1, 1],                                                # a level that does not exist: nothing
        [1, 2, 0, 0], [1, 2, 1, 1], [1, 2, 1, 1],                    # the 2 x 2 map: every window covers all of it
        [1, 1, 0, 3], [1, 1, 2, 0], [0, 1, 1, 2], [0, 1, 1, 1],
    ]
    g = torch.Generator().manual_seed(99)
    while len(rows) < 37:
        l = int(torch.randint(0, 3, (), generator=g))
        h, w = SCATTER_HWS[l]
        rows.append([int(torch.randint(0, 2, (), generator=g)), l, int(torch.randint(0, h, (), generator=g)),
                     int(torch.randint(0, w, (), generator=g))])
    return torch.tensor(rows, dtype=torch.int32)


def scatter_patches_ref(dpatch, rows, hws, n_images):
    """dpatch [M,3,3,C], rows int [M,4] -> per level (sum, A, T), float64 [N,H,W,C]."""
    dp = dpatch.double().numpy()
    c = dp.shape[3]
    res = [[np.zeros((n_images, h, w, c)) for _ in range(3)] for h, w in hws]
    for m, (img, lvl, y, x) in enumerate(rows.tolist()):
        if not (0 <= img < n_images and 0 <= lvl < len(hws)):
            continue
        h, w = hws[lvl]
        if not (0 <= y < h and 0 <= x < w):
            continue
        s, a, t = res[lvl]
        for r in range(3):
            for q in range(3):
                yy, xx = y + r - 1, x + q - 1
                if 0 <= yy < h and 0 <= xx < w:
                    s[img, yy, xx] += dp[m, r, q]
                    a[img, yy, xx] += np.abs(dp[m, r, q])
                    t[img, yy, xx] += 1.0
    return [tuple(torch.from_numpy(v) for v in r) for r in res]


def gather_patches_ref(feats, rows):
    """The forward: windows [M,3,3,C] float64 of NHWC maps, zeros outside and for a row out of range."""
    c = feats[0].shape[3]
    out = torch.zeros((rows.shape[0], 3, 3, c), dtype=torch.float64)
    for m, (img, lvl, y, x) in enumerate(rows.tolist()):
        if not (0 <= img < feats[0].shape[0] and 0 <= lvl < len(feats)):
            continue
        h, w = feats[lvl].shape[1:3]
        if not (0 <= y < h and 0 <= x < w):
            continue
        for r in range(3):
            for q in range(3):
                yy, xx = y + r - 1, x + q - 1
                if 0 <= yy < h and 0 <= xx < w:
                    out[m, r, q] = feats[lvl][img, yy, xx].double()
    return out


# ------------------------------------------------------------------------------ top-down merge
def nearest_src(n_out: int, n_in: int) -> np.ndarray:
    """ATen upsample_nearest: source index of every destination index, floor(dst * (in / out)) in fp32, clamped."""
    scale = np.float32(n_in) / np.float32(n_out)
    return np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)


def upsample_add_bwd_ref(dlat, top_hw, base=None):
    """dlat [N,H,W,C] -> (sum, A, T) float64 [N,Ht,Wt,C]; ``base`` counts as one more contribution."""
    d = dlat.double().numpy()
    n, h, w, c = d.shape
    ht, wt = top_hw
    sy, sx = nearest_src(h, ht), nearest_src(w, wt)
    s, a, t = (np.zeros((n, ht, wt, c)) for _ in range(3))
    for y in range(h):
        for x in range(w):
            s[:, sy[y], sx[x]] += d[:, y, x]
            a[:, sy[y], sx[x]] += np.abs(d[:, y, x])
            t[:, sy[y], sx[x]] += 1.0
    if base is not None:
        b = base.double().numpy()
        s, a, t = s + b, a + np.abs(b), t + 1.0
    return tuple(torch.from_numpy(v) for v in (s, a, t))


# ------------------------------------------------------------------------------ comparison rules of the project, restated
def compare_grads(grads, refs, keys, tol=2e-3):
    """``_compare`` of tests/test_gpu_roi_train.py for gradient tensors: relative Frobenius error <= tol and largest error
    <= 10 tol of the reference's largest element (a pre-activation within rounding of zero can take the other side of a
    ReLU).  Every figure is printed before it is asserted."""
    for k in keys:
        gref = refs[k].double()
        d = grads[k].detach().cpu().double() - gref
        big = float(gref.abs().max())
        fro = float(d.norm() / gref.norm()) if big > 0 else float(d.norm())
        err = float(d.abs().max())
        print(f"{k}: rel Frobenius {fro:.3e} max err {err:.3e} of {big:.3e}")
        assert fro <= tol, (k, fro)
        assert err <= 10 * tol * big + 1e-9, (k, err, big)


def wgrad_close(got, want, rtol=2e-4, atol_frac=2e-5):
    """``close`` of tests/test_gpu_train.py: the project's tolerance of a weight gradient."""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_frac * (float(np.abs(want).max()) + 1e-30) + 1e-9)


def within(dev, ref, extra):
    """|dev - sum| <= (T + extra) * 2^-24 * A per element; returns the largest error / bound ratio (0/0 counts as 0)."""
    s, a, t = ref
    err = (dev.detach().cpu().double() - s).abs()
    bound = (t + extra) * U * a
    assert bool((err <= bound).all()), (float(err.max()), float((err - bound).max()))
    assert bool((dev.detach().cpu()[a == 0] == 0).all())
    return float((err / bound.clamp(min=1e-300)).max())


# ------------------------------------------------------------------------------ float64 restatements down to the pyramid
def roi_align64(feats_nchw, boxes, image_sizes, pooled, sampling_ratio=2):
    """MultiScaleRoIAlign as ``oracle.detection.multiscale_roi_align`` but in the dtype of the maps and differentiable:
    feats_nchw four maps [N,C,H,W], boxes a list of [k_i,4] -> [sum k_i, C, P, P]."""
    rois = torch.cat([torch.cat([torch.full((b.shape[0], 1), float(i)), b.to(torch.float32)], 1) for i, b in enumerate(boxes)], 0)
    scales = OD.infer_scales([f.shape[-2:] for f in feats_nchw], image_sizes)
    k_min, k_max = int(-math.log2(scales[0])), int(-math.log2(scales[-1]))
    lv = OD.map_levels(rois[:, 1:], k_min, k_max)
    parts, order = [], []
    for l, (f, s) in enumerate(zip(feats_nchw, scales)):
        sel = torch.nonzero(lv == l).squeeze(1)
        if sel.numel():
            parts.append(OD.roi_align(f, rois[sel], s, pooled, sampling_ratio))
            order.append(sel)
    return torch.cat(parts)[torch.argsort(torch.cat(order))]


def rpn_losses64(P, feats_nchw, padded_hw, gt_boxes, keys):
    """The dense float64 RPN restatement of tests/test_gpu_rpn_train.py::restate on given (differentiable) maps: P the six head
    parameters (float64), feats_nchw the five maps, gt_boxes per image (resized frame, CPU), keys [N,A] the sampler's draws."""
    import rpn_train_refs as PR
    anchors, _ = PR.anchor_grid(*padded_hw)
    samp = [PR.assign_and_sample(anchors, g, keys[i]) for i, g in enumerate(gt_boxes)]
    obj, dlt = PR.dense_head(feats_nchw, P)
    o = torch.cat([obj[i, s["idx"]] for i, s in enumerate(samp)])
    d = torch.cat([dlt[i, s["idx"]] for i, s in enumerate(samp)])
    lo, lb = PR.rpn_losses(o, d, torch.cat([s["labels"] for s in samp]), torch.cat([s["targets"] for s in samp]).double())
    return dict(loss_objectness=lo, loss_rpn_box_reg=lb)


def roi_losses64(P, feats_nchw, proposals, targets, image_sizes, keys, bn_eps, batch=512, pos_max=128):
    """The float64 restatement of ``NewRoIHeads.training_losses`` (tests/test_gpu_roi_train.py::restate) with RoIAlign inside
    the tape: P the heads' parameters (float64, names of ``NewRoIHeads.named_parameters``), feats_nchw the four maps,
    proposals / targets on the CPU, keys [N, >= proposals + GT] the sampler's draws, batch / pos_max the sampler's sizes."""
    import torch.nn.functional as F

    import roi_train_refs as RR
    samp = RR.select_training_samples(proposals, [t["boxes"] for t in targets], [t["labels"] for t in targets], list(keys),
                                      batch, pos_max)
    bx = roi_align64(feats_nchw, [s["boxes"] for s in samp], image_sizes, 7)
    x = bx.reshape(bx.shape[0], -1)
    x = F.relu(F.linear(x, P["box_head.fc6.weight"], P["box_head.fc6.bias"]))
    x = F.relu(F.linear(x, P["box_head.fc7.weight"], P["box_head.fc7.bias"]))
    cl = F.linear(x, P["box_predictor.cls_score.weight"], P["box_predictor.cls_score.bias"])
    br = F.linear(x, P["box_predictor.bbox_pred.weight"], P["box_predictor.bbox_pred.bias"])
    lab = torch.cat([s["labels"] for s in samp])
    l_cls, l_box = RR.fastrcnn_loss(cl, br, lab, torch.cat([s["targets"] for s in samp]).double())
    pos = [torch.nonzero(s["labels"] > 0).view(-1) for s in samp]
    pboxes = [s["boxes"][p] for s, p in zip(samp, pos)]
    mr = roi_align64(feats_nchw, pboxes, image_sizes, 14)
    y = mr
    for i in range(1, 5):
        y = F.relu(F.conv2d(y, P[f"mask_head.mask_fcn{i}.weight"], P[f"mask_head.mask_fcn{i}.bias"], padding=1))
    y = F.relu(F.conv_transpose2d(y, P["mask_predictor.conv5_mask.weight"], P["mask_predictor.conv5_mask.bias"], stride=2))
    y = F.conv2d(y, P["mask_predictor.mask_fcn_logits.weight"], P["mask_predictor.mask_fcn_logits.bias"])
    plab = torch.cat([s["labels"][p] for s, p in zip(samp, pos)])
    t28 = np.concatenate([RR.project_masks(t["masks"].numpy(), b.numpy(), s["matched"][p].numpy())
                          for t, b, s, p in zip(targets, pboxes, samp, pos)])
    l_mask = F.binary_cross_entropy_with_logits(y[torch.arange(len(plab)), plab], torch.from_numpy(t28))
    kp, km, rows = RR.filter_proposals(pboxes, [t["boxes"] for t in targets], [s["matched"][p] for s, p in zip(samp, pos)])
    off = np.cumsum([0] + [len(p) for p in pos[:-1]])
    sel = torch.cat([r + int(o) for r, o in zip(rows, off)])
    types = torch.cat([torch.full((len(p),), int(int(t["sources"][0]) == 1), dtype=torch.int32) for p, t in zip(kp, targets)])
    z = mr[sel]
    for i in (0, 2, 4, 6):
        z = F.relu(F.conv2d(z, P[f"match_predictor.conv_seq.{i}.weight"], P[f"match_predictor.conv_seq.{i}.bias"]))
    z = F.relu(F.avg_pool2d(z, 6)).flatten(1)
    z = F.linear(z, P["match_predictor.linear.0.weight"], P["match_predictor.linear.0.bias"])
    z = F.batch_norm(z, None, None, P["match_predictor.linear.1.weight"], P["match_predictor.linear.1.bias"], True, 0.0, bn_eps)
    x5 = F.linear((z[types == 0][:, None] - z[types == 1][None]) ** 2, P["match_predictor.last.weight"],
                  P["match_predictor.last.bias"])
    l_match = RR.match_loss(x5, [t["pair_ids"] for t in targets], [t["styles"] for t in targets], types, km)
    return dict(loss_classifier=l_cls, loss_box_reg=l_box, loss_mask=l_mask, loss_match=l_match)
