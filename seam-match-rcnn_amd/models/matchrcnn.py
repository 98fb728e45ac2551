"""Image Match R-CNN (phase 1), mirror of reference ``models/matchrcnn.py``.

``matchrcnn_resnet50_fpn(pretrained=False, progress=True, num_classes=91,
pretrained_backbone=True, **kwargs)``                                ref :481-492
eval forward -> per image ``boxes, labels, scores, masks, match_features, w, b``
(no ``roi_features`` key; fallback detection score 1.0)              ref :373-379,451-468

Same pipeline as ``video_matchrcnn`` without the temporal aggregator.  The reference runs
RoIAlign a second time for the match branch on the same boxes (ref :463); the result is
identical, so the 14x14 ROI features are computed once here.

Training branch of the heads (``NewRoIHeads.forward`` with ``self.training``)    ref :333-472
-> ``([], {loss_classifier, loss_box_reg, loss_mask, loss_match})``; backward fills the gradients
of the box, mask and match heads, and of the feature maps when they carry a tape (``autograd.RoIAlignFunction``).

``MatchRCNN.forward(images, targets)`` in training mode adds the RPN's two losses (``detection.RegionProposalNetwork``)
and returns the six-entry loss dict of the reference's phase-1 loop (ref stuffs/engine.py:40-43).  ``backbone.fpn`` learns from
all six losses when its parameters require a gradient (``autograd.FPNFunction``), and so do the bottlenecks of
``backbone.body.layer1..layer4`` (``autograd.BodyFunction``); the stem (``conv1``) learns only with ``train_stem=True`` and is
refused without it.  ``trainable_backbone_layers=3`` is the reference's configuration (torchvision's default of
``resnet_fpn_backbone``: layer2..layer4 learn).
"""
from __future__ import annotations

import numpy as np
import torch
from torch.nn.utils.rnn import pad_sequence

from .. import ops
from ..autograd import (BoxHeadFunction, FastRCNNLossFunction, GatherRowsFunction, MaskHeadFunction, MaskLossFunction,
                        WeightedCE2Function)
from . import detection as det
from .match_head import MatchPredictor
from .video_matchrcnn import TemporalRoIHeads, VideoMatchRCNN, model_urls  # noqa: F401

# non-default RPN / RoI-pool kwargs of the reference (ref :14-29), expressed for this build's ctor
params = {
    'rpn_pre_nms_top_n_train': 2000,
    'rpn_pre_nms_top_n_test': 1000,
    'rpn_post_nms_top_n_test': 4000,
    'rpn_post_nms_top_n_train': 8000,
}


def bb_iou_xywh(dt: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """``pycocotools.mask.iou(dt, gt, [0] * len(gt))`` (maskApi.c bbIou, iscrowd 0): boxes read as xywh, float64,
    o[d, g] = intersection / (area_d + area_g - intersection), 0 where the overlap is empty."""
    dt, gt = np.asarray(dt, np.float64), np.asarray(gt, np.float64)
    o = np.zeros((len(dt), len(gt)))
    for g in range(len(gt)):
        G = gt[g]
        ga = G[2] * G[3]
        for d in range(len(dt)):
            D = dt[d]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            o[d, g] = i / (D[2] * D[3] + ga - i)
    return o


def filter_positive_rows(boxes: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """The rows of one image's positive proposals that the reference's ``filter_proposals`` keeps (match_head.py:441-463),
    quirks included: xyxy boxes go to bbIou, which reads them as xywh; the IoU is rounded to fp32 and squeezed; per GT
    column the proposals are ranked by IoU (descending) and the first min(8 // n_gt, n) ranks are kept, flattened row by
    row (with several GT boxes a proposal can appear more than once); an image with at most one proposal is unchanged."""
    n = len(boxes)
    if n <= 1:
        return np.arange(n, dtype=np.int64)
    ious = torch.from_numpy(bb_iou_xywh(boxes, gt).astype(np.float32)).squeeze()
    top = torch.argsort(ious, descending=True, dim=0)[:min(8 // len(gt), n)].reshape(-1)
    return top.numpy().astype(np.int64)


def match_targets(pairs: np.ndarray, styles: np.ndarray, types: np.ndarray) -> np.ndarray:
    """MatchLossPreTrained's targets (match_head.py:471-493): [n_street, n_shop] int64, 1 where the pair ids and the
    styles agree and both styles are non-zero."""
    pu, su = pairs[types == 0], styles[types == 0]
    ps, ss = pairs[types == 1], styles[types == 1]
    return ((pu[:, None] == ps[None, :]) & (su[:, None] == ss[None, :]) & (ss[None, :] != 0) & (su[:, None] != 0)).astype(np.int64)


def _host(v) -> np.ndarray:
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


class NewRoIHeads(TemporalRoIHeads):
    video = False
    fallback_score = 1.0
    # torchvision RoIHeads training defaults, as MaskRCNN builds them for the reference (ref :41-52)
    batch_size_per_image = 512
    positive_fraction = 0.25
    bbox_reg_weights = (10.0, 10.0, 5.0, 5.0)
    # torch.Generator (on the features' device) that draws the sampler's keys; None: torch's default generator
    sample_generator = None

    def __init__(self, num_classes=91, n_frames=None, *a, **k):
        super().__init__(num_classes, n_frames, *a, **k)
        self.temporal_aggregator = None         # phase-1 model has no aggregator (ref :333-472)

    def forward(self, features, proposals, image_shapes, targets=None):
        if not self.training:
            return super().forward(features, proposals, image_shapes, targets)
        return [], self.training_losses(features, proposals, image_shapes, targets)

    def training_losses(self, features, proposals, image_shapes, targets):
        """The reference's training branch (ref :343-472): ``select_training_samples``, ``fastrcnn_loss``,
        ``maskrcnn_loss`` and the match branch with ``filter_proposals`` + ``MatchLossPreTrained``.

        Sampling: torchvision draws its sample with ``randperm``; here ONE uniform key per candidate is drawn with
        ``sample_generator`` and the sampler keeps the positives / negatives with the smallest keys (lower index on a
        tie): the same distribution as ``randperm(n)[:k]``, but not torchvision's draw, which cannot be reproduced.
        Given the keys the result is deterministic.

        ``loss_match`` is NaN when the kept ROIs hold no street (sources[0] != 1) or no shop image: the reference's
        ``nn.CrossEntropyLoss`` then averages over zero pairs; the match head's gradients are zeros."""
        if targets is None:
            raise ValueError("training mode needs targets")
        for t in targets:
            assert t["boxes"].dtype.is_floating_point, 'target boxes must of float type'
            assert t["labels"].dtype == torch.int64, 'target labels must of int64 type'
            for k in ("boxes", "labels", "masks", "pair_ids", "styles", "sources"):
                if k not in t:
                    raise KeyError(f"training targets need the key '{k}'")
        mods = (self, self.box_head, self.box_predictor, self.mask_head, self.mask_predictor, self.match_predictor)
        if any(det.cdt(m) != torch.float32 for m in mods) or features["0"].dtype != torch.float32:
            raise NotImplementedError("the training branch of the RoI heads is fp32 only: call set_compute_dtype(torch.float32)")
        if isinstance(proposals, tuple):                        # padded RPN form (boxes [N,P,4], counts [N])
            padded, cnt = proposals
            proposals = [padded[i, :c] for i, c in enumerate(cnt.tolist())]
        n = len(proposals)
        if len(targets) != n or len(image_shapes) != n:
            raise ValueError("one target dict and one image size per image are needed")
        dev = features["0"].device
        gt_boxes = [t["boxes"].to(dev, torch.float32).reshape(-1, 4) for t in targets]
        n_gt = [int(b.shape[0]) for b in gt_boxes]
        if min(n_gt) == 0:
            raise ValueError("No ground-truth boxes available for one of the images during training")
        # ---- select_training_samples (ref :146-167): GT boxes appended, match, sample, encode -- seam_roi_sample_f32
        cands = [torch.cat([p.to(dev, torch.float32).reshape(-1, 4), g]) for p, g in zip(proposals, gt_boxes)]
        n_cand = [int(c.shape[0]) for c in cands]
        if max(n_cand) > ops.SAMPLE_MAX_CANDIDATES:
            raise ValueError(f"{max(n_cand)} proposals + GT boxes in one image exceed the sampler's capacity "
                             f"of {ops.SAMPLE_MAX_CANDIDATES}")
        cand = pad_sequence(cands, batch_first=True)
        gtp = pad_sequence(gt_boxes, batch_first=True)
        glp = pad_sequence([t["labels"].to(dev).reshape(-1) for t in targets], batch_first=True)
        keys = torch.rand(cand.shape[:2], generator=self.sample_generator, device=dev)
        counts_dev = torch.tensor(n_cand + n_gt, dtype=torch.int32).to(dev)
        bs = int(self.batch_size_per_image)
        idx, labels, matched, sboxes, stargets, count = ops.roi_sample(
            cand, counts_dev[:n], keys, gtp, glp, counts_dev[n:], bs, int(bs * self.positive_fraction), self.bbox_reg_weights)
        # ONE device->host copy: counts, labels, matched GT, the sampled boxes and the GT boxes (floats as their bits)
        g_max = gtp.shape[1]
        host = torch.cat([count.to(torch.int64), labels, matched, sboxes.reshape(n, 4 * bs).view(torch.int64),
                          gtp.reshape(n, 4 * g_max).view(torch.int64)], 1).cpu()
        h_count = host[:, 0].numpy()
        h_labels = host[:, 2:2 + bs].numpy()
        h_matched = host[:, 2 + bs:2 + 2 * bs].numpy()
        h_boxes = host[:, 2 + 2 * bs:2 + 4 * bs].contiguous().view(torch.float32).reshape(n, bs, 4).numpy()
        h_gt = host[:, 2 + 4 * bs:].contiguous().view(torch.float32).reshape(n, g_max, 4).numpy()
        rows = [int(c) for c in h_count]
        # ---- box branch + fastrcnn_loss (ref :351-359)
        props = [sboxes[i, :c] for i, c in enumerate(rows)]
        box_feats = self.box_roi_pool(features, props, image_shapes)
        bh, bp = self.box_head, self.box_predictor
        class_logits, box_regression = BoxHeadFunction.apply(
            box_feats, bh.fc6.weight, bh.fc6.bias, bh.fc7.weight, bh.fc7.bias,
            bp.cls_score.weight, bp.cls_score.bias, bp.bbox_pred.weight, bp.bbox_pred.bias)
        lab_cat = torch.cat([labels[i, :c] for i, c in enumerate(rows)])
        loss_classifier, loss_box_reg = FastRCNNLossFunction.apply(
            class_logits, box_regression, lab_cat, torch.cat([stargets[i, :c] for i, c in enumerate(rows)]))
        # ---- mask branch + maskrcnn_loss on the positives (ref :383-412); every image has one: its GT boxes match themselves
        pos = [np.flatnonzero(h_labels[i, :c] > 0) for i, c in enumerate(rows)]
        n_pos = [len(p) for p in pos]
        row_off = np.cumsum([0] + rows[:-1])
        pos_rows = torch.from_numpy(np.concatenate([p + o for p, o in zip(pos, row_off)])).to(dev)
        pos_boxes = torch.cat(props)[pos_rows]
        mask_roi = self.mask_roi_pool(features, list(pos_boxes.split(n_pos)), image_shapes)     # [P,14,14,256]
        mh, mp = self.mask_head, self.mask_predictor
        mask_logits = MaskHeadFunction.apply(
            mask_roi, *(t for i in range(1, mh.n + 1) for t in (getattr(mh, f"mask_fcn{i}").weight, getattr(mh, f"mask_fcn{i}").bias)),
            mp.conv5_mask.weight, mp.conv5_mask.bias, mp.mask_fcn_logits.weight, mp.mask_fcn_logits.bias)
        masks = [t["masks"].to(dev) for t in targets]
        for m, g in zip(masks, n_gt):
            if m.dtype != torch.uint8 or m.dim() != 3 or m.shape[0] != g:
                raise ValueError("targets['masks'] must be uint8 [n_gt,H,W]")
        base = np.cumsum([0] + [m.numel() for m in masks[:-1]])
        pos_matched = [h_matched[i, p] for i, p in enumerate(pos)]
        mask_off = np.concatenate([base[i] + pm * masks[i].shape[1] * masks[i].shape[2] for i, pm in enumerate(pos_matched)])
        mask_hw = np.concatenate([np.tile(np.asarray(masks[i].shape[1:], np.int32), (n_pos[i], 1)) for i in range(n)])
        loss_mask = MaskLossFunction.apply(mask_logits, lab_cat[pos_rows], pos_boxes, torch.cat([m.reshape(-1) for m in masks]),
                                           torch.from_numpy(mask_off.astype(np.int64)).to(dev),
                                           torch.from_numpy(mask_hw).to(dev))
        # ---- match branch (ref :414-448): filter_proposals, types from sources[0], MatchPredictor, MatchLossPreTrained
        keep, types, pairs, styles = [], [], [], []
        pos_off = np.cumsum([0] + n_pos[:-1])
        for i in range(n):
            sel = filter_positive_rows(h_boxes[i, pos[i]], h_gt[i, :n_gt[i]])
            mi = pos_matched[i][sel]
            keep.append(sel + pos_off[i])
            types.append(np.full(len(sel), 1 if int(_host(targets[i]["sources"]).reshape(-1)[0]) == 1 else 0, np.int64))
            pairs.append(_host(targets[i]["pair_ids"]).reshape(-1)[mi])
            styles.append(_host(targets[i]["styles"]).reshape(-1)[mi])
        keep, types = np.concatenate(keep), np.concatenate(types)
        if mask_roi.requires_grad:          # `keep` can hold duplicates: their gradients are added in a fixed order
            feats = GatherRowsFunction.apply(mask_roi, keep)
        else:
            feats = mask_roi[torch.from_numpy(keep).to(dev)]
        _, match_logits = self.match_predictor(feats.permute(0, 3, 1, 2), torch.from_numpy(types).to(torch.int32))
        gts = match_targets(np.concatenate(pairs), np.concatenate(styles), types)
        if gts.size == 0:           # no street or no shop ROI: mean over zero pairs, NaN as in the reference
            loss_match = match_logits.sum() * 0.0 + float("nan")
        else:
            loss_match = WeightedCE2Function.apply(match_logits.reshape(-1, 2), torch.from_numpy(gts.reshape(-1)).to(dev),
                                                   torch.ones(2, device=dev))
            loss_match = torch.where(loss_match > 1.0, loss_match * 0.5, loss_match)      # ref :501-502
        return dict(loss_classifier=loss_classifier, loss_box_reg=loss_box_reg, loss_mask=loss_mask, loss_match=loss_match)


class MatchRCNN(VideoMatchRCNN):
    roi_heads_cls = NewRoIHeads

    def __init__(self, backbone, num_classes, **kwargs):
        super().__init__(backbone, num_classes, None, **kwargs)

    def load_saved_matchrcnn(self, sd):
        self.load_state_dict(sd, strict=False)

    def forward(self, images, targets=None):
        """Eval: the detections (``VideoMatchRCNN.forward``).  Training mode with ``targets``: the reference's loss dict
        (ref stuffs/engine.py:40-43) -- loss_classifier, loss_box_reg, loss_mask, loss_match from the RoI heads and
        loss_objectness, loss_rpn_box_reg from the RPN.  ``backward()`` reaches ``rpn.head``, the RoI heads and -- when one of
        its parameters requires a gradient -- the sixteen parameters of ``backbone.fpn`` (through RoIAlign, the RPN's windows
        and the top-down merges) and the conv weights of ``backbone.body.layer1..layer4`` that require one
        (``autograd.BodyFunction``; the tape starts at the first block that holds such a weight).  The stem is opt-in:
        ``backbone.body.conv1.weight`` must be frozen unless ``backbone.body.train_stem`` is set, and then it learns too.  With
        the whole backbone frozen nothing is taped and the launches are unchanged; with only the body frozen the step is the
        FPN-training one."""
        if not self.training or targets is None:
            return super().forward(images, targets)
        body = self.backbone.body
        if body.conv1.weight.requires_grad and not body.train_stem:
            raise NotImplementedError(
                "MatchRCNN training: the stem of the backbone (backbone.body.conv1 and its max-pool) has no backward, so it cannot "
                "learn; freeze it with `model.backbone.body.conv1.weight.requires_grad_(False)` or build the model with "
                "trainable_backbone_layers <= 4 (layer1..layer4 and backbone.fpn may stay trainable; a silent partial gradient "
                "would be worse).  Stem training is opt-in: build the model with `train_stem=True`.")
        body_learns = any(p.requires_grad for p in body.parameters())
        fpn_learns = any(p.requires_grad for p in self.backbone.fpn.parameters())
        if any(det.cdt(m) != torch.float32 for m in (self, self.backbone, self.rpn, self.roi_heads)):
            raise NotImplementedError("MatchRCNN training is fp32 only: call set_compute_dtype(torch.float32)")
        if not isinstance(images, det.PreparedImages):
            images = list(images)
        if len(images) != len(targets):
            raise ValueError("one target dict per image is needed")
        if body_learns or fpn_learns:
            with torch.no_grad():
                x, sizes, orig, padded = self.transform(det.image_list(images))
            spad = x.shape[-1] == 12 and x.shape[1] == padded[0] // 2 + 3      # (training mode: the transform does not pad; told all the same)
            if body_learns:                 # the body through BodyFunction; a frozen FPN still passes its gradient to C2..C5
                c = body(x, spad, taped=True)
            else:                           # body without a tape, the pyramid through FPNFunction
                with torch.no_grad():
                    c = body(x, spad)
            feats = self.backbone.fpn.forward_taped(c)
        else:
            with torch.no_grad():
                feats, sizes, orig, padded = self.extract_features(det.image_list(images))
        dev = feats["0"].device
        tg = []
        for t, s, o in zip(targets, sizes, orig):         # GeneralizedRCNNTransform.resize of the targets [TV]
            t = dict(t, boxes=det.GeneralizedRCNNTransform.rescale_boxes(t["boxes"].to(dev).to(torch.float32), o, s))
            if "masks" in t:
                t["masks"] = resize_masks_nearest(t["masks"].to(dev), s)
            tg.append(t)
        proposals, rpn_losses = self.rpn(feats, sizes, padded, targets=tg)
        _, losses = self.roi_heads(feats, proposals, sizes, tg)
        losses = dict(losses)
        losses.update(rpn_losses)
        return losses


def resize_masks_nearest(masks: torch.Tensor, hw) -> torch.Tensor:
    """``F.interpolate(masks[:, None].float(), size=hw)[:, 0].byte()`` (mode "nearest": source index = floor(dst * in / out) in
    fp32, clamped) as two index selections, which keep the masks uint8 [n,H,W] -> [n,h,w]."""
    h, w = int(hw[0]), int(hw[1])
    if masks.dim() != 3:
        raise ValueError("targets['masks'] must be [n_gt,H,W]")
    if tuple(masks.shape[1:]) == (h, w):
        return masks

    def src(n_in, n_out):
        scale = np.float32(n_in) / np.float32(n_out)
        i = np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64)
        return torch.from_numpy(np.minimum(i, n_in - 1)).to(masks.device)
    return masks.index_select(1, src(masks.shape[1], h)).index_select(2, src(masks.shape[2], w)).contiguous()


def matchrcnn_resnet50_fpn(pretrained=False, progress=True, num_classes=91, pretrained_backbone=True,
                           trainable_backbone_layers=None, train_stem=False, **kwargs):
    """``trainable_backbone_layers``: torchvision's keyword, passed to ``det.resnet_fpn_backbone`` (None: nothing is frozen here;
    3: the reference's layer2..layer4).  ``train_stem``: a trainable ``backbone.body.conv1`` learns (5, or None) instead of being
    refused: ``ResNet50Body.train_stem``."""
    if pretrained:
        pretrained_backbone = False
    backbone = det.resnet_fpn_backbone('resnet50', pretrained_backbone, trainable_layers=trainable_backbone_layers,
                                       train_stem=train_stem)
    model = MatchRCNN(backbone, num_classes, **kwargs)
    if pretrained:
        raise RuntimeError("pretrained=True needs a download (" + model_urls['maskrcnn_resnet50_fpn_coco'] +
                           "); fetch it yourself and call model.load_state_dict(state_dict)")
    return model
