"""Launch wrappers of the detection post-processing kernels: IoU, GT selection, box decoding, NMS, the RPN top-k and the
mask paste / intersection / selection."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _native
from ._ops_common import F32, _ptr, _req, _req_fp, _sfx, _stream

__all__ = ["box_iou", "gt_select", "decode_boxes", "nms_sorted", "rpn_topk_max", "rpn_topk_decode", "paste_masks", "mask_inter",
           "mask_select"]


def box_iou(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """xyxy boxes a [Na,4], b [Nb,4] -> IoU [Na,Nb]."""
    a, b = _req(a), _req(b)
    out = torch.empty((a.shape[0], b.shape[0]), dtype=F32, device=a.device)
    _native.check(_native.lib().seam_box_iou_f32(_ptr(a), _ptr(b), _ptr(out), a.shape[0], b.shape[0], _stream()),
                  "seam_box_iou_f32")
    return out


def gt_select(det_boxes: torch.Tensor, det_scores: torch.Tensor, det_off, gt_boxes: torch.Tensor, gt_off, gt_row: torch.Tensor,
              score_threshold: float):
    """Multi-DF2 ground-truth selection for N images in one launch (``seam_gt_select_f32``; ref evaluate_multiDF2.py:43-57,75-89):
    detections det_boxes [Dtot,4] / det_scores [Dtot] and GT boxes gt_boxes [Gtot,4] (xyxy, the images concatenated, device),
    their boundaries det_off / gt_off [N+1] (host sequences, checked here and uploaded with the launch) and gt_row int32 [N]
    (device; negative = from the end) -> (sel_idx, sel_pos, status) int32 [N] on the device.  Per image: the kept detection
    (score >= threshold, compared in fp32 as torch compares) with the largest pycocotools bbIou against its GT row, first maximum,
    as an index into the image's detections and as a position in the kept subsequence (-1 / -1 when nothing is kept); status
    1 = no GT box, 2 = row out of range (the GT is consulted only when something is kept)."""
    import numpy as np
    det_boxes, det_scores = _req(det_boxes, name="det_boxes"), _req(det_scores, name="det_scores")
    gt_boxes, gt_row = _req(gt_boxes, name="gt_boxes"), _req(gt_row, torch.int32, "gt_row")
    n = gt_row.numel()
    if det_boxes.dim() != 2 or det_boxes.shape[1] != 4 or gt_boxes.dim() != 2 or gt_boxes.shape[1] != 4:
        raise ValueError("gt_select: det_boxes and gt_boxes must be [*,4]")
    if det_scores.numel() != det_boxes.shape[0]:
        raise ValueError("gt_select: det_scores must hold one score per detection")
    det_boxes = det_boxes if det_boxes.data_ptr() % 16 == 0 else det_boxes.clone()      # the kernel reads boxes as float4
    gt_boxes = gt_boxes if gt_boxes.data_ptr() % 16 == 0 else gt_boxes.clone()
    offs = []
    for o, total, what in ((det_off, det_boxes.shape[0], "det_off"), (gt_off, gt_boxes.shape[0], "gt_off")):
        o = np.asarray(o, dtype=np.int64).reshape(-1)
        if o.size != n + 1 or o[0] != 0 or (np.diff(o) < 0).any() or int(o[-1]) > total or total >= 2 ** 31:
            raise ValueError(f"gt_select: {what} must be N+1 non-decreasing int32 offsets from 0 inside the table")
        offs.append(o)
    offs_d = torch.as_tensor(np.concatenate(offs).astype(np.int32)).to(det_boxes.device, non_blocking=False)
    outs = torch.empty((3, n), dtype=torch.int32, device=det_boxes.device)
    _native.check(_native.lib().seam_gt_select_f32(_ptr(det_boxes), _ptr(det_scores), _ptr(offs_d[:n + 1]), _ptr(gt_boxes),
                                                   _ptr(offs_d[n + 1:]), _ptr(gt_row), float(score_threshold), _ptr(outs[0]),
                                                   _ptr(outs[1]), _ptr(outs[2]), n, _stream()),
                  "seam_gt_select_f32")
    return outs[0], outs[1], outs[2]


# ------------------------------------------------------------------------------ detection
def decode_boxes(deltas: torch.Tensor, boxes: torch.Tensor, weights, clip_hw=None) -> torch.Tensor:
    """deltas [N,ncls*4], boxes [N,4] -> [N,ncls*4]; optional clip to (h,w)."""
    deltas, boxes = _req(deltas), _req(boxes)
    n = boxes.shape[0]
    ncls = deltas.shape[1] // 4
    out = torch.empty_like(deltas)
    ch, cw = (float(clip_hw[0]), float(clip_hw[1])) if clip_hw is not None else (0.0, 0.0)
    _native.check(_native.lib().seam_decode_boxes_f32(_ptr(deltas), _ptr(boxes), _ptr(out), n, ncls, *map(float, weights),
                                                      ch, cw, _stream()), "seam_decode_boxes_f32")
    return out


def nms_sorted(boxes: torch.Tensor, thr: float, max_keep: int = 0) -> torch.Tensor:
    """boxes [N,4] or [B,N,4], already sorted by descending score (per image) -> keep mask int32 [N] / [B,N].
    max_keep > 0: only the first ``max_keep`` survivors of each image are marked (== the full result truncated; the scan stops
    there)."""
    boxes = _req(boxes)
    single = boxes.dim() == 2
    b3 = boxes[None] if single else boxes
    bsz, n = b3.shape[0], b3.shape[1]
    keep = torch.empty((bsz, n), dtype=torch.int32, device=boxes.device)
    if n and bsz:
        nb = (n + 63) // 64
        ws = torch.empty((bsz * n * nb,), dtype=torch.int64, device=boxes.device)
        _native.check(_native.lib().seam_nms_sorted_topn_f32(_ptr(b3), _ptr(keep), bsz, n, float(thr), int(max_keep), _ptr(ws),
                                                             _stream()), "seam_nms_sorted_topn_f32")
    return keep[0] if single else keep


def rpn_topk_max() -> int:
    return int(_native.lib().seam_rpn_topk_max())


def rpn_topk_decode(head: torch.Tensor, num_anchors: int, anchors: torch.Tensor, clip_hw: torch.Tensor, k: int,
                    boxes: torch.Tensor, scores: torch.Tensor, offset: int, index: Optional[torch.Tensor] = None) -> None:
    """One pyramid level of RPN ``filter_proposals`` [TV] in one launch (``seam_rpn_topk_decode_f32``).

    head    [N,H,W,A+4A] fp32: the fused RPN head output (objectness logits | deltas per pixel), read in place
    anchors [H*W*A,4]; clip_hw [N,2] (height, width of each resized image), both fp32 on the device
    Writes, for every image, the top-``k`` anchors by logit (descending; ties lowest anchor index first) as decoded + clipped
    boxes into ``boxes[:, offset:offset+k]`` ([N,Ktot,4]) and sigmoid scores into ``scores[:, offset:offset+k]`` ([N,Ktot]);
    ``index`` (int64 [N,Ktot], optional) receives the anchor indices."""
    lib = _native.lib()
    head, anchors, clip_hw = _req(head, name="head"), _req(anchors, name="anchors"), _req(clip_hw, name="clip_hw")
    n_img, h, w, c = head.shape
    a = int(num_anchors)
    if c != 5 * a or anchors.shape != (h * w * a, 4) or clip_hw.shape != (n_img, 2):
        raise ValueError("rpn_topk_decode: head must be [N,H,W,5A], anchors [H*W*A,4], clip_hw [N,2]")
    if (boxes.dtype != F32 or scores.dtype != F32 or not boxes.is_cuda or not boxes.is_contiguous() or not scores.is_contiguous()
            or boxes.dim() != 3 or boxes.shape[0] != n_img or boxes.shape[2] != 4 or tuple(scores.shape) != tuple(boxes.shape[:2])
            or offset < 0 or offset + k > boxes.shape[1]):
        raise ValueError("rpn_topk_decode: boxes [N,Ktot,4] / scores [N,Ktot] fp32 contiguous with room for k rows at offset")
    if index is not None and (index.dtype != torch.int64 or tuple(index.shape) != tuple(scores.shape) or not index.is_contiguous()):
        raise ValueError("rpn_topk_decode: index must be int64 [N,Ktot] contiguous")
    if k < 1 or k > h * w * a or k > int(lib.seam_rpn_topk_max()):
        raise ValueError(f"rpn_topk_decode: k = {k} outside 1..min(n, {int(lib.seam_rpn_topk_max())})")
    obj = C.c_void_p(head.data_ptr())
    dlt = C.c_void_p(head.data_ptr() + 4 * a)
    _native.check(lib.seam_rpn_topk_decode_f32(obj, dlt, _ptr(anchors), _ptr(clip_hw), _ptr(boxes), _ptr(scores), _ptr(index),
                                               n_img, h * w * a, a, k, h * w * c, c, h * w * c, c, boxes.shape[1], offset,
                                               _stream()), "seam_rpn_topk_decode_f32")


def paste_masks(masks: torch.Tensor, boxes: torch.Tensor, hw) -> torch.Tensor:
    """masks [K,1,28,28] prob, boxes [K,4] original-image px -> [K,1,H,W]."""
    masks, boxes = _req(masks), _req(boxes)
    k = masks.shape[0]
    out = torch.empty((k, 1, int(hw[0]), int(hw[1])), dtype=F32, device=masks.device)
    if k:
        _native.check(_native.lib().seam_paste_masks_f32(_ptr(masks), _ptr(boxes), _ptr(out), k, int(hw[0]), int(hw[1]),
                                                         _stream()), "seam_paste_masks_f32")
    return out


def mask_inter(probs: torch.Tensor, boxes: torch.Tensor, gt_masks: torch.Tensor):
    """probs [D,1,28,28] or [D,28,28] (``mask_select``'s output), boxes [D,4] original-image px, gt_masks uint8 [G,H,W]
    (set iff != 0) -> (inter int32 [D,G], det_area int32 [D]): pixel counts of ``paste_masks(probs, boxes, (H, W)) > 0.5``
    against every ground truth and on its own, bit for bit, without the [D,1,H,W] paste (``seam_mask_inter_f32``)."""
    probs, boxes = _req(probs, name="probs"), _req(boxes, name="boxes")
    gt_masks = _req(gt_masks, torch.uint8, "gt_masks")
    d = probs.shape[0]
    if tuple(probs.shape[1:]) not in ((1, 28, 28), (28, 28)) or tuple(boxes.shape) != (d, 4):
        raise ValueError("mask_inter: probs must be [D,1,28,28] or [D,28,28] and boxes [D,4]")
    if gt_masks.dim() != 3:
        raise ValueError("mask_inter: gt_masks must be uint8 [G,H,W]")
    g, h, w = (int(s) for s in gt_masks.shape)
    if h * w >= 2 ** 31:
        raise ValueError("mask_inter: H*W must stay below 2^31")
    inter = torch.empty((d, g), dtype=torch.int32, device=probs.device)
    area = torch.empty((d,), dtype=torch.int32, device=probs.device)
    if d:
        _native.check(_native.lib().seam_mask_inter_f32(_ptr(probs), _ptr(boxes), d, _ptr(gt_masks) if g else None, g, h, w,
                                                        _ptr(inter) if g else None, _ptr(area), _stream()),
                      "seam_mask_inter_f32")
    return inter, area


def mask_select(logits: torch.Tensor, labels: torch.Tensor, ncls: int) -> torch.Tensor:
    """logits [K,14,14,4*ncls] (sub-pixel groups) -> sigmoid prob of channel labels[k]: [K,1,28,28]."""
    logits = _req_fp(logits)
    labels = _req(labels, torch.int64, "labels")
    k = logits.shape[0]
    out = torch.empty((k, 1, 28, 28), dtype=F32, device=logits.device)
    fn = getattr(_native.lib(), "seam_mask_select_" + _sfx(logits.dtype))
    _native.check(fn(_ptr(logits), _ptr(labels), _ptr(out), k, ncls, _stream()), "seam_mask_select")
    return out
