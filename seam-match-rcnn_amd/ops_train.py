"""Launch wrappers of the training kernels that are not convolutions: the weight gradient and its chunking, the match head's
backward, the RoI-head and RPN sampling and losses, the FPN / body / stem adjoints, and the host side of the fused SGD step's chunk table."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _native
from ._ops_common import F32, _ptr, _req, _stream
from .ops_heads import PackedNLB

__all__ = ["conv_wgrad", "conv_wgrad_chunked", "colsum", "avgpool_relu_bwd", "bn1d_train_fwd", "ce2_fwd_bwd", "bn1d_bwd",
           "pair_logits_bwd", "nlb_attnpool_bwd", "nlb_block_bwd", "SAMPLE_MAX_CANDIDATES", "roi_sample",
           "fastrcnn_loss_fwd_bwd", "mask_loss_fwd_bwd", "RPN_MAX_ANCHORS", "rpn_max_gt", "rpn_match", "rpn_sample",
           "rpn_gather_patches", "rpn_loss_fwd_bwd", "roi_align_bwd", "rpn_scatter_patches", "upsample_add_bwd",
           "subsample_add_bwd_", "subsample_add_bwd", "relu_mask_add", "maxpool3s2_relu_bwd",
           "sgd_chunk_table"]


def conv_wgrad(x: torch.Tensor, dy: torch.Tensor, R: int, S: int, stride: int = 1, pad: int = 0,
               out_hw: Optional[Sequence[int]] = None) -> torch.Tensor:
    """x NHWC [N,H,W,C], dy NHWC [N,Ho,Wo,K] -> dW in PyTorch OIHW layout [K,C,R,S] (fp32 MFMA, split over pixels).
    ``out_hw``: dy belongs to a conv cropped to its first ``out_hw`` output positions (``conv2d(..., out_hw=)``); it is read as it
    lies (``seam_conv_wgrad_crop_f32``)."""
    lib = _native.lib()
    x, dy = _req(x, name="x"), _req(dy, name="dy")
    n, h, w, c = x.shape
    k = dy.shape[-1]
    m = dy.numel() // k
    if out_hw is not None:
        ho, wo = int(out_hw[0]), int(out_hw[1])
        if tuple(dy.shape[:3]) != (n, ho, wo) or ho > (h + 2 * pad - R) // stride + 1 or wo > (w + 2 * pad - S) // stride + 1:
            raise ValueError(f"conv_wgrad: dy {tuple(dy.shape)} is not the output of this conv on x {tuple(x.shape)} cropped to {ho} x {wo}")
    dw = torch.empty((k, c, R, S), dtype=F32, device=x.device)
    ws = torch.empty((int(lib.seam_conv_wgrad_workspace_floats(m, c, k, R, S)),), dtype=F32, device=x.device)
    if out_hw is not None:
        _native.check(lib.seam_conv_wgrad_crop_f32(_ptr(x), _ptr(dy), _ptr(dw), n, h, w, c, k, R, S, stride, pad, ho, wo, _ptr(ws),
                                                   _stream()), "seam_conv_wgrad_crop_f32")
        return dw
    _native.check(lib.seam_conv_wgrad_f32(_ptr(x), _ptr(dy), _ptr(dw), n, h, w, c, k, R, S, stride, pad, _ptr(ws), _stream()),
                  "seam_conv_wgrad_f32")
    return dw


# seam_conv_wgrad_f32 indexes an operand with 32 bits: one of 2^31 bytes or more is split over images (FPN level 0 at
# 800x1333 passes that at 32 images).  A module constant so that a test can lower it.
WGRAD_MAX_OPERAND_BYTES = (1 << 31) - 1


def conv_wgrad_chunked(x: torch.Tensor, dy: torch.Tensor, R: int, S: int, stride: int = 1, pad: int = 0,
                       out_hw: Optional[Sequence[int]] = None) -> torch.Tensor:
    """``conv_wgrad`` for operands of any size: the images are split into equal consecutive chunks (the last may be shorter) whose
    operands stay within ``WGRAD_MAX_OPERAND_BYTES``, and the partial dW are added in chunk order -- a fixed order, so two calls
    give the same bits.  One chunk is exactly ``conv_wgrad``."""
    x, dy = _req(x, name="x"), _req(dy, name="dy")
    n = x.shape[0]
    if dy.shape[0] != n or n == 0:
        raise ValueError("conv_wgrad_chunked: x and dy need the same, non-zero number of images")
    per = max(x[0].numel(), dy[0].numel()) * 4
    if per > WGRAD_MAX_OPERAND_BYTES:
        raise ValueError(f"conv_wgrad_chunked: one image's operand ({per} bytes) exceeds the limit of {WGRAD_MAX_OPERAND_BYTES}")
    step = max(1, min(n, WGRAD_MAX_OPERAND_BYTES // per))
    if step >= n:
        return conv_wgrad(x, dy, R, S, stride, pad, out_hw)
    dw = None
    for i in range(0, n, step):
        part = conv_wgrad(x[i:i + step], dy[i:i + step], R, S, stride, pad, out_hw)
        dw = part if dw is None else dw.add_(part)
    return dw


def colsum(x: torch.Tensor) -> torch.Tensor:
    """[..., K] -> [K] sum over all leading dims (bias gradients)."""
    x = _req(x)
    k = x.shape[-1]
    m = x.numel() // k
    lib = _native.lib()
    out = torch.empty((k,), dtype=F32, device=x.device)
    ws = torch.empty((int(lib.seam_colsum_workspace_floats(m, k)),), dtype=F32, device=x.device)
    _native.check(lib.seam_colsum_f32(_ptr(x), _ptr(out), m, k, _ptr(ws), _stream()), "seam_colsum_f32")
    return out


def avgpool_relu_bwd(dpool: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """dpool [N,C], y NHWC [N,H,W,C] (post-ReLU conv output) -> dy [N,H,W,C]."""
    dpool, y = _req(dpool), _req(y)
    n, h, w, c = y.shape
    dy = torch.empty_like(y)
    _native.check(_native.lib().seam_avgpool_relu_bwd_f32(_ptr(dpool), _ptr(y), _ptr(dy), n, h * w, c, _stream()),
                  "seam_avgpool_relu_bwd_f32")
    return dy


def bn1d_train_fwd(x, gamma, beta, running_mean, running_var, momentum: float, eps: float):
    """BatchNorm1d with batch statistics; running buffers (or None) updated in place -> (y, save_mean, save_invstd)."""
    x = _req(x)
    m, f = x.shape
    if m < 2:
        raise ValueError("Expected more than 1 value per channel when training, got input size " + str(tuple(x.shape)))
    y = torch.empty_like(x)
    mean = torch.empty((f,), dtype=F32, device=x.device)
    inv = torch.empty((f,), dtype=F32, device=x.device)
    _native.check(_native.lib().seam_bn1d_train_fwd_f32(_ptr(x), _ptr(_req(gamma.detach())), _ptr(_req(beta.detach())), _ptr(y),
                                                        _ptr(mean), _ptr(inv), _ptr(running_mean), _ptr(running_var), m, f,
                                                        float(momentum), float(eps), _stream()), "seam_bn1d_train_fwd_f32")
    return y, mean, inv


def ce2_fwd_bwd(logits: torch.Tensor, target: torch.Tensor, weight: torch.Tensor):
    """Weighted 2-class cross entropy (mean): logits [n,2], target int64 [n], weight [2] -> (loss [], dlogits [n,2])."""
    logits = _req(logits)
    target = _req(target.to(logits.device), torch.int64, "target")
    weight = _req(weight.to(logits.device))
    loss = torch.empty((), dtype=F32, device=logits.device)
    dl = torch.empty_like(logits)
    _native.check(_native.lib().seam_ce2_fwd_bwd_f32(_ptr(logits), _ptr(target), _ptr(weight), _ptr(loss), _ptr(dl),
                                                     logits.shape[0], _stream()), "seam_ce2_fwd_bwd_f32")
    return loss, dl


def bn1d_bwd(dy, x, save_mean, save_invstd, gamma, frozen: bool = False):
    dy, x = _req(dy), _req(x)
    m, f = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty((f,), dtype=F32, device=x.device)
    db = torch.empty((f,), dtype=F32, device=x.device)
    _native.check(_native.lib().seam_bn1d_bwd_f32(_ptr(dy), _ptr(x), _ptr(save_mean), _ptr(save_invstd), _ptr(_req(gamma.detach())),
                                                  _ptr(dx), _ptr(dg), _ptr(db), m, f, int(frozen), _stream()), "seam_bn1d_bwd_f32")
    return dx, dg, db


def pair_logits_bwd(a, b, w, g):
    """Gradients of ``pair_logits``: g [Q,G,2] -> (da [Q,256], db [G,256], dw [2,256], dbias [2])."""
    a, b, w, g = _req(a), _req(b), _req(w.detach()), _req(g)
    q, gg, d = a.shape[0], b.shape[0], a.shape[1]
    da, db = torch.zeros_like(a), torch.zeros_like(b)
    dw = torch.zeros((2, d), dtype=F32, device=a.device)
    dbias = torch.zeros((2,), dtype=F32, device=a.device)
    if q and gg:
        _native.check(_native.lib().seam_pair_logits_bwd_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(g), _ptr(da), _ptr(db), _ptr(dw),
                                                             _ptr(dbias), q, gg, d, _stream()), "seam_pair_logits_bwd_f32")
    return da, db, dw, dbias


def nlb_attnpool_bwd(seq, t_stride, s_stride, lens, n_seq, t_max, pk: "PackedNLB", dout, use_nlb=1):
    """Gradients of ``nlb_attnpool``: dout [S,256] -> (dseq like seq, [11 parameter gradients in the reference's layouts:
    theta.w, theta.b, phi.w, phi.b, g.w, g.b, concat_project.w, W.w, W.b, attention_scorer.w, attention_scorer.b])."""
    lib = _native.lib()
    seq, dout = _req(seq, name="seq"), _req(dout, name="dout")
    dev = seq.device
    dseq = torch.zeros_like(seq)
    shapes = [(128, 256, 1), (128,), (128, 256, 1), (128,), (128, 256, 1), (128,), (1, 256, 1, 1), (256, 128, 1), (256,), (1, 256), (1,)]
    grads = [torch.zeros(sh, dtype=F32, device=dev) for sh in shapes]
    if n_seq:
        ws = torch.empty((int(lib.seam_nlb_bwd_workspace_floats(n_seq, t_max)),), dtype=F32, device=dev)
        arr = (C.c_void_p * 11)(*[g.data_ptr() for g in grads])
        _native.check(lib.seam_nlb_attnpool_bwd_f32(_ptr(seq), t_stride, s_stride, _ptr(_req(lens, torch.int32, "lens")), n_seq, t_max,
                                                    _ptr(pk.w_proj_t), _ptr(pk.b_proj), _ptr(pk.w_cat), _ptr(pk.w_out_t),
                                                    _ptr(pk.b_out), _ptr(pk.w_att), _ptr(pk.b_att), _ptr(dout), _ptr(dseq), arr,
                                                    _ptr(ws), int(use_nlb), _stream()), "seam_nlb_attnpool_bwd_f32")
    return dseq, grads


def nlb_block_bwd(seq, t_stride, s_stride, lens, n_seq, t_max, pk: "PackedNLB", dz, dz_t_stride, dz_s_stride, use_nlb=2):
    """Gradients of the non-local block alone (the ``z`` output of ``nlb_attnpool``): dz rows -> (dseq like seq, [9 parameter
    gradients: theta.w, theta.b, phi.w, phi.b, g.w, g.b, concat_project.w, W.w, W.b])."""
    lib = _native.lib()
    seq, dz = _req(seq, name="seq"), _req(dz, name="dz")
    dev = seq.device
    dseq = torch.zeros_like(seq)
    shapes = [(128, 256, 1), (128,), (128, 256, 1), (128,), (128, 256, 1), (128,), (1, 256, 1, 1), (256, 128, 1), (256,)]
    grads = [torch.zeros(sh, dtype=F32, device=dev) for sh in shapes]
    if n_seq:
        ws = torch.empty((int(lib.seam_nlb_bwd_workspace_floats(n_seq, t_max)),), dtype=F32, device=dev)
        arr = (C.c_void_p * 9)(*[g.data_ptr() for g in grads])
        _native.check(lib.seam_nlb_block_bwd_f32(_ptr(seq), t_stride, s_stride, _ptr(_req(lens, torch.int32, "lens")), n_seq, t_max,
                                                 _ptr(pk.w_proj_t), _ptr(pk.b_proj), _ptr(pk.w_cat), _ptr(pk.w_out_t), _ptr(pk.b_out),
                                                 _ptr(dz), dz_t_stride, dz_s_stride, _ptr(dseq), arr, _ptr(ws), int(use_nlb), _stream()),
                      "seam_nlb_block_bwd_f32")
    return dseq, grads


# ------------------------------------------------------------------------------ RoI heads training branch (csrc/seam_roi_train.hip)
SAMPLE_MAX_CANDIDATES = 16384      # per image: rpn_post_nms_top_n_train (8000) + the GT boxes fit


def roi_sample(cand: torch.Tensor, n_cand: torch.Tensor, keys: torch.Tensor, gt_boxes: torch.Tensor, gt_labels: torch.Tensor,
               n_gt: torch.Tensor, batch: int = 512, pos_max: int = 128, weights=(10.0, 10.0, 5.0, 5.0)):
    """select_training_samples [TV] on padded per-image arrays: cand [N,P,4] (proposals then GT boxes), n_cand int32 [N],
    keys [N,P], gt_boxes [N,G,4], gt_labels int64 [N,G], n_gt int32 [N] -> (idx, labels, matched int64 [N,batch],
    boxes, targets [N,batch,4], count int32 [N,2] = (sampled rows, positives)); rows past the count hold -1 / 0."""
    cand, keys, gt_boxes = _req(cand, name="cand"), _req(keys, name="keys"), _req(gt_boxes, name="gt_boxes")
    n_cand, n_gt = _req(n_cand, torch.int32, "n_cand"), _req(n_gt, torch.int32, "n_gt")
    gt_labels = _req(gt_labels, torch.int64, "gt_labels")
    n, p = cand.shape[0], cand.shape[1]
    g = gt_boxes.shape[1]
    if p > SAMPLE_MAX_CANDIDATES:
        raise ValueError(f"roi_sample: {p} candidates per image exceed the kernel's capacity of {SAMPLE_MAX_CANDIDATES}")
    if tuple(keys.shape) != (n, p) or tuple(gt_labels.shape) != (n, g) or n_cand.numel() != n or n_gt.numel() != n:
        raise ValueError("roi_sample: inconsistent shapes")
    dev = cand.device
    idx = torch.empty((n, batch), dtype=torch.int64, device=dev)
    labels = torch.empty_like(idx)
    matched = torch.empty_like(idx)
    boxes = torch.empty((n, batch, 4), dtype=F32, device=dev)
    targets = torch.empty_like(boxes)
    count = torch.empty((n, 2), dtype=torch.int32, device=dev)
    wx, wy, ww, wh = (float(w) for w in weights)
    _native.check(_native.lib().seam_roi_sample_f32(_ptr(cand), _ptr(n_cand), _ptr(keys), _ptr(gt_boxes), _ptr(gt_labels), _ptr(n_gt),
                                                    n, p, g, int(batch), int(pos_max), wx, wy, ww, wh, _ptr(idx), _ptr(labels),
                                                    _ptr(matched), _ptr(boxes), _ptr(targets), _ptr(count), _stream()),
                  "seam_roi_sample_f32")
    return idx, labels, matched, boxes, targets, count


def fastrcnn_loss_fwd_bwd(class_logits: torch.Tensor, box_regression: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor):
    """fastrcnn_loss [TV] -> (loss [2] = (classifier, box_reg), dclass_logits, dbox_regression) for a unit upstream gradient."""
    class_logits, box_regression = _req(class_logits, name="class_logits"), _req(box_regression, name="box_regression")
    labels, targets = _req(labels, torch.int64, "labels"), _req(targets, name="targets")
    r, ncls = class_logits.shape
    if tuple(box_regression.shape) != (r, 4 * ncls) or labels.numel() != r or tuple(targets.shape) != (r, 4):
        raise ValueError("fastrcnn_loss_fwd_bwd: inconsistent shapes")
    loss = torch.empty((2,), dtype=F32, device=class_logits.device)
    dcls, dbox = torch.empty_like(class_logits), torch.empty_like(box_regression)
    _native.check(_native.lib().seam_fastrcnn_loss_fwd_bwd_f32(_ptr(class_logits), _ptr(box_regression), _ptr(labels), _ptr(targets),
                                                               r, ncls, _ptr(loss), _ptr(dcls), _ptr(dbox), _stream()),
                  "seam_fastrcnn_loss_fwd_bwd_f32")
    return loss, dcls, dbox


def mask_loss_fwd_bwd(logits: torch.Tensor, labels: torch.Tensor, rois: torch.Tensor, masks: torch.Tensor, mask_off: torch.Tensor,
                      mask_hw: torch.Tensor):
    """maskrcnn_loss [TV] on the sub-pixel logits [P,14,14,4*ncls]: labels int64 [P], rois [P,4] in the masks' frame, masks a flat
    uint8 buffer holding each ROI's GT mask at byte mask_off[k] (int64 [P]) with size mask_hw[k] (int32 [P,2])
    -> (loss [], dlogits like logits) for a unit upstream gradient."""
    logits, rois = _req(logits, name="logits"), _req(rois, name="rois")
    labels, masks = _req(labels, torch.int64, "labels"), _req(masks, torch.uint8, "masks")
    mask_off, mask_hw = _req(mask_off, torch.int64, "mask_off"), _req(mask_hw, torch.int32, "mask_hw")
    p = logits.shape[0]
    ncls = logits.shape[-1] // 4
    if tuple(logits.shape) != (p, 14, 14, 4 * ncls) or labels.numel() != p or tuple(rois.shape) != (p, 4) or mask_off.numel() != p \
            or tuple(mask_hw.shape) != (p, 2):
        raise ValueError("mask_loss_fwd_bwd: inconsistent shapes")
    loss = torch.empty((), dtype=F32, device=logits.device)
    dl = torch.empty_like(logits)
    ws = torch.empty((max(p, 1),), dtype=F32, device=logits.device)
    _native.check(_native.lib().seam_mask_loss_fwd_bwd_f32(_ptr(logits), _ptr(labels), _ptr(rois), _ptr(masks), _ptr(mask_off),
                                                           _ptr(mask_hw), p, ncls, _ptr(loss), _ptr(dl), _ptr(ws), _stream()),
                  "seam_mask_loss_fwd_bwd_f32")
    return loss, dl


# ------------------------------------------------------------------------------ RPN training branch (csrc/seam_rpn_train.hip)
RPN_MAX_ANCHORS = 1 << 20          # per image


def rpn_max_gt() -> int:
    return int(_native.lib().seam_rpn_max_gt())


def rpn_match(anchors: torch.Tensor, gt_boxes: torch.Tensor, n_gt: torch.Tensor, fg_thresh: float = 0.7, bg_thresh: float = 0.3):
    """Matcher(fg, bg, allow_low_quality_matches=True) [TV]: anchors [A,4] (shared by the batch), gt_boxes [N,G,4], n_gt int32 [N]
    -> (labels int8 [N,A]: -1 ignored / 0 background / 1 foreground, matched int32 [N,A]: the argmax GT of a foreground anchor)."""
    anchors, gt_boxes = _req(anchors, name="anchors"), _req(gt_boxes, name="gt_boxes")
    n_gt = _req(n_gt, torch.int32, "n_gt")
    if anchors.dim() != 2 or anchors.shape[1] != 4 or gt_boxes.dim() != 3 or gt_boxes.shape[2] != 4 or n_gt.numel() != gt_boxes.shape[0]:
        raise ValueError("rpn_match: inconsistent shapes")
    a, (n, g) = anchors.shape[0], gt_boxes.shape[:2]
    lib = _native.lib()
    nws = int(lib.seam_rpn_match_workspace_floats(n, a, g))
    if nws <= 0:
        raise ValueError(f"rpn_match: N = {n}, A = {a}, G = {g} outside the kernel's caps (A <= {RPN_MAX_ANCHORS}, G <= {rpn_max_gt()})")
    dev = anchors.device
    labels = torch.empty((n, a), dtype=torch.int8, device=dev)
    matched = torch.empty((n, a), dtype=torch.int32, device=dev)
    ws = torch.empty((nws,), dtype=F32, device=dev)
    _native.check(lib.seam_rpn_match_f32(_ptr(anchors), _ptr(gt_boxes), _ptr(n_gt), n, a, g, float(fg_thresh), float(bg_thresh),
                                         _ptr(labels), _ptr(matched), _ptr(ws), _stream()), "seam_rpn_match_f32")
    return labels, matched


def rpn_sample(labels: torch.Tensor, matched: torch.Tensor, keys: torch.Tensor, anchors: torch.Tensor, gt_boxes: torch.Tensor,
               batch: int = 256, pos_max: int = 128):
    """BalancedPositiveNegativeSampler [TV] with the key rule of ``roi_sample`` on ``rpn_match``'s outputs: keys [N,A]
    -> (idx, labels, matched int64 [N,batch] in ascending anchor order, -1 past the count; targets [N,batch,4] =
    BoxCoder((1,1,1,1)).encode on the foreground rows; count int32 [N,2] = (rows, foreground rows))."""
    labels, matched = _req(labels, torch.int8, "labels"), _req(matched, torch.int32, "matched")
    keys, anchors, gt_boxes = _req(keys, name="keys"), _req(anchors, name="anchors"), _req(gt_boxes, name="gt_boxes")
    n, a = labels.shape
    g = gt_boxes.shape[1]
    if tuple(matched.shape) != (n, a) or tuple(keys.shape) != (n, a) or tuple(anchors.shape) != (a, 4) or gt_boxes.shape[0] != n:
        raise ValueError("rpn_sample: inconsistent shapes")
    lib = _native.lib()
    nws = int(lib.seam_rpn_sample_workspace_bytes(n, int(batch)))
    if nws <= 0 or a > RPN_MAX_ANCHORS:
        raise ValueError(f"rpn_sample: N = {n}, A = {a}, batch = {batch} outside the kernel's caps")
    dev = labels.device
    idx = torch.empty((n, batch), dtype=torch.int64, device=dev)
    slab, smat = torch.empty_like(idx), torch.empty_like(idx)
    targets = torch.empty((n, batch, 4), dtype=F32, device=dev)
    count = torch.empty((n, 2), dtype=torch.int32, device=dev)
    ws = torch.empty((nws,), dtype=torch.uint8, device=dev)
    _native.check(lib.seam_rpn_sample_f32(_ptr(labels), _ptr(matched), _ptr(keys), _ptr(anchors), _ptr(gt_boxes), n, a, g, int(batch),
                                          int(pos_max), _ptr(idx), _ptr(slab), _ptr(smat), _ptr(targets), _ptr(count), _ptr(ws),
                                          _stream()), "seam_rpn_sample_f32")
    return idx, slab, smat, targets, count


def rpn_gather_patches(feats: Sequence[torch.Tensor], rows: torch.Tensor) -> torch.Tensor:
    """feats: the NHWC fp32 pyramid maps [N,H_l,W_l,C]; rows int32 [M,4] = (image, level, y, x) -> [M,3,3,C], the 3x3 window of
    each row's pixel with the conv's zero padding."""
    feats = [_req(f, name="feats") for f in feats]
    rows = _req(rows, torch.int32, "rows")
    n, c = feats[0].shape[0], feats[0].shape[3]
    if rows.dim() != 2 or rows.shape[1] != 4 or any(f.dim() != 4 or f.shape[0] != n or f.shape[3] != c for f in feats):
        raise ValueError("rpn_gather_patches: inconsistent shapes")
    m, l = rows.shape[0], len(feats)
    out = torch.empty((m, 3, 3, c), dtype=F32, device=rows.device)
    maps = (C.c_void_p * l)(*[f.data_ptr() for f in feats])
    hw = (C.c_int * (2 * l))(*[int(v) for f in feats for v in f.shape[1:3]])
    _native.check(_native.lib().seam_rpn_gather_patches_f32(maps, hw, _ptr(rows), m, n, l, c, _ptr(out), _stream()),
                  "seam_rpn_gather_patches_f32")
    return out


def rpn_loss_fwd_bwd(head: torch.Tensor, slot: torch.Tensor, labels: torch.Tensor, targets: torch.Tensor, num_anchors: int,
                     grad_cols: int = 32):
    """RegionProposalNetwork.compute_loss [TV] on the sampled rows: head [M,>=5A], slot int32 [M], labels int64 [M], targets [M,4]
    -> (loss [2] = (objectness, rpn_box_reg), grad [M,grad_cols]) for a unit upstream gradient."""
    head, targets = _req(head, name="head"), _req(targets, name="targets")
    slot, labels = _req(slot, torch.int32, "slot"), _req(labels, torch.int64, "labels")
    m = head.shape[0]
    if head.dim() != 2 or slot.numel() != m or labels.numel() != m or tuple(targets.shape) != (m, 4):
        raise ValueError("rpn_loss_fwd_bwd: inconsistent shapes")
    loss = torch.empty((2,), dtype=F32, device=head.device)
    grad = torch.empty((m, int(grad_cols)), dtype=F32, device=head.device)
    _native.check(_native.lib().seam_rpn_loss_fwd_bwd_f32(_ptr(head), _ptr(slot), _ptr(labels), _ptr(targets), m, int(num_anchors),
                                                          head.shape[1], int(grad_cols), _ptr(loss), _ptr(grad), _stream()),
                  "seam_rpn_loss_fwd_bwd_f32")
    return loss, grad


# ------------------------------------------------------------------------------ FPN training: the adjoints (csrc/seam_fpn_train.hip)
def roi_align_bwd(dout: torch.Tensor, rois: torch.Tensor, feat_hws: Sequence[Sequence[int]], n_images: int, scales: Sequence[float],
                  sampling_ratio: int = 2, k_min: int = 2, levels: Optional[torch.Tensor] = None) -> list:
    """Adjoint of ``roi_align``: dout NHWC fp32 [K,P,P,C], rois fp32 [K,5], feat_hws the four (H_l, W_l) -> the four gradient
    maps [N,H_l,W_l,C], written completely (zeros where no ROI reaches).  Fixed summation order: two calls give the same bits."""
    dout, rois = _req(dout, name="dout"), _req(rois, name="rois")
    if dout.dim() != 4 or dout.shape[1] != dout.shape[2] or rois.dim() != 2 or rois.shape[1] != 5 or rois.shape[0] != dout.shape[0]:
        raise ValueError("roi_align_bwd: dout must be [K,P,P,C] and rois [K,5]")
    if len(feat_hws) != 4 or len(scales) != 4:
        raise ValueError("roi_align_bwd: four levels are needed")
    k, p, c = dout.shape[0], dout.shape[1], dout.shape[3]
    n = int(n_images)
    if levels is not None:
        levels = _req(levels, torch.int32, "levels")
        if levels.numel() != k:
            raise ValueError("roi_align_bwd: one level per ROI is needed")
    lib = _native.lib()
    hws = [(int(h), int(w)) for h, w in feat_hws]
    nws = int(lib.seam_roi_align_bwd_workspace_bytes(n, k))
    if nws <= 0:
        raise ValueError(f"roi_align_bwd: {n} images / {k} ROIs are outside the kernel's caps")
    outs = [torch.empty((n, h, w, c), dtype=F32, device=dout.device) for h, w in hws]
    ws = torch.empty((nws,), dtype=torch.uint8, device=dout.device)
    hw = (C.c_int * 8)(*[d for s in hws for d in s])
    _native.check(lib.seam_roi_align_bwd_f32(_ptr(dout) if k else None, _ptr(rois) if k else None, _ptr(levels), hw, c,
                                             scales[0], scales[1], scales[2], scales[3], k_min, n, k, p, int(sampling_ratio),
                                             _ptr(outs[0]), _ptr(outs[1]), _ptr(outs[2]), _ptr(outs[3]), _ptr(ws), _stream()),
                  "seam_roi_align_bwd_f32")
    return outs


def rpn_scatter_patches(dpatch: torch.Tensor, rows: torch.Tensor, feat_hws: Sequence[Sequence[int]], n_images: int) -> list:
    """Adjoint of ``rpn_gather_patches``: dpatch fp32 [M,3,3,C], rows int32 [M,4] = (image, level, y, x), feat_hws the (H_l, W_l)
    of the levels -> the gradient maps [N,H_l,W_l,C] (zeros where no window reaches).  Rows are added in row order."""
    dpatch = _req(dpatch, name="dpatch")
    rows = _req(rows, torch.int32, "rows")
    if dpatch.dim() != 4 or tuple(dpatch.shape[1:3]) != (3, 3) or rows.dim() != 2 or rows.shape[1] != 4 or rows.shape[0] != dpatch.shape[0]:
        raise ValueError("rpn_scatter_patches: inconsistent shapes")
    m, c, n, l = dpatch.shape[0], dpatch.shape[3], int(n_images), len(feat_hws)
    hws = [(int(h), int(w)) for h, w in feat_hws]
    if m == 0:
        return [torch.zeros((n, h, w, c), dtype=F32, device=dpatch.device) for h, w in hws]
    outs = [torch.empty((n, h, w, c), dtype=F32, device=dpatch.device) for h, w in hws]
    maps = (C.c_void_p * l)(*[o.data_ptr() for o in outs])
    hw = (C.c_int * (2 * l))(*[d for s in hws for d in s])
    _native.check(_native.lib().seam_rpn_scatter_patches_f32(_ptr(dpatch), _ptr(rows), m, n, l, c, maps, hw, _stream()),
                  "seam_rpn_scatter_patches_f32")
    return outs


def upsample_add_bwd(dlat: torch.Tensor, top_hw: Sequence[int], base: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Adjoint of the nearest top-down merge (``upsample_add_`` / ``conv2d_topdown``): dlat [N,H,W,C] -> [N,Ht,Wt,C], each
    coarse pixel the sum of the fine pixels the forward mapped to it, plus ``base`` [N,Ht,Wt,C] when given."""
    dlat = _req(dlat, name="dlat")
    n, h, w, c = dlat.shape
    ht, wt = int(top_hw[0]), int(top_hw[1])
    if base is not None:
        base = _req(base, name="base")
        if tuple(base.shape) != (n, ht, wt, c):
            raise ValueError("upsample_add_bwd: base must be [N,Ht,Wt,C]")
    out = torch.empty((n, ht, wt, c), dtype=F32, device=dlat.device)
    _native.check(_native.lib().seam_upsample_add_bwd_f32(_ptr(dlat), _ptr(base), _ptr(out), n, h, w, ht, wt, c, _stream()),
                  "seam_upsample_add_bwd_f32")
    return out


def subsample_add_bwd_(d: torch.Tensor, dpool: torch.Tensor) -> torch.Tensor:
    """Adjoint of LastLevelMaxPool (k=1, s=2), in place: d[n,2i,2j,:] += dpool[n,i,j,:]; returns d."""
    if not d.is_contiguous():
        raise ValueError("subsample_add_bwd_: d is updated in place and must be contiguous")
    d, dpool = _req(d, name="d"), _req(dpool, name="dpool")
    n, h, w, c = d.shape
    if tuple(dpool.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise ValueError("subsample_add_bwd_: dpool must be [N,(H-1)//2+1,(W-1)//2+1,C]")
    _native.check(_native.lib().seam_subsample_add_bwd_f32(_ptr(d), _ptr(dpool), n, h, w, dpool.shape[1], dpool.shape[2], c, _stream()),
                  "seam_subsample_add_bwd_f32")
    return d


subsample_add_bwd = subsample_add_bwd_


# ---------------------------------------------------------------------------------------------------- ResNet body training
def relu_mask_add(y: torch.Tensor, a: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = y > 0 ? a + b : 0 over [..., C] (``seam_relu_mask_add_f32``): the ReLU at a bottleneck's output, whose gradient
    feeds both the residual branch and the shortcut; ``b`` (or None) is a second gradient arriving at the same map."""
    y, a = _req(y, name="y"), _req(a, name="a")
    if a.shape != y.shape or (b is not None and b.shape != y.shape):
        raise ValueError("relu_mask_add: y, a and b need one shape")
    if b is not None:
        b = _req(b, name="b")
    c = y.shape[-1]
    out = torch.empty_like(y)
    _native.check(_native.lib().seam_relu_mask_add_f32(_ptr(y), _ptr(a), _ptr(b), _ptr(out), y.numel() // c, c, _stream()),
                  "seam_relu_mask_add_f32")
    return out


def maxpool3s2_relu_bwd(y: torch.Tensor, dpool: torch.Tensor) -> torch.Tensor:
    """Adjoint of ``maxpool2d(y, 3, 2, 1)`` behind the ReLU that made ``y`` (``seam_maxpool3s2_relu_bwd_f32``): y NHWC
    [N,H,W,C], the pool's input; dpool NHWC [N,(H-1)//2+1,(W-1)//2+1,C] -> dy [N,H,W,C], each pixel the sum of the dpool of the
    windows whose argmax it is (torch's: the first maximum in row-major order), zero where y <= 0.  A batch whose y passes
    ``WGRAD_MAX_OPERAND_BYTES`` is split over images, as ``conv_wgrad_chunked`` splits: images are independent, no bit changes."""
    y, dpool = _req(y, name="y"), _req(dpool, name="dpool")
    if y.dim() != 4 or y.shape[0] == 0 or y.shape[-1] % 4:
        raise ValueError(f"maxpool3s2_relu_bwd: y must be a non-empty NHWC tensor with C % 4 == 0, got {tuple(y.shape)}")
    n, h, w, c = y.shape
    if tuple(dpool.shape) != (n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c):
        raise ValueError(f"maxpool3s2_relu_bwd: dpool {tuple(dpool.shape)} must be [N,(H-1)//2+1,(W-1)//2+1,C] of y {tuple(y.shape)}")
    per = h * w * c * 4
    if per > WGRAD_MAX_OPERAND_BYTES:
        raise ValueError(f"maxpool3s2_relu_bwd: one image's y ({per} bytes) exceeds the limit of {WGRAD_MAX_OPERAND_BYTES}")
    step = max(1, min(n, WGRAD_MAX_OPERAND_BYTES // per))
    dy = torch.empty_like(y)
    lib = _native.lib()
    for i in range(0, n, step):
        m = min(step, n - i)
        _native.check(lib.seam_maxpool3s2_relu_bwd_f32(_ptr(y[i:i + m]), _ptr(dpool[i:i + m]), _ptr(dy[i:i + m]), m, h, w, c, _stream()),
                      "seam_maxpool3s2_relu_bwd_f32")
    return dy


# ------------------------------------------------------------------------------ optimizer step (csrc/seam_optim.hip)
def sgd_chunk_table(numels: Sequence[int], chunk: int):
    """Host logic of ``seam_sgd_step_f32``'s chunk table: (tensor, count, offset) rows that put every element of every tensor into
    exactly one chunk of at most ``chunk`` elements, offsets multiples of ``chunk``, no row for an empty tensor."""
    rows = []
    for t, n in enumerate(numels):
        n = int(n)
        if n < 0:
            raise ValueError("sgd_chunk_table: negative element count")
        for off in range(0, n, chunk):
            rows.append((t, min(chunk, n - off), off))
    return rows
