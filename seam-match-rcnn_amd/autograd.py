"""torch.autograd bridges of the match heads.

The training caller (ref stuffs/engine.py:120-121,158-168,183-185) puts ``match_predictor`` and
``temporal_aggregator`` in ``.train()`` and back-propagates the reference's losses through them.  Each
``Function`` below is one fused stage of the heads: forward = the same HIP kernels the inference path uses
(+ BatchNorm1d batch statistics), backward = the gradient kernels of csrc/seam_backward.hip and the
implicit-GEMM conv kernel on rotated weights.  torch is the tape (plus the scalar chain-rule factor of the loss).
"""
from __future__ import annotations

import torch

from . import ops

F32 = torch.float32


class TrunkFunction(torch.autograd.Function):
    """conv_seq (4 valid 3x3 convs + ReLU) -> AvgPool2d(6,6) + ReLU -> Linear -> BatchNorm1d
    (ref models/match_head.py:50-62,67-69).  x NCHW [K,256,14,14] -> x3 [K,256]."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, w2, b2, w3, b3, lw, lb, gamma, beta, running_mean, running_var, bn_train,
                momentum, eps):
        ws, bs = (w0, w1, w2, w3), (b0, b1, b2, b3)
        acts = [ops.nchw_to_nhwc(x.detach().to(F32))]
        for w, b in zip(ws, bs):                                 # 14 -> 12 -> 10 -> 8 -> 6
            acts.append(ops.conv2d(acts[-1], ops.pack_conv(w, b, wino=False), relu=True))
        pool = ops.avgpool(acts[-1])                             # its ReLU is the identity on a mean of ReLU outputs
        lin = ops.linear(pool, ops.pack_conv(lw, lb))
        if bn_train:
            out, mean, inv = ops.bn1d_train_fwd(lin, gamma, beta, running_mean, running_var, momentum, eps)
        else:
            inv = torch.rsqrt(running_var.detach() + eps)        # frozen statistics: plain affine map
            mean = running_mean.detach().clone()
            out = ops.linear(pool, ops.pack_conv(lw, lb, (gamma, beta, running_mean, running_var), bn_eps=eps))
        ctx.save_for_backward(*acts, pool, lin, mean, inv, w1, w2, w3, w0, lw, gamma)
        ctx.bn_train = bn_train
        ctx.x_shape = x.shape
        return out

    @staticmethod
    def backward(ctx, dout):
        x0, y1, y2, y3, y4, pool, lin, mean, inv, w1, w2, w3, w0, lw, gamma = ctx.saved_tensors
        dout = dout.contiguous().to(F32)
        k = dout.shape[0]
        dlin, dgamma, dbeta = ops.bn1d_bwd(dout, lin, mean, inv, gamma, frozen=not ctx.bn_train)
        dlw = ops.conv_wgrad(pool.view(k, 1, 1, -1), dlin.view(k, 1, 1, -1), 1, 1).view(lw.shape)
        dlb = ops.colsum(dlin)
        dpool = ops.linear(dlin, ops.pack_conv_dgrad(lw))
        dy = ops.avgpool_relu_bwd(dpool, y4)
        acts = (x0, y1, y2, y3)
        weights = (w0, w1, w2, w3)
        dws, dbs = [None] * 4, [None] * 4
        dx = None
        for l in (3, 2, 1, 0):
            dws[l] = ops.conv_wgrad(acts[l], dy, 3, 3)
            dbs[l] = ops.colsum(dy)
            if l > 0:                                             # input gradient, masked by the ReLU of the producer
                dy = ops.conv2d(dy, ops.pack_conv_dgrad(weights[l], wino=False), relu=2, residual=acts[l])
            elif ctx.needs_input_grad[0]:
                dx = ops.nhwc_to_nchw(ops.conv2d(dy, ops.pack_conv_dgrad(weights[0], wino=False)))
        return (dx, dws[0], dbs[0], dws[1], dbs[1], dws[2], dbs[2], dws[3], dbs[3], dlw, dlb, dgamma, dbeta,
                None, None, None, None, None)


class PairLogitsFunction(torch.autograd.Function):
    """x5 = last((a_i - b_j)^2)   (ref models/match_head.py:73-74,161-162)."""

    @staticmethod
    def forward(ctx, a, b, w, bias):
        a, b = a.detach().contiguous(), b.detach().contiguous()
        ctx.save_for_backward(a, b, w)
        return ops.pair_logits(a, b, w, bias)

    @staticmethod
    def backward(ctx, g):
        a, b, w = ctx.saved_tensors
        da, db, dw, dbias = ops.pair_logits_bwd(a, b, w, g.contiguous())
        return da, db, dw, dbias


class NlbAttnPoolFunction(torch.autograd.Function):
    """Batched non-local block (sequences longer than one row) + softmax attention pooling
    (ref models/nlb.py:66-101, models/match_head.py:114-121).  seq time-major [T,S,256], lens int32 [S]."""

    @staticmethod
    def forward(ctx, seq, lens, use_nlb, theta_w, theta_b, phi_w, phi_b, g_w, g_b, cat_w, W_w, W_b, att_w, att_b):
        seq = seq.detach().contiguous()
        pk = ops.PackedNLB(
            w_proj_t=torch.cat([theta_w[:, :, 0], phi_w[:, :, 0], g_w[:, :, 0]], 0).detach().t().contiguous(),
            b_proj=torch.cat([theta_b, phi_b, g_b]).detach().contiguous(),
            w_cat=cat_w.detach().reshape(256).contiguous(),
            w_out_t=W_w.detach()[:, :, 0].t().contiguous(), b_out=W_b.detach().contiguous(),
            w_att=att_w.detach().reshape(256).contiguous(), b_att=att_b.detach().reshape(1).contiguous())
        t, s = seq.shape[0], seq.shape[1]
        out, _ = ops.nlb_attnpool(seq, s * 256, 256, lens, s, t, pk, use_nlb=use_nlb)
        ctx.save_for_backward(seq, lens)
        ctx.pk, ctx.use_nlb = pk, use_nlb
        return out

    @staticmethod
    def backward(ctx, dout):
        seq, lens = ctx.saved_tensors
        t, s = seq.shape[0], seq.shape[1]
        dseq, grads = ops.nlb_attnpool_bwd(seq, s * 256, 256, lens, s, t, ctx.pk, dout.contiguous(), ctx.use_nlb)
        return (dseq, None, None, *grads)


class NlbBlockFunction(torch.autograd.Function):
    """The non-local block alone, ``NONLocalBlock1D.forward`` called directly (ref models/nlb.py:66-101):
    x [b,256,t] -> z [b,256,t].  The block is applied whatever t is (the length-1 bypass is the aggregator's rule)."""

    @staticmethod
    def forward(ctx, x, theta_w, theta_b, phi_w, phi_b, g_w, g_b, cat_w, W_w, W_b):
        b, c, t = x.shape
        xt = ops.nchw_to_nhwc(x.detach().to(F32).contiguous().view(b, c, t))             # rows [b,t,256]
        dev = x.device
        pk = ops.PackedNLB(
            w_proj_t=torch.cat([theta_w[:, :, 0], phi_w[:, :, 0], g_w[:, :, 0]], 0).detach().t().contiguous(),
            b_proj=torch.cat([theta_b, phi_b, g_b]).detach().contiguous(),
            w_cat=cat_w.detach().reshape(256).contiguous(),
            w_out_t=W_w.detach()[:, :, 0].t().contiguous(), b_out=W_b.detach().contiguous(),
            w_att=torch.zeros(256, device=dev), b_att=torch.zeros(1, device=dev))
        lens = torch.full((b,), t, dtype=torch.int32, device=dev)
        _, _, z = ops.nlb_attnpool(xt, 256, t * 256, lens, b, t, pk, use_nlb=2, want_z=True)
        ctx.save_for_backward(xt, lens)
        ctx.pk = pk
        return ops.nhwc_to_nchw(z)

    @staticmethod
    def backward(ctx, dz):
        xt, lens = ctx.saved_tensors
        b, t, _ = xt.shape
        dzt = ops.nchw_to_nhwc(dz.contiguous().to(F32))                                    # [b,t,256]
        dxt, grads = ops.nlb_block_bwd(xt, 256, t * 256, lens, b, t, ctx.pk, dzt, 256, t * 256, use_nlb=2)
        return (ops.nhwc_to_nchw(dxt), *grads)


class WeightedCE2Function(torch.autograd.Function):
    """nn.CrossEntropyLoss(weight=[w0,w1]) over [n,2] logits (the criterion of every loss in the reference's
    models/match_head.py:213,257,367,386): weighted mean of -log softmax(x)[y]."""

    @staticmethod
    def forward(ctx, logits, target, weight):
        loss, dlogits = ops.ce2_fwd_bwd(logits.detach().contiguous(), target, weight)
        ctx.save_for_backward(dlogits)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return dlogits * g, None, None


# ---------------------------------------------------------------------------------------------------- RoI heads training
# (ref models/matchrcnn.py:333-472).  Each head returns an input gradient only when its input carries a tape (a trainable FPN).

def _pad_rows(w: torch.Tensor, rows: int) -> torch.Tensor:
    """[K,...] -> [rows,...] with zero rows appended (pack_conv_dgrad needs Cout % 32 == 0)."""
    if w.shape[0] == rows:
        return w.contiguous()
    out = w.new_zeros((rows,) + tuple(w.shape[1:]))
    out[:w.shape[0]] = w
    return out


def _pad_cols(x: torch.Tensor, cols: int) -> torch.Tensor:
    """[M,K] -> [M,cols], zero columns appended."""
    if x.shape[1] == cols:
        return x.contiguous()
    out = x.new_zeros((x.shape[0], cols))
    out[:, :x.shape[1]] = x
    return out


def _up32(k: int) -> int:
    return (k + 31) // 32 * 32


def _full_dgrad_1x1(dy: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """Input gradient of a VALID RxS conv whose output is 1x1 (fc6 over its 7x7 tile, the RPN conv over a 3x3 window):
    dy [M,K], w OIHW [K,C,R,S] -> dx NHWC [M,R,S,C] = dy @ W with W[k, (r,s,c)] -- the full transposed conv has one tap per
    output pixel, so it is one GEMM and the result lands in NHWC order."""
    k, c, r, s = w.shape
    wt = w.detach().permute(2, 3, 1, 0).reshape(r * s * c, k).contiguous()
    return ops.linear(dy.contiguous(), ops.pack_conv(wt, None)).view(dy.shape[0], r, s, c)


class BoxHeadFunction(torch.autograd.Function):
    """TwoMLPHead + FastRCNNPredictor (ref torchvision roi_heads box branch): x NHWC [R,7,7,256] ->
    (class_logits [R,ncls], box_regression [R,4*ncls]).  fc6 is the 7x7 valid conv over the tile; fc7 and the fused
    ncls + 4*ncls predictor rows are 1x1 convs.  The input gradient (asked for when the RoIAlign output carries a tape) is the
    full 7x7 transposed conv of the 1x1 gradient, i.e. one GEMM [R,1024] x [1024, 7*7*256] straight into the NHWC tile."""

    @staticmethod
    def forward(ctx, x, w6, b6, w7, b7, wc, bc, wb, bb):
        x = x.detach().contiguous()
        r = x.shape[0]
        w6c = w6.detach().view(w6.shape[0], x.shape[-1], 7, 7)
        h6 = ops.conv2d(x, ops.pack_conv(w6c, b6, wino=False), relu=True)                       # [R,1,1,1024]
        h7 = ops.linear(h6.view(r, -1), ops.pack_conv(w7, b7), relu=True)                       # [R,1024]
        wp = torch.cat([wc.detach(), wb.detach()], 0)
        o = ops.linear(h7, ops.pack_conv(wp, torch.cat([bc.detach(), bb.detach()], 0)), out_f32=True)
        ncls = wc.shape[0]
        ctx.save_for_backward(x, h6, h7, w6c, w7, wp)
        ctx.ncls = ncls
        return o[:, :ncls].contiguous(), o[:, ncls:].contiguous()

    @staticmethod
    def backward(ctx, dcls, dbox):
        x, h6, h7, w6c, w7, wp = ctx.saved_tensors
        r, ncls = x.shape[0], ctx.ncls
        kp = _up32(wp.shape[0])
        do = torch.zeros((r, kp), dtype=F32, device=x.device)
        if dcls is not None:
            do[:, :ncls] = dcls
        if dbox is not None:
            do[:, ncls:wp.shape[0]] = dbox
        dwp = ops.conv_wgrad(h7.view(r, 1, 1, -1), do.view(r, 1, 1, kp), 1, 1).view(kp, -1)[:wp.shape[0]]
        dbp = ops.colsum(do)[:wp.shape[0]]
        dh7 = ops.conv2d(do.view(r, 1, 1, kp), ops.pack_conv_dgrad(_pad_rows(wp, kp), wino=False), relu=2,
                         residual=h7.view(r, 1, 1, -1))                                          # [R,1,1,1024]
        dw7 = ops.conv_wgrad(h6, dh7, 1, 1).view(w7.shape)
        db7 = ops.colsum(dh7)
        dh6 = ops.conv2d(dh7, ops.pack_conv_dgrad(w7, wino=False), relu=2, residual=h6)
        dw6 = ops.conv_wgrad(x, dh6, 7, 7).view(w6c.shape[0], -1)
        db6 = ops.colsum(dh6)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = _full_dgrad_1x1(dh6.view(r, -1), w6c)
        return dx, dw6, db6, dw7, db7, dwp[:ncls], dbp[:ncls], dwp[ncls:], dbp[ncls:]


class MaskHeadFunction(torch.autograd.Function):
    """MaskRCNNHeads (4 x conv3x3 pad 1 + ReLU) + MaskRCNNPredictor: x NHWC [P,14,14,256] -> logits in the sub-pixel
    layout [P,14,14,4*ncls] (detection.MaskRCNNPredictor.forward).  conv5_mask (ConvTranspose2d 2x2/s2) is the 1x1 conv
    to the 4 sub-pixel groups (a,b) (channel (a*2+b)*256+co), so its backward is a 1x1 dgrad + wgrad with no shuffle.
    The input gradient (asked for when the RoIAlign output carries a tape) is one more 3x3 dgrad."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, w3, b3, w4, b4, wt, bt, wl, bl):
        x = x.detach().contiguous()
        p = x.shape[0]
        ws3 = (w1, w2, w3, w4)
        acts = [x]
        for w, b in zip(ws3, (b1, b2, b3, b4)):
            acts.append(ops.conv2d(acts[-1], ops.pack_conv(w, b, pad=1, wino=False), relu=True))
        u = ops.conv2d(acts[-1], ops.pack_conv(wt, bt, transposed2x2=True), relu=True)          # [P,14,14,4*256]
        ncls = wl.shape[0]
        logits = ops.linear(u.view(p * 784, -1), ops.pack_conv(wl, bl)).view(p, 14, 14, 4 * ncls)
        ctx.save_for_backward(*acts, u, *(w.detach() for w in ws3), wt.detach(), wl.detach())
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        a0, a1, a2, a3, a4, u, w1, w2, w3, w4, wt, wl = ctx.saved_tensors
        p = a0.shape[0]
        ncls, cr = wl.shape[0], wl.shape[1]
        kp = _up32(ncls)
        # mask_fcn_logits: one 1x1 conv over the P*196*4 rows (the sub-pixel group is the fastest row index)
        dl = _pad_cols(dlogits.contiguous().view(p * 784, ncls).to(F32), kp).view(p * 784, 1, 1, kp)
        dwl = ops.conv_wgrad(u.view(p * 784, 1, 1, cr), dl, 1, 1)[:ncls]
        dbl = ops.colsum(dl)[:ncls]
        du = ops.conv2d(dl, ops.pack_conv_dgrad(_pad_rows(wl, kp), wino=False), relu=2,
                        residual=u.view(p * 784, 1, 1, cr)).view(p, 14, 14, 4 * cr)
        # conv5_mask as the 1x1 conv with rows (a*2+b)*Cout+co over Cin
        cin, cout = wt.shape[0], wt.shape[1]
        wt1 = wt.permute(2, 3, 1, 0).reshape(4 * cout, cin)
        dwt1 = ops.conv_wgrad(a4, du, 1, 1).view(2, 2, cout, cin)
        dwt = dwt1.permute(3, 2, 0, 1).contiguous()
        dbt = ops.colsum(du).view(4, cout).sum(0)
        dy = ops.conv2d(du, ops.pack_conv_dgrad(wt1, wino=False), relu=2, residual=a4)
        acts, weights = (a0, a1, a2, a3), (w1, w2, w3, w4)
        dws, dbs = [None] * 4, [None] * 4
        for l in (3, 2, 1, 0):
            dws[l] = ops.conv_wgrad(acts[l], dy, 3, 3, pad=1)
            dbs[l] = ops.colsum(dy)
            if l > 0:
                dy = ops.conv2d(dy, ops.pack_conv_dgrad(weights[l], pad_fwd=1, wino=False), relu=2, residual=acts[l])
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.conv2d(dy, ops.pack_conv_dgrad(weights[0], pad_fwd=1, wino=False))
        return (dx, dws[0], dbs[0], dws[1], dbs[1], dws[2], dbs[2], dws[3], dbs[3], dwt, dbt, dwl, dbl)


class FastRCNNLossFunction(torch.autograd.Function):
    """fastrcnn_loss [TV] -> (loss_classifier, loss_box_reg), 0-d each; the forward launch computes both gradients."""

    @staticmethod
    def forward(ctx, class_logits, box_regression, labels, targets):
        loss, dcls, dbox = ops.fastrcnn_loss_fwd_bwd(class_logits.detach().contiguous(), box_regression.detach().contiguous(),
                                                     labels, targets.detach())
        ctx.save_for_backward(dcls, dbox)
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_cls, g_box):
        dcls, dbox = ctx.saved_tensors
        return dcls * g_cls, dbox * g_box, None, None


class MaskLossFunction(torch.autograd.Function):
    """maskrcnn_loss [TV] on the sub-pixel logits; the forward launch computes the gradient."""

    @staticmethod
    def forward(ctx, logits, labels, rois, masks, mask_off, mask_hw):
        loss, dl = ops.mask_loss_fwd_bwd(logits.detach().contiguous(), labels, rois.detach(), masks, mask_off, mask_hw)
        ctx.save_for_backward(dl)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dl,) = ctx.saved_tensors
        return dl * g, None, None, None, None, None


# ---------------------------------------------------------------------------------------------------- RPN training
# d loss / d head output is zero outside the sampled (pixel, anchor) slots, so the gradient of the 3x3 conv and of the two
# 1x1 predictors is exactly a sum over the sampled rows: no dense backward conv.

class RPNHeadRowsFunction(torch.autograd.Function):
    """RPNHead at M sampled pixels: patches NHWC [M,3,3,256] (the conv's 3x3 input windows, zero padding included; slots
    that share a pixel are separate rows) -> [M, A + 4A] (objectness logits | deltas).  The input gradient (asked for when the
    windows carry a tape, ``RPNPatchesFunction``) is the full 3x3 transposed conv of the [M,1,1,256] gradient: one GEMM."""

    @staticmethod
    def forward(ctx, patches, w, b, wc, bc, wb, bb):
        x = patches.detach().contiguous()
        m = x.shape[0]
        t = ops.conv2d(x, ops.pack_conv(w, b, pad=0, wino=False), relu=True)                    # [M,1,1,256]
        wp = torch.cat([wc.detach().reshape(wc.shape[0], -1), wb.detach().reshape(wb.shape[0], -1)], 0)
        o = ops.linear(t.view(m, -1), ops.pack_conv(wp, torch.cat([bc.detach(), bb.detach()], 0)), out_f32=True)
        ctx.save_for_backward(x, t, wp, w.detach())
        ctx.shapes = (wc.shape, wb.shape)
        return o

    @staticmethod
    def backward(ctx, do):
        x, t, wp, w = ctx.saved_tensors
        m, k = x.shape[0], wp.shape[0]
        kp = _up32(k)
        do = _pad_cols(do.to(F32), kp).view(m, 1, 1, kp)
        dwp = ops.conv_wgrad(t, do, 1, 1).view(kp, -1)[:k]
        dbp = ops.colsum(do)[:k]
        dt = ops.conv2d(do, ops.pack_conv_dgrad(_pad_rows(wp, kp), wino=False), relu=2, residual=t)    # [M,1,1,256]
        dw = ops.conv_wgrad(x, dt, 3, 3)
        db = ops.colsum(dt)
        a = ctx.shapes[0][0]
        dx = _full_dgrad_1x1(dt.view(m, -1), w) if ctx.needs_input_grad[0] else None
        return (dx, dw, db, dwp[:a].reshape(ctx.shapes[0]), dbp[:a], dwp[a:].reshape(ctx.shapes[1]), dbp[a:])


class RPNLossFunction(torch.autograd.Function):
    """RegionProposalNetwork.compute_loss [TV] on the sampled rows -> (loss_objectness, loss_rpn_box_reg), 0-d each; the
    forward launch computes the gradient."""

    @staticmethod
    def forward(ctx, head, slot, labels, targets, num_anchors):
        loss, grad = ops.rpn_loss_fwd_bwd(head.detach().contiguous(), slot, labels, targets.detach(), num_anchors,
                                          _up32(head.shape[1]))
        ctx.save_for_backward(grad)
        ctx.a, ctx.k = num_anchors, head.shape[1]
        return loss[0], loss[1]

    @staticmethod
    def backward(ctx, g_obj, g_box):
        (grad,) = ctx.saved_tensors
        scale = torch.cat([g_obj.expand(ctx.a), g_box.expand(grad.shape[1] - ctx.a)])
        return (grad * scale)[:, :ctx.k], None, None, None, None


# ---------------------------------------------------------------------------------------------------- FPN training
# The adjoints of csrc/seam_fpn_train.hip behind torch's tape: RoIAlign, the RPN's window gather, and the pyramid itself.
# Every gradient is summed in a fixed order (no float atomics), so two identical steps give the same bits.

class RoIAlignFunction(torch.autograd.Function):
    """MultiScaleRoIAlign on four NHWC maps [N,H_l,W_l,C] -> [K,P,P,C]; backward = ``ops.roi_align_bwd`` (the maps'
    gradients are written completely; the ROIs are constants)."""

    @staticmethod
    def forward(ctx, rois, scales, pooled, sampling_ratio, k_min, f0, f1, f2, f3):
        feats = [f.detach() for f in (f0, f1, f2, f3)]
        rois = rois.detach().contiguous()
        ctx.save_for_backward(rois)
        ctx.geom = ([tuple(f.shape[1:3]) for f in feats], feats[0].shape[0], tuple(scales), sampling_ratio, k_min)
        return ops.roi_align(feats, rois, scales, pooled, sampling_ratio, k_min)

    @staticmethod
    def backward(ctx, dout):
        (rois,) = ctx.saved_tensors
        hws, n, scales, sr, k_min = ctx.geom
        d = ops.roi_align_bwd(dout.contiguous().to(F32), rois, hws, n, scales, sr, k_min)
        return (None, None, None, None, None, *d)


class RPNPatchesFunction(torch.autograd.Function):
    """``ops.rpn_gather_patches`` over the pyramid maps; backward = ``ops.rpn_scatter_patches`` (rows in row order)."""

    @staticmethod
    def forward(ctx, rows, *maps):
        maps = [m.detach() for m in maps]
        ctx.save_for_backward(rows)
        ctx.geom = ([tuple(m.shape[1:3]) for m in maps], maps[0].shape[0])
        return ops.rpn_gather_patches(maps, rows)

    @staticmethod
    def backward(ctx, dpatch):
        (rows,) = ctx.saved_tensors
        hws, n = ctx.geom
        return (None, *ops.rpn_scatter_patches(dpatch.contiguous().to(F32), rows, hws, n))


class GatherRowsFunction(torch.autograd.Function):
    """``x[idx]`` for a HOST index array that may hold duplicates (``filter_proposals`` can keep a ROI once per GT box).  The
    backward adds the j-th occurrence of every index in round j -- inside a round the indices are unique -- so the sum has a
    fixed order whatever the device's index_put does with duplicates."""

    @staticmethod
    def forward(ctx, x, idx):
        import numpy as np
        idx = np.asarray(idx, np.int64)
        order = np.argsort(idx, kind="stable")
        srt = idx[order]
        first = np.r_[True, srt[1:] != srt[:-1]] if len(srt) else np.zeros(0, bool)
        start = np.maximum.accumulate(np.where(first, np.arange(len(srt)), 0)) if len(srt) else np.zeros(0, np.int64)
        occ = np.arange(len(srt)) - start                        # 0 for the first occurrence of an index, 1 for the second ...
        dev = x.device
        ctx.rounds = [(torch.from_numpy(srt[occ == j]).to(dev), torch.from_numpy(order[occ == j]).to(dev))
                      for j in range(int(occ.max()) + 1 if len(occ) else 0)]
        ctx.shape = x.shape
        return x.detach()[torch.from_numpy(idx).to(dev)]

    @staticmethod
    def backward(ctx, g):
        dx = torch.zeros(ctx.shape, dtype=g.dtype, device=g.device)
        for rows, pos in ctx.rounds:
            dx[rows] += g[pos]
        return dx, None


class FPNFunction(torch.autograd.Function):
    """FeaturePyramidNetwork + LastLevelMaxPool on NHWC maps: (C2..C5, the sixteen parameters) -> (P2..P5, pool).

    forward: the launches of ``FeaturePyramidNetwork.forward`` in its single-stream form on the module's packed weights (the
    same bits), keeping the four merged inner maps.  backward, finest level first (an inner map's gradient needs the finer
    level's): the pool adjoint into P5's gradient, then per level colsum + conv_wgrad of the 3x3 output conv, its dgrad
    (exact fp32), ``upsample_add_bwd`` of the finer inner gradient with that dgrad as its base, conv_wgrad + colsum of the
    lateral 1x1, and -- only when a C map asks for it -- the 1x1 dgrad."""

    @staticmethod
    def forward(ctx, packed, c2, c3, c4, c5, *params):
        inner, layer = packed[:2]      # (the exact packs: the split twins behind them are never taped)
        feats = [f.detach() for f in (c2, c3, c4, c5)]
        last = ops.conv2d(feats[3], inner[3])
        inners = [None, None, None, last]
        outs = [None, None, None, ops.conv2d(last, layer[3])]
        for i in (2, 1, 0):
            last = ops.conv2d_topdown(feats[i], inner[i], last)
            inners[i] = last
            outs[i] = ops.conv2d(last, layer[i])
        pool = ops.maxpool2d(outs[3], 1, 2, 0)
        ctx.save_for_backward(*feats, *inners, *(params[2 * i].detach() for i in range(8)))
        return (*outs, pool)

    @staticmethod
    def backward(ctx, g0, g1, g2, g3, gpool):
        saved = ctx.saved_tensors
        feats, inners, iw, lw = saved[0:4], saved[4:8], saved[8:12], saved[12:16]
        gs = [g0, g1, g2, g3]
        for i in range(4):
            gs[i] = (torch.zeros_like(inners[i]) if gs[i] is None else gs[i].contiguous().to(F32))
        if gpool is not None:
            gs[3] = ops.subsample_add_bwd_(gs[3].clone(), gpool.contiguous().to(F32))
        d_in = [None] * 4            # gradients of the merged inner maps
        diw, dib, dlw, dlb, dfeat = [None] * 4, [None] * 4, [None] * 4, [None] * 4, [None] * 4
        for i in range(4):
            dlw[i] = ops.conv_wgrad_chunked(inners[i], gs[i], 3, 3, 1, 1)
            dlb[i] = ops.colsum(gs[i])
            own = ops.conv2d(gs[i], ops.pack_conv_dgrad(lw[i], pad_fwd=1))
            d_in[i] = own if i == 0 else ops.upsample_add_bwd(d_in[i - 1], own.shape[1:3], base=own)
            diw[i] = ops.conv_wgrad_chunked(feats[i], d_in[i], 1, 1)
            dib[i] = ops.colsum(d_in[i])
            if ctx.needs_input_grad[1 + i]:
                dfeat[i] = ops.conv2d(d_in[i], ops.pack_conv_dgrad(iw[i]))
        grads = [t for i in range(4) for t in (diw[i], dib[i])] + [t for i in range(4) for t in (dlw[i], dlb[i])]
        return (None, *dfeat, *grads)


# ---------------------------------------------------------------------------------------------------- ResNet body training
# Bottleneck v1.5 with FrozenBatchNorm2d: y = relu(bn3(conv3(o2)) + shortcut(x)), o2 = relu(bn2(conv2(o1))), o1 = relu(bn1(conv1(x))).
# A FrozenBN is y = scale[k] * conv + shift[k], so a conv's output gradient carries scale[k]: the dgrad weights are packed from
# scale[k] * W (once per backward) and the wgrad result is scaled by row.

def _scaled(w: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return w.detach() * scale.view(-1, 1, 1, 1)


class BodyFunction(torch.autograd.Function):
    """A run of consecutive bottlenecks of ``ResNet50Body``, from the first one that holds a trainable weight to the last of
    layer4: (input of the first block, the conv weights of every block in ``detection.block_weights`` order) -> the outputs of
    the layers that end inside the run (C2..C5 or the upper ones of them).

    forward: ``detection.body_block`` per block -- the launches of ``ResNet50Body._run``, the fused ``conv2d_dual`` shortcut
    blocks included -- keeping per block its input, the two post-ReLU inner activations and its output.  backward, last block
    first: g = relu_mask_add(y, gradient from the block above, gradient of the FPN into this layer's map); conv3: wgrad + 1x1
    dgrad masked by o2; conv2: wgrad + dgrad masked by o1 (stride 1: the rotated-weight conv, stride 2: ``conv3x3s2_dgrad``);
    conv1: wgrad + 1x1 dgrad whose epilogue adds the shortcut gradient -- g itself, or for a projection block the 1x1 dgrad of
    the downsample conv on the coarse grid, scattered to the even pixels when the stride is 2.  A weight gradient is computed
    only for a weight that requires one, an input gradient only where a block below still needs it (for the first only when the stem trains).

    ``stem`` = (the stem conv + FrozenBN + ReLU on the body's packed weights, the FrozenBN scale) when the stem trains, else
    None.  Then ``x`` is the frame (NHWC4 or space-to-depth), ``weights`` starts with ``conv1.weight`` and the run is all sixteen
    blocks; the frame and the stem output y0 are kept too.  The first block then computes its input gradient as well, which is the
    gradient of the pooled map: dy0 = ``maxpool3s2_relu_bwd(y0, .)``, and conv1's gradient is ``conv_wgrad`` of the frame
    the forward consumed -- 7x7 / stride 2 on NHWC4 (the padding channel dropped), or the cropped 4x4 / stride 1 of the
    space-to-depth form mapped back by ``detection.stem_s2d_grad_to_oihw`` -- scaled by row.  No gradient for the frame."""

    @staticmethod
    def forward(ctx, meta, stem, x, *weights):
        from .models.detection import body_block
        x = x.detach()
        ctx.stem_scale = None
        stem_saved = ()
        if stem is not None:
            conv, ctx.stem_scale = stem
            y0 = conv(x)
            stem_saved = (x, y0)
            x = ops.maxpool2d(y0, 3, 2, 1)
        xs, o1s, o2s, outs = [x], [], [], []
        for e, stride, _, last in meta:
            x, o1, o2 = body_block(x, e, stride)
            xs.append(x)
            o1s.append(o1)
            o2s.append(o2)
            if last:
                outs.append(x)
        ctx.save_for_backward(*xs, *o1s, *o2s, *stem_saved, *(w.detach() for w in weights))
        ctx.meta = [(dict(s1=e["c1"].scale, s2=e["c2"].scale, s3=e["c3"].scale, sd=e["ds"].scale if "ds" in e else None),
                     stride, proj, last) for e, stride, proj, last in meta]
        ctx.n_blocks = len(meta)
        return tuple(outs)

    @staticmethod
    def backward(ctx, *gouts):
        nb = ctx.n_blocks
        saved = ctx.saved_tensors
        xs, o1s, o2s, ws = saved[:nb + 1], saved[nb + 1:2 * nb + 1], saved[2 * nb + 1:3 * nb + 1], saved[3 * nb + 1:]
        need = ctx.needs_input_grad[3:]
        stem = ctx.stem_scale is not None
        if stem:                                      # (frame, y0, conv1.weight) ahead of the blocks' weights
            frame, y0, ws = ws[0], ws[1], ws[3:]
            need_stem, need = need[0], need[1:]
        wpos, k = [], 0
        for _, _, proj, _ in ctx.meta:
            wpos.append(k)
            k += 4 if proj else 3
        dws = [None] * len(ws)
        gouts = list(gouts)
        g_up = None                                   # gradient of the block above into this block's output
        for b in range(nb - 1, -1, -1):
            sc, stride, proj, last = ctx.meta[b]
            x, o1, o2, y = xs[b], o1s[b], o2s[b], xs[b + 1]
            g_fpn = gouts.pop() if last else None
            if g_fpn is not None:
                g_fpn = g_fpn.contiguous().to(F32)
            first, second = (g_up, g_fpn) if g_up is not None else (g_fpn, None)
            if first is None:
                first = torch.zeros_like(y)
            g = ops.relu_mask_add(y, first, second)
            p = wpos[b]
            w1, w2, w3 = ws[p], ws[p + 1], ws[p + 2]
            need_dx = b > 0 or stem
            need1 = need[p] or need_dx                # the gradient of o1 is wanted
            need2 = need[p + 1] or need1              # ... of o2
            if need[p + 2]:
                dws[p + 2] = ops.conv_wgrad_chunked(o2, g, 1, 1) * sc["s3"].view(-1, 1, 1, 1)
            if proj and need[p + 3]:
                dws[p + 3] = ops.conv_wgrad_chunked(x, g, 1, 1, stride, 0) * sc["sd"].view(-1, 1, 1, 1)
            g_up = None
            if not need2:
                continue
            d2 = ops.conv2d(g, ops.pack_conv_dgrad(_scaled(w3, sc["s3"])), relu=2, residual=o2)
            if need[p + 1]:
                dws[p + 1] = ops.conv_wgrad_chunked(o1, d2, 3, 3, stride, 1) * sc["s2"].view(-1, 1, 1, 1)
            if not need1:
                continue
            if stride == 2:
                d1 = ops.conv3x3s2_dgrad(d2, ops.pack_conv3x3s2_dgrad(w2, sc["s2"]), o1.shape[1:3], mask=o1)
            else:
                d1 = ops.conv2d(d2, ops.pack_conv_dgrad(_scaled(w2, sc["s2"]), pad_fwd=1), relu=2, residual=o1)
            if need[p]:
                dws[p] = ops.conv_wgrad_chunked(x, d1, 1, 1) * sc["s1"].view(-1, 1, 1, 1)
            if not need_dx:
                continue
            if proj:
                short = ops.conv2d(g, ops.pack_conv_dgrad(_scaled(ws[p + 3], sc["sd"])))
                if stride == 2:
                    short = ops.subsample_add_bwd_(torch.zeros_like(x), short)
            else:
                short = g
            g_up = ops.conv2d(d1, ops.pack_conv_dgrad(_scaled(w1, sc["s1"])), relu=False, residual=short)
        if not stem:
            return (None, None, None, *dws)
        dw0 = None
        if need_stem:
            from .models.detection import stem_s2d_grad_to_oihw
            dy0 = ops.maxpool3s2_relu_bwd(y0, g_up)
            if frame.shape[-1] == 4:
                dw0 = ops.conv_wgrad_chunked(frame, dy0, 7, 7, 2, 3)[:, :3].contiguous()
            else:
                dw0 = stem_s2d_grad_to_oihw(ops.conv_wgrad_chunked(frame, dy0, 4, 4, 1, 2, out_hw=dy0.shape[1:3]))
            dw0 = dw0 * ctx.stem_scale.view(-1, 1, 1, 1)
        return (None, None, None, dw0, *dws)
