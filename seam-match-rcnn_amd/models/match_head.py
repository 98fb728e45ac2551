"""SEAM match heads, mirror of reference ``models/match_head.py`` (heads only).

``MatchPredictor.forward(x, types) -> (x3, x5)``                      ref :66-76
``TemporalAggregationNLB.forward(x, types, ids, x3_1_seq=None, x3_1_mask=None, x3_2=None,
                                 getatt=False) -> 6- or 7-tuple``       ref :90-169

Same constructor arguments, attribute names (``conv_seq, pool, linear, last,
attention_scorer, newnlb, nlb, n_frames``) and state-dict keys as the reference, so
checkpoints and callers (``stuffs/engine.py:158``, ``evaluate_movingfashion.py:42,73,258``,
the aggregation losses at ``models/match_head.py:339``) are interchangeable.  The training
losses of the reference file are callers of these heads, not part of the forward hot path.

Arithmetic: trunk = 4 valid 3x3 implicit-GEMM convs + avg-pool + Linear/BatchNorm epilogue
(``seam_conv2d_f32``), sequences -> one batched NLB+attention-pool launch
(``seam_nlb_attnpool_f32``), pairwise classifier (``seam_pair_logits_f32``).  No CPU or
eager fallback: CPU tensors raise.  In ``.train()`` / with autograd on (the grad-enabled pass of
``stuffs/engine.py:158-168``) the same stages run as ``autograd.py`` nodes whose backward is
``csrc/seam_backward.hip``; the reference's losses (``models/losses.py``) are re-exported
here because ``stuffs/engine.py:11-12`` imports them from this module.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import ops
from .nlb import NONLocalBlock1D
from .packed import PackedWeights


def _wants_tape(module: nn.Module, *tensors) -> bool:
    """True when the call must go through the autograd bridges (``autograd.py``): BatchNorm1d in training mode
    (batch statistics, even under no_grad), or grad mode with something that requires grad -- the grad-enabled
    pass of the training loop, ref stuffs/engine.py:120-121,158-168."""
    if module.linear[1].training:
        return True
    if not torch.is_grad_enabled():
        return False
    return any(p.requires_grad for p in module.parameters()) or any(
        t is not None and torch.is_tensor(t) and t.requires_grad for t in tensors)


def pack_nlb_from_state(sd: dict, prefix: str = "") -> ops.PackedNLB:
    """Build the NLB/attention kernel's weight pack from a flat (device) state dict."""
    g = lambda k: sd[prefix + k]  # noqa: E731
    return ops.PackedNLB(
        w_proj_t=torch.cat([g("newnlb.theta.weight")[:, :, 0], g("newnlb.phi.weight")[:, :, 0],
                            g("newnlb.g.weight")[:, :, 0]], 0).t().contiguous(),
        b_proj=torch.cat([g("newnlb.theta.bias"), g("newnlb.phi.bias"), g("newnlb.g.bias")]).contiguous(),
        w_cat=g("newnlb.concat_project.0.weight").reshape(256).contiguous(),
        w_out_t=g("newnlb.W.weight")[:, :, 0].t().contiguous(),
        b_out=g("newnlb.W.bias").contiguous(),
        w_att=g("attention_scorer.weight").reshape(256).contiguous(),
        b_att=g("attention_scorer.bias").reshape(1).contiguous())


def plan_sequences(types_c: torch.Tensor, ids_c: torch.Tensor):
    """Host-side sequence packing plan of Mode A (ref models/match_head.py:96-111).

    types_c / ids_c: CPU tensors [K].  Street rows (type 0) are grouped by *sorted unique id*;
    ``maxlen`` = count of the modal id; inside a sequence rows keep their original order.
    Returns (sel0, order, pos, seq_of_row, counts):
      sel0        indices (into the K rows) of the type-0 rows
      order       permutation of sel0-local rows, grouped by sequence
      pos         position of each ordered row inside its sequence (0-based)
      seq_of_row  sequence index of each ordered row
      counts      rows per sequence (int64 [S])"""
    sel0 = (types_c == 0).nonzero().view(-1)
    ids0 = ids_c[sel0]
    uniq, inv, counts = torch.unique(ids0, sorted=True, return_inverse=True, return_counts=True)
    order = torch.argsort(inv, stable=True)
    starts = torch.cumsum(counts, 0) - counts
    seq_of_row = inv[order]
    pos = torch.arange(order.numel()) - starts[seq_of_row]
    return sel0, order, pos, seq_of_row, counts


_PLAN_CACHE = {}     # (types bytes, ids bytes, device) -> device-resident packing plan of Mode A


def device_plan(types_c: torch.Tensor, ids_c: torch.Tensor, dev: torch.device):
    """``plan_sequences`` with its index tensors uploaded once per distinct (types, ids): callers such as the
    evaluator / the bench pass the same layout for every clip, so steady-state calls issue no host-to-device
    copies (and stay capturable in a HIP graph)."""
    key = (types_c.numpy().tobytes(), ids_c.numpy().tobytes(), str(types_c.dtype), str(ids_c.dtype), str(dev))
    plan = _PLAN_CACHE.get(key)
    if plan is None:
        sel0, order, pos, seq_of_row, counts = plan_sequences(types_c, ids_c)
        n_seqs = int(counts.numel())
        maxlen = int(counts.max()) if n_seqs else 0
        plan = dict(
            n0=int(sel0.numel()), n_seqs=n_seqs, maxlen=maxlen, counts=counts,
            rows=sel0[order].to(dev), pos1=(pos + 1).to(dev), seq_of_row=seq_of_row.to(dev),
            sel1=(types_c == 1).nonzero().view(-1).to(dev),
            mask=(torch.arange(1 + maxlen)[None, :] > counts[:, None]).to(dev) if n_seqs else None,
            lens=counts.to(torch.int32).to(dev) if n_seqs else None,
            ids0=ids_c[sel0])
        if len(_PLAN_CACHE) > 64:
            _PLAN_CACHE.clear()
        _PLAN_CACHE[key] = plan
    return plan


class MatchPredictor(PackedWeights, nn.Module):
    def __init__(self):
        super().__init__()
        self.conv_seq = nn.Sequential(nn.Conv2d(256, 256, 3), nn.ReLU(),
                                      nn.Conv2d(256, 256, 3), nn.ReLU(),
                                      nn.Conv2d(256, 256, 3), nn.ReLU(),
                                      nn.Conv2d(256, 1024, 3), nn.ReLU())
        self.pool = nn.Sequential(nn.AvgPool2d((6, 6)), nn.ReLU())
        self.linear = nn.Sequential(nn.Linear(1024, 256), nn.BatchNorm1d(256))
        self.last = nn.Linear(256, 2)

    # ---- trunk: conv_seq -> pool -> linear(+BN); the packs are the trunk's alone (``last`` and a subclass's heads read their own) ----
    def _pack_tensors(self):
        bn = self.linear[1]
        return [self.conv_seq[i].weight for i in (0, 2, 4, 6)] + [self.conv_seq[i].bias for i in (0, 2, 4, 6)] + [
            self.linear[0].weight, self.linear[0].bias, bn.weight, bn.bias, bn.running_mean, bn.running_var]

    def _build_packs(self):
        bn = self.linear[1]
        dt = getattr(self, "compute_dtype", torch.float32)      # fp32 (exact) | fp16 MFMA trunk (config 5)
        convs = [ops.pack_conv(self.conv_seq[i].weight, self.conv_seq[i].bias, dtype=dt) for i in (0, 2, 4, 6)]
        lin = ops.pack_conv(self.linear[0].weight, self.linear[0].bias,
                            (bn.weight, bn.bias, bn.running_mean, bn.running_var), bn_eps=bn.eps, dtype=dt)
        return convs, lin

    _packed_trunk = PackedWeights.packed

    def trunk_nhwc(self, x: torch.Tensor) -> torch.Tensor:
        """x NHWC [K,14,14,256] -> x3 [K,256]   (ref :67-69 / :93-95)."""
        if x.shape[0] == 0:
            return torch.empty((0, 256), dtype=torch.float32, device=x.device)
        convs, lin = self._packed_trunk()
        if (x.dtype == torch.float32 and ops.CONV_TRACE is None and tuple(x.shape[1:]) == (14, 14, 256)
                and all(pc.dtype == torch.float32 for pc in convs)):
            return ops.match_trunk(x, convs, lin)     # one ABI call (seam_match_trunk_f32): the same six launches
        for pc in convs:                       # 14 -> 12 -> 10 -> 8 -> 6, ReLU fused
            x = ops.conv2d(x, pc, relu=True)
        x = ops.avgpool(x)                     # AvgPool2d(6,6); the following ReLU is a no-op (x >= 0)
        return ops.linear(x, lin, out_f32=True)   # Linear + BatchNorm1d(eval) epilogue; descriptors are always fp32

    def trunk(self, x: torch.Tensor) -> torch.Tensor:
        """x NCHW [K,256,14,14] (the reference's layout) -> x3 [K,256]."""
        if _wants_tape(self, x):
            return self.trunk_taped(x)
        dt = getattr(self, "compute_dtype", torch.float32)
        x = x.detach()
        if (x.dim() == 4 and x.is_cuda and x.shape[0] > 0 and x.permute(0, 2, 3, 1).is_contiguous()
                and ((x.dtype == torch.float32 and dt != torch.float16) or (x.dtype == torch.float16 and dt == torch.float16))):
            # channels_last input (what the extractor hands out as 'roi_features' with roi_features_contiguous = False): already
            # the kernels' NHWC layout, in the trunk's own precision
            return self.trunk_nhwc(x.permute(0, 2, 3, 1))
        return self.trunk_nhwc(ops.nchw_to_nhwc(x.to(torch.float32), torch.float16 if dt == torch.float16 else torch.float32))

    def trunk_taped(self, x: torch.Tensor) -> torch.Tensor:
        """The trunk as ONE autograd node (fp32): forward kernels + BatchNorm1d batch statistics when the BN layer
        is in training mode; backward = csrc/seam_backward.hip.  Mirrors nn.BatchNorm1d's buffer updates."""
        from ..autograd import TrunkFunction
        bn = self.linear[1]
        if not x.is_cuda:
            raise ops._native.SeamNativeError("x: expected a tensor on the HIP device (no CPU path exists)")
        bn_train = bn.training or bn.running_mean is None
        momentum = 0.0
        if bn_train and bn.track_running_stats and bn.running_mean is not None:
            bn.num_batches_tracked += 1
            momentum = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
        c = self.conv_seq
        rm = bn.running_mean if bn.track_running_stats else None
        rv = bn.running_var if bn.track_running_stats else None
        if not bn_train and rm is None:
            raise NotImplementedError("BatchNorm1d without running statistics in eval mode")
        return TrunkFunction.apply(x, c[0].weight, c[0].bias, c[2].weight, c[2].bias, c[4].weight, c[4].bias,
                                   c[6].weight, c[6].bias, self.linear[0].weight, self.linear[0].bias, bn.weight, bn.bias,
                                   rm, rv, bn_train, momentum, bn.eps)

    def pair(self, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
        """x5 = last((a_i - b_j)^2): [Q,256] x [G,256] -> [Q,G,2]   (ref :73-74, :161-162)."""
        if torch.is_grad_enabled() and (a.requires_grad or b.requires_grad or self.last.weight.requires_grad):
            from ..autograd import PairLogitsFunction
            return PairLogitsFunction.apply(a, b, self.last.weight, self.last.bias)
        return ops.pair_logits(a, b, self.last.weight, self.last.bias)

    def forward(self, x, types):
        x3 = self.trunk(x)
        types = torch.as_tensor(types).to(x3.device)       # callers pass a CPU IntTensor (video_matchrcnn.py:307)
        x5 = self.pair(x3[types == 0], x3[types == 1])
        return x3, x5


class TemporalAggregationNLB(MatchPredictor):
    def __init__(self, d_model=256):
        super().__init__()
        # same parameters and same forward as MatchPredictor, plus temporal aggregation (ref :81-88)
        self.n_frames = -1
        self.attention_scorer = nn.Linear(d_model, 1)
        self.newnlb = NONLocalBlock1D(in_channels=d_model, sub_sample=False, bn_layer=False)
        self.nlb = True

    # ---- sequence aggregation: NLB (len > 1) + softmax attention pooling ---------------------------
    def aggregate(self, seq_tm: torch.Tensor, lens: torch.Tensor, want_att: bool = False):
        """seq_tm: time-major [T,S,256] (rows >= len[s] ignored); lens int32 [S] on device."""
        t, s = seq_tm.shape[0], seq_tm.shape[1]
        pk = self.newnlb.packed(self.attention_scorer)
        n = self.newnlb
        params = (n.theta.weight, n.theta.bias, n.phi.weight, n.phi.bias, n.g.weight, n.g.bias, n.concat_project[0].weight,
                  n.W.weight, n.W.bias, self.attention_scorer.weight, self.attention_scorer.bias)
        if torch.is_grad_enabled() and (seq_tm.requires_grad or any(p.requires_grad for p in params)):
            from ..autograd import NlbAttnPoolFunction
            out = NlbAttnPoolFunction.apply(seq_tm, lens, 1 if self.nlb else 0, *params)
            att = None
            if want_att:
                with torch.no_grad():
                    _, att = ops.nlb_attnpool(seq_tm.detach(), s * 256, 256, lens, s, t, pk, use_nlb=1 if self.nlb else 0,
                                              want_att=True)
            return out, att
        return ops.nlb_attnpool(seq_tm, s * 256, 256, lens, s, t, pk, use_nlb=1 if self.nlb else 0,
                                want_att=want_att)

    def forward(self, x, types, ids, x3_1_seq=None, x3_1_mask=None, x3_2=None, getatt=False):
        attention_scores = None
        if x3_1_seq is None:
            # ---------------- Mode A: raw ROI features (ref :92-132) ----------------
            x3 = self.trunk(x)
            dev = x3.device
            types_c = torch.as_tensor(types).cpu()
            ids_c = torch.as_tensor(ids).cpu()
            plan = device_plan(types_c, ids_c, dev)
            x3_1_ids_c = plan["ids0"]
            x3_2 = x3[plan["sel1"]]
            if plan["n0"] > 0:
                # packing rules: sequences ordered by sorted unique id; maxlen = modal count;
                # dummy zero row 0; mask True on padding (ref :98-111)
                n_seqs, maxlen, counts = plan["n_seqs"], plan["maxlen"], plan["counts"]
                x3_1_seq = torch.zeros((1 + maxlen, n_seqs, 256), device=dev, dtype=x3.dtype)
                x3_1_seq[plan["pos1"], plan["seq_of_row"]] = x3[plan["rows"]]
                x3_1_mask = plan["mask"].clone()
                x3_1b, att = self.aggregate(x3_1_seq[1:], plan["lens"], getatt)
                if getatt:
                    attention_scores = [att[i, :int(c)].reshape(-1, 1) for i, c in enumerate(counts)]
            else:
                x3_1b = None
            x3_1_ids = x3_1_ids_c.to(torch.as_tensor(ids).device) if isinstance(ids, torch.Tensor) else x3_1_ids_c
        else:
            # ---------------- Mode B: pre-extracted descriptors (ref :133-158) ----------------
            dev = x3_1_seq.device
            tp1, n_seqs = x3_1_seq.shape[0], x3_1_seq.shape[1]
            m = x3_1_mask.to(dev)
            first = torch.where(m.any(1), m.to(torch.int32).argmax(1), torch.full((n_seqs,), tp1, device=dev))
            lens = (first - 1).clamp(min=0).to(torch.int32)             # slice 1:first_masked (ref :136-139)
            seq = x3_1_seq.to(torch.float32).contiguous()
            x3_1b, att = self.aggregate(seq[1:], lens, getatt)
            if getatt:
                lc = lens.cpu().tolist()
                attention_scores = [att[i, :n].reshape(-1, 1) for i, n in enumerate(lc)]
            x3_2 = x3_2.to(torch.float32)
            if x3_2.dim() == 1:
                x3_2 = x3_2[None]
            x3_1_ids = torch.zeros((1, 2))      # just to have numel > 0 (ref :158)

        x5 = self.pair(x3_1b, x3_2) if x3_1b is not None else None
        if getatt:
            return x3_1b, x3_2, x5, x3_1_seq, x3_1_mask, x3_1_ids, attention_scores
        return x3_1b, x3_2, x5, x3_1_seq, x3_1_mask, x3_1_ids


TemporalAggregation = TemporalAggregationNLB


# the loss classes the reference's training loops import from this module (ref stuffs/engine.py:11-12)
from .losses import (AggregationMatchLossDF2, MatchLossDF2, MatchLossWeak,          # noqa: E402,F401
                     NEWBalancedAggregationMatchLossWeak)
