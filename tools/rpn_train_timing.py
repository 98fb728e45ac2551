#!/usr/bin/env python3
"""Time of the RPN's training branch next to the dense head forward it rides on (GPU box; HIP events).

8 frames at 800x1344 (268 569 anchors each), 1..8 GT boxes per frame:
  dense       rpn.head.fused(feats): the 3x3 conv + the fused 1x1 predictors on all 5 levels (what inference pays too)
  train       RegionProposalNetwork.training_losses + backward(): matching, sampling, the gather of the sampled windows, the
              head on <= 2048 rows, the two losses and the gradients of the six head parameters
  parts       the stages of `train`, each timed alone (the host copy of the sampled anchors sits in `train` only; the last part
              packs the weights, runs the head on the rows, the loss kernel and the five gradient launches)
Usage: python tools/rpn_train_timing.py [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from seam_match_rcnn_amd import ops
from seam_match_rcnn_amd.models import detection as det

dev = torch.device("cuda:0")
N, H, W = 8, 800, 1344


def timeit(fn, reps=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    hws = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
    feats = {k: (torch.randn((N, h, w, 256), generator=g) * 0.5).to(dev) for k, (h, w) in zip(("0", "1", "2", "3", "pool"), hws)}
    targets = []
    for i in range(N):
        wh = 30 + torch.rand((i + 1, 2), generator=g) * 270
        xy = torch.rand((i + 1, 2), generator=g) * (torch.tensor([float(W), float(H)]) - wh)
        targets.append(dict(boxes=torch.cat([xy, xy + wh], 1).to(dev)))
    rpn = det.RegionProposalNetwork().to(dev).train()
    fl = list(feats.values())

    def dense():
        with torch.no_grad():
            rpn.head.fused(fl)

    def train():
        rpn.zero_grad(set_to_none=True)
        losses = rpn.training_losses(feats, (H, W), targets)
        (losses["loss_objectness"] + losses["loss_rpn_box_reg"]).backward()

    anchors = torch.cat(rpn.anchors((H, W), hws, dev)).contiguous()
    n_gt = torch.tensor([len(t["boxes"]) for t in targets], dtype=torch.int32, device=dev)
    gtp = torch.zeros((N, 8, 4), device=dev)
    for i, t in enumerate(targets):
        gtp[i, :len(t["boxes"])] = t["boxes"]
    labels, matched = ops.rpn_match(anchors, gtp, n_gt)
    keys = torch.rand(labels.shape, device=dev)
    idx, slab, _, stg, count = ops.rpn_sample(labels, matched, keys, anchors, gtp)
    m = int(count[:, 0].sum())
    rows = torch.zeros((m, 4), dtype=torch.int32, device=dev)
    rows[:, 0] = torch.arange(m, device=dev) % N
    rows[:, 2] = torch.arange(m, device=dev) % 200
    rows[:, 3] = torch.arange(m, device=dev) % 336
    from seam_match_rcnn_amd.autograd import RPNHeadRowsFunction, RPNLossFunction
    patches = ops.rpn_gather_patches(fl, rows)
    keep = idx.reshape(-1) >= 0
    lab, tgt = slab.reshape(-1)[keep].contiguous(), stg.reshape(-1, 4)[keep].contiguous()
    slot = (torch.arange(m, device=dev) % 3).to(torch.int32)
    h = rpn.head

    def head_rows():
        rpn.zero_grad(set_to_none=True)
        o = RPNHeadRowsFunction.apply(patches, h.conv.weight, h.conv.bias, h.cls_logits.weight, h.cls_logits.bias,
                                      h.bbox_pred.weight, h.bbox_pred.bias)
        lo, lb = RPNLossFunction.apply(o, slot, lab, tgt, 3)
        (lo + lb).backward()

    lines = [f"RPN training branch, {N} frames {H}x{W}, {anchors.shape[0]} anchors per frame, {m} sampled rows; ms per call (HIP events)",
             f"dense  rpn.head.fused forward (5 levels)          {timeit(dense):8.3f}",
             f"train  training_losses + backward                 {timeit(train):8.3f}",
             f"  part seam_rpn_match_f32                         {timeit(lambda: ops.rpn_match(anchors, gtp, n_gt)):8.3f}",
             f"  part torch.rand keys [{N},{anchors.shape[0]}]                 {timeit(lambda: torch.rand(labels.shape, device=dev)):8.3f}",
             f"  part seam_rpn_sample_f32                        {timeit(lambda: ops.rpn_sample(labels, matched, keys, anchors, gtp)):8.3f}",
             f"  part seam_rpn_gather_patches_f32 ({m} rows)     {timeit(lambda: ops.rpn_gather_patches(fl, rows)):8.3f}",
             f"  part head on the rows + losses + backward        {timeit(head_rows):8.3f}"]
    print("\n".join(lines))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
