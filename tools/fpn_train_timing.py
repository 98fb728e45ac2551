#!/usr/bin/env python3
"""Time of one phase-1 training step of ``matchrcnn_resnet50_fpn`` (GPU box; HIP events): batch 8 at 800x1333, 512 RoI samples
and 256 anchors per image -- forward of the six losses + backward, no optimizer step.

  frozen      the whole backbone frozen (runs unchanged on a checkout that has no FPN training: only the public model API)
  fpn         backbone.body frozen, backbone.fpn trainable
  parts       with --parts: the new adjoints and the dense FPN backward alone, on the shapes of that step
Usage: python tools/fpn_train_timing.py [--parts] [--reps N] [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import seam_match_rcnn_amd.synth as synth
from seam_match_rcnn_amd import ops
from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params

dev = torch.device("cuda:0")
N, H, W, NCLS = 8, 800, 1333, 14


def timeit(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def batch():
    g = torch.Generator().manual_seed(0)
    images, targets = [], []
    for i in range(N):
        images.append(torch.from_numpy(synth.frames(70 + i, 1, H, W)[0]).to(dev))
        ng = 1 + i % 4
        wh = 60 + torch.rand((ng, 2), generator=g) * 340
        xy = torch.rand((ng, 2), generator=g) * (torch.tensor([float(W), float(H)]) - wh)
        gt = torch.cat([xy, xy + wh], 1)
        masks = torch.zeros((ng, H, W), dtype=torch.uint8)
        for j, b in enumerate(gt.round().to(torch.int64).tolist()):
            masks[j, b[1]:b[3], b[0]:b[2]] = 1
        targets.append(dict(boxes=gt.to(dev), labels=torch.randint(1, NCLS, (ng,), generator=g).to(dev), masks=masks.to(dev),
                            pair_ids=torch.randint(0, 3, (ng,), generator=g), styles=torch.randint(1, 3, (ng,), generator=g),
                            sources=torch.tensor([i % 2])))
    return images, targets


def model(fpn_trainable):
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS, **params)
    sd = synth.detector_state(5, NCLS)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    for p in m.backbone.parameters():
        p.requires_grad_(False)
    if fpn_trainable:
        for p in m.backbone.fpn.parameters():
            p.requires_grad_(True)
    return m.to(dev).train()


def step_of(m, images, targets):
    def step():
        m.rpn.sample_generator = torch.Generator(device=dev).manual_seed(1)
        m.roi_heads.sample_generator = torch.Generator(device=dev).manual_seed(2)
        m.zero_grad(set_to_none=True)
        losses = m(images, targets)
        sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
    return step


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    if "--reps" in sys.argv:
        args = [a for a in args if a != str(reps)]
    images, targets = batch()
    lines = [f"phase-1 training step, {N} frames {H}x{W}, 512 RoI samples + 256 anchors per image; ms per step (HIP events, {reps} steps)"]
    lines.append(f"frozen  whole backbone frozen                         {timeit(step_of(model(False), images, targets), reps):9.2f}")
    if hasattr(ops, "roi_align_bwd"):
        lines.append(f"fpn     body frozen, FPN trainable                    {timeit(step_of(model(True), images, targets), reps):9.2f}")
    if "--parts" in sys.argv and hasattr(ops, "roi_align_bwd"):
        from seam_match_rcnn_amd.autograd import FPNFunction
        g = torch.Generator().manual_seed(3)
        hws = [(200, 336), (100, 168), (50, 84), (25, 42)]
        scales = [0.25, 0.125, 0.0625, 0.03125]

        def rois(k):
            wh = 16 + torch.rand((k, 2), generator=g) * 500
            xy = torch.rand((k, 2), generator=g) * torch.tensor([float(W), float(H)]) * 0.8
            return torch.cat([(torch.arange(k) % N).float()[:, None], xy, xy + wh], 1).to(dev)
        rb, rm = rois(N * 512), rois(N * 128)
        db, dm = torch.randn((N * 512, 7, 7, 256), device=dev), torch.randn((N * 128, 14, 14, 256), device=dev)
        lines.append(f"  part  roi_align_bwd 7x7, {N * 512} ROIs                  {timeit(lambda: ops.roi_align_bwd(db, rb, hws, N, scales), reps):9.2f}")
        lines.append(f"  part  roi_align_bwd 14x14, {N * 128} ROIs                {timeit(lambda: ops.roi_align_bwd(dm, rm, hws, N, scales), reps):9.2f}")
        hw5 = hws + [(13, 21)]
        m_rows = N * 256
        rows = torch.stack([torch.arange(m_rows) % N, torch.arange(m_rows) % 5, torch.arange(m_rows) % 13,
                            torch.arange(m_rows) * 7 % 21], 1).to(torch.int32).to(dev)
        dp = torch.randn((m_rows, 3, 3, 256), device=dev)
        lines.append(f"  part  rpn_scatter_patches, {m_rows} rows                 {timeit(lambda: ops.rpn_scatter_patches(dp, rows, hw5, N), reps):9.2f}")
        fpn = model(True).backbone.fpn
        cs = [torch.randn((N, h, w, c), device=dev) * 0.1 for (h, w), c in zip(hws, (256, 512, 1024, 2048))]
        ups = [torch.randn((N, h, w, 256), device=dev) for h, w in hw5]

        def fpn_fwd_bwd():
            fpn.zero_grad(set_to_none=True)
            out = fpn.forward_taped(cs)
            torch.autograd.backward(list(out.values()), ups)

        def fpn_fwd():
            with torch.no_grad():
                fpn.forward_taped(cs)
        t_all, t_fwd = timeit(fpn_fwd_bwd, reps), timeit(fpn_fwd, reps)
        lines.append(f"  part  FPN forward (taped form, single stream)        {t_fwd:9.2f}")
        lines.append(f"  part  FPN backward: dense dgrad + wgrad + colsum + merges {t_all - t_fwd:9.2f}")
    print("\n".join(lines))
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
