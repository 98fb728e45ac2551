#!/usr/bin/env python3
"""Time of one phase-1 training step of ``matchrcnn_resnet50_fpn`` with a trainable ResNet body (GPU box; HIP events): the step of
tools/fpn_train_timing.py -- batch 8 at 800x1333, 512 RoI samples and 256 anchors per image, forward of the six losses + backward,
no optimizer step.

  frozen      the whole backbone frozen
  fpn         backbone.body frozen, backbone.fpn trainable
  body234     trainable_backbone_layers=3: layer2..layer4 + the FPN (the reference's configuration)
  body1234    trainable_backbone_layers=4: layer1 as well
  body_all    trainable_backbone_layers=5, train_stem=True: the stem (conv1 through its max-pool) as well
  parts       the three 3x3 / stride-2 input gradients on the step's shapes under SEAM_S2_DGRAD=1 (the gather kernel) and =0 (dy
              zero-stuffed + the stride-1 dgrad), the per-step weight packing of the body, and the two steps of the stem backward:
              the max-pool + ReLU adjoint (against its compulsory traffic 2 |y| + |dpool|) and conv1's weight gradient on the
              space-to-depth frame the step feeds (and on the NHWC4 form)
Usage: python tools/body_train_timing.py [--reps N] [out.txt]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from fpn_train_timing import N, NCLS, batch, dev, model, step_of, timeit  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import seam_match_rcnn_amd.synth as synth  # noqa: E402
from seam_match_rcnn_amd import _native, ops  # noqa: E402
from seam_match_rcnn_amd.autograd import _scaled  # noqa: E402
from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params  # noqa: E402


def body_model(layers, train_stem=False):
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS, trainable_backbone_layers=layers, train_stem=train_stem,
                               **params)
    sd = synth.detector_state(5, NCLS)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    return m.to(dev).train()


def dgrad_packs(body, first_layer):
    """The packing ``autograd.BodyFunction.backward`` does once per step: every conv of layer ``first_layer``.. in its dgrad form."""
    pk = body.packed()
    for li, bi, b in body.blocks():
        if li < first_layer:
            continue
        e = pk[(li, bi)]
        ops.pack_conv_dgrad(_scaled(b.conv3.weight, e["c3"].scale))
        if b.stride == 2:
            ops.pack_conv3x3s2_dgrad(b.conv2.weight, e["c2"].scale)
        else:
            ops.pack_conv_dgrad(_scaled(b.conv2.weight, e["c2"].scale), pad_fwd=1)
        ops.pack_conv_dgrad(_scaled(b.conv1.weight, e["c1"].scale))
        if b.downsample is not None:
            ops.pack_conv_dgrad(_scaled(b.downsample[0].weight, e["ds"].scale))


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    if "--reps" in sys.argv:
        args = [a for a in args if a != str(reps)]
    images, targets = batch()
    lines = [f"phase-1 training step, {N} frames 800x1333, 512 RoI samples + 256 anchors per image; ms per step (HIP events, {reps} steps)"]
    lines.append(f"frozen    whole backbone frozen                       {timeit(step_of(model(False), images, targets), reps):9.2f}")
    lines.append(f"fpn       body frozen, FPN trainable                  {timeit(step_of(model(True), images, targets), reps):9.2f}")
    for name, layers, what in (("body234 ", 3, "layer2..4 + FPN trainable (the reference)"), ("body1234", 4, "layer1..4 + FPN trainable            "),
                               ("body_all", 5, "stem + layer1..4 + FPN (train_stem)   ")):
        m = body_model(layers, train_stem=layers == 5)
        torch.cuda.reset_peak_memory_stats()
        t = timeit(step_of(m, images, targets), reps)
        lines.append(f"{name}  {what}  {t:9.2f}   (peak device memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB)")
        del m
        torch.cuda.empty_cache()
    # the three stride-2 input gradients of the step: dy of layer{2,3,4}.0.conv2, masked by the block's first activation
    g = torch.Generator().manual_seed(3)
    before = _native.get_option("SEAM_S2_DGRAD")
    for li, (h, w, c) in ((2, (200, 336, 128)), (3, (100, 168, 256)), (4, (50, 84, 512))):
        dy = torch.randn((N, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c), generator=g).to(dev)
        mask = torch.randn((N, h, w, c), generator=g).to(dev)
        pk = ops.pack_conv3x3s2_dgrad((torch.randn((c, c, 3, 3), generator=g) * 0.05).to(dev), (torch.rand((c,), generator=g) + 0.5).to(dev))
        ts = []
        for sel in (1, 0):
            _native.set_option("SEAM_S2_DGRAD", sel)
            ts.append(timeit(lambda: ops.conv3x3s2_dgrad(dy, pk, (h, w), mask=mask), reps))
        _native.set_option("SEAM_S2_DGRAD", before)
        flop = 2.0 * N * ((h - 1) // 2 + 1) * ((w - 1) // 2 + 1) * 9 * c * c
        lines.append(f"  part  layer{li}.0.conv2 dgrad [{N},{h},{w},{c}]  SEAM_S2_DGRAD=1 {ts[0]:7.3f} ({flop / ts[0] * 1e-9:5.1f} TF)   =0 {ts[1]:7.3f}")
    # the stem backward on the step's shapes: y0 = the stem output of 8 frames padded to 800 x 1344, the frame in both forms
    hs, wst = 400, 672
    y0 = torch.randn((N, hs, wst, 64), generator=g).clamp_(min=0).to(dev)
    dpool = torch.randn((N, hs // 2, wst // 2, 64), generator=g).to(dev)
    t = timeit(lambda: ops.maxpool3s2_relu_bwd(y0, dpool), reps)
    gb = (2 * y0.numel() + dpool.numel()) * 4e-9
    lines.append(f"  part  max-pool + ReLU adjoint [{N},{hs},{wst},64]   {t:7.3f}   ({gb:.2f} GB compulsory: {gb / t:5.2f} TB/s)")
    dy0 = ops.maxpool3s2_relu_bwd(y0, dpool)
    del dpool
    fs = torch.randn((N, hs, wst, 12), generator=g).to(dev)
    t = timeit(lambda: ops.conv_wgrad_chunked(fs, dy0, 4, 4, 1, 2, out_hw=(hs, wst)), reps)
    lines.append(f"  part  conv1 wgrad, space-to-depth frame [{N},{hs},{wst},12], 4x4 cropped   {t:7.3f}")
    del fs
    f4 = torch.randn((N, 2 * hs, 2 * wst, 4), generator=g).to(dev)
    t = timeit(lambda: ops.conv_wgrad_chunked(f4, dy0, 7, 7, 2, 3), reps)
    lines.append(f"  part  conv1 wgrad, NHWC4 frame [{N},{2 * hs},{2 * wst},4], 7x7 / stride 2       {t:7.3f}")
    del f4, y0, dy0
    torch.cuda.empty_cache()
    body = body_model(3).backbone.body

    def repack():
        body._pk = None
        body.packed()
    lines.append(f"  part  forward weights of the body repacked (after an optimizer step)   {timeit(repack, reps):7.3f}")
    lines.append(f"  part  dgrad weights of layer2..4 packed (once per backward)             {timeit(lambda: dgrad_packs(body, 2), reps):7.3f}")
    lines.append(f"  part  dgrad weights of layer1..4 packed                                 {timeit(lambda: dgrad_packs(body, 1), reps):7.3f}")
    print("\n".join(lines))
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
