#!/usr/bin/env python3
"""Mask intersections for segm AP, one image: ``ops.mask_inter`` (seam_mask_inter_f32, no pasted mask) against the torch
formulation on the existing paste kernel (paste [K,1,H,W] fp32, threshold, intersect with every ground truth -- the
evaluator's slow route).  Both are timed with device events in ONE process, alternating, after a warm-up; the report gives
median and minimum, the peak allocator bytes of one call of each, and the host time of the COCO matching per image.

usage: det_eval_bench.py [--height 800] [--width 1216] [--dets 100] [--gts 8] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from seam_match_rcnn_amd import evaluator_det as E
from seam_match_rcnn_amd import ops


def make_image(h, w, n_det, n_gt, seed=0):
    """Detections of mixed sizes (sides log-uniform 16 px ... the image) with blob-shaped probability maps; elliptic ground
    truths.  Everything from one seed."""
    rng = np.random.RandomState(seed)
    side = np.exp(rng.uniform(np.log(16.0), np.log(float(min(h, w))), size=(n_det, 2)))
    bw, bh = np.minimum(side[:, 0] * 1.3, w - 1.0), np.minimum(side[:, 1], h - 1.0)
    x, y = rng.uniform(0, w - bw), rng.uniform(0, h - bh)
    boxes = np.stack([x, y, x + bw, y + bh], 1).astype(np.float32)
    yy, xx = np.mgrid[0:28, 0:28]
    r = rng.uniform(8.0, 15.0, size=(n_det, 1, 1))
    dist = np.sqrt((yy - 13.5) ** 2 + (xx - 13.5) ** 2)[None]
    probs = 1.0 / (1.0 + np.exp((dist - r) * 1.5)) + rng.normal(0, 0.05, size=(n_det, 28, 28))
    gt, gt_boxes = np.zeros((n_gt, h, w), dtype=np.uint8), np.zeros((n_gt, 4), dtype=np.float32)
    Y, X = np.mgrid[0:h, 0:w]
    for g in range(n_gt):
        cy, cx, ry, rx = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(40, h / 2), rng.uniform(40, w / 3)
        gt[g] = (((Y - cy) / ry) ** 2 + ((X - cx) / rx) ** 2 <= 1.0)
        gt_boxes[g] = [max(cx - rx, 0), max(cy - ry, 0), min(cx + rx, w), min(cy + ry, h)]
    return (torch.from_numpy(np.clip(probs, 0, 1).astype(np.float32))[:, None].contiguous(), torch.from_numpy(boxes),
            torch.from_numpy(gt), torch.from_numpy(gt_boxes))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (a median of fewer says little)")
    if not torch.cuda.is_available():
        sys.exit("det_eval_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    probs, boxes, gt, gt_boxes = make_image(h, w, a.dets, a.gts)
    probs, boxes, gt = probs.to(dev), boxes.to(dev), gt.to(dev)

    def new_route():
        return ops.mask_inter(probs, boxes, gt)

    def torch_route():
        pasted = ops.paste_masks(probs, boxes, (h, w))
        inter, area, _ = E.DetectionEvaluator._mask_tables(dict(masks=pasted, boxes=boxes), dict(masks=gt))
        return inter, area

    routes = (("ops.mask_inter", new_route), ("paste + threshold + intersect (torch)", torch_route))
    for _ in range(a.warmup):
        outs = [fn() for _, fn in routes]
    torch.cuda.synchronize()
    same = torch.equal(outs[0][0].long(), outs[1][0].long()) and torch.equal(outs[0][1].long(), outs[1][1].long())
    times = {name: [] for name, _ in routes}
    for _ in range(a.reps):                                   # alternate the two inside one process
        for name, fn in routes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    peaks = {}
    for name, fn in routes:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        del out

    # host side of the protocol: 8 images with these tables, labels spread over 3 classes
    ev = E.DetectionEvaluator()
    n_img = 8
    t0 = time.perf_counter()
    for i in range(n_img):
        r = np.random.RandomState(100 + i)
        ev.update([dict(boxes=boxes, labels=torch.from_numpy(r.randint(1, 4, size=a.dets)).to(dev),
                        scores=torch.from_numpy(r.permutation(a.dets).astype(np.float32) / a.dets).to(dev), mask_probs=probs)],
                  [dict(boxes=gt_boxes, labels=torch.from_numpy(r.randint(1, 4, size=a.gts)), masks=gt)])
    torch.cuda.synchronize()
    t_update = (time.perf_counter() - t0) / n_img
    t0 = time.perf_counter()
    ev.summarize(verbose=False)
    t_match = (time.perf_counter() - t0) / n_img

    lines = ["command: " + " ".join([os.path.basename(sys.argv[0])] + sys.argv[1:]),
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP {torch.version.hip}",
             f"one image {h} x {w}, {a.dets} detections of mixed sizes (box area {float(((boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])).sum()):.0f} px in all), "
             f"{a.gts} ground truths; device events, {a.warmup} warm-up + {a.reps} timed calls of each route, alternating",
             f"pasted masks of this image, counted from the shape: {a.dets * h * w * 4 / 1e6:.0f} MB fp32",
             f"identical integer tables from both routes: {same}"]
    for name, _ in routes:
        t = times[name]
        lines.append(f"{name:<40s} median {statistics.median(t):8.3f} ms   min {min(t):8.3f} ms   max {max(t):8.3f} ms   "
                     f"peak allocator bytes {peaks[name]:>12d}")
    a_t, b_t = statistics.median(times[routes[0][0]]), statistics.median(times[routes[1][0]])
    lines.append(f"ratio of medians (torch route / ops.mask_inter): {b_t / a_t:.1f}x")
    lines.append(f"host, per image ({n_img} images, 3 classes): update() incl. its one copy {t_update * 1e3:.2f} ms; "
                 f"summarize() (matching + accumulation, bbox and segm) {t_match * 1e3:.2f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
