#!/usr/bin/env python3
"""RLE operations on bitmaps (csrc/seam_rle.hip: bits from runs, combine, pair intersections) at one image's size: 100 detection
RLEs (``encode_detections`` of seeded probabilities) against 8 ground-truth RLEs (seeded garment outlines) on 800 x 1216.

  (i)   ``mask_utils.iou`` through the bit kernels against the route it had before, kept here as ``iou_dense``: decode both sides
        into uint8 [n,H,W] stacks, intersect them with torch in a loop over the ground truths.  Both end to end (string decode,
        table packing, upload, kernels, the copy of the table to the host) and their device parts alone (tables packed before).
  (ii)  ``mask_utils.merge`` of the 8 ground-truth RLEs, union and intersection.
  (iii) ``evaluator_det.evaluate_results`` on a synthetic file of 64 images of that size (--eval-dets detections and --eval-gts
        polygon ground truths each), end to end and the mask tables alone.
Everything is timed with device events after a warm-up, the two iou routes alternating; each timed span ends in a copy to the
host or a synchronise.  The bytes each route writes on the device are counted from the shapes.  The tables of both iou routes are
compared first.

usage: rle_algebra_bench.py [--dets 100] [--gts 8] [--height 800] [--width 1216] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mask_raster_bench import garment
from rle_encode_bench import make_detections
from seam_match_rcnn_amd import evaluator_det as E
from seam_match_rcnn_amd import mask_utils as M
from seam_match_rcnn_amd import ops, ops_masks


def iou_dense(dt, gt, iscrowd):
    """``mask_utils.iou`` on RLE lists as it was before the bit kernels: both sides decoded into dense stacks."""
    crowd = np.asarray(iscrowd, dtype=np.int64).reshape(-1) != 0
    dm, gm = M.decode(dt, keep_on_device=True) != 0, M.decode(gt, keep_on_device=True) != 0
    inter = torch.stack([(dm & g[None]).sum((1, 2)) for g in gm], 1)
    table = torch.cat([inter.reshape(-1).to(torch.float64), dm.sum((1, 2)).to(torch.float64),
                       gm.sum((1, 2)).to(torch.float64)]).cpu().numpy()
    nd, ng = len(dt), len(gt)
    return E._mask_iou(table[:nd * ng].reshape(nd, ng), table[nd * ng:nd * ng + nd], table[nd * ng + nd:], crowd)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def line(name, ms):
    return f"{name:<72s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--eval-images", type=int, default=64)
    ap.add_argument("--eval-dets", type=int, default=20)
    ap.add_argument("--eval-gts", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (a median of fewer says little)")
    if not torch.cuda.is_available():
        sys.exit("rle_algebra_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w, nd, ng = a.height, a.width, a.dets, a.gts
    rng = np.random.default_rng(0)
    probs, boxes = (t.to(dev) for t in make_detections(nd, h, w))
    dt = M.encode_detections(probs, boxes, (h, w))
    outlines = [[garment(rng, h, w, int(rng.integers(40, 300)))] for _ in range(ng)]
    gt = M.encode(M.masks_from_annotations([outlines], [(h, w)], dev)[0])
    crowd = [int(k == ng - 1) for k in range(ng)]
    out = [f"RLE algebra on bitmaps: {nd} detection RLEs x {ng} ground-truth RLEs on {h} x {w}; {a.reps} reps after {a.warmup} warm-up",
           f"device: {torch.cuda.get_device_name(0)}",
           f"runs per RLE: detections median {int(np.median([len(M.rle_from_string(r['counts'])) for r in dt]))}, "
           f"ground truths median {int(np.median([len(M.rle_from_string(r['counts'])) for r in gt]))}"]

    # ---- (i) iou
    bits, dense = M.iou(dt, gt, crowd), iou_dense(dt, gt, crowd)
    if not np.array_equal(bits, dense):
        sys.exit("the two iou routes disagree")
    out.append(f"iou tables of both routes are equal ({int((bits > 0).sum())} of {bits.size} pairs overlap)")
    d_counts = [M._counts(r, "dt") for r in dt]
    g_counts = [M._counts(r, "gt") for r in gt]
    pairs = np.stack(np.meshgrid(np.arange(nd), nd + np.arange(ng), indexing="ij"), -1).reshape(-1, 2)

    def device_bits():
        ws, lay = ops.rle_bits(d_counts + g_counts, [(h, w)] * (nd + ng))
        return ops.bits_inter(ws, lay, pairs)

    def device_dense():
        dm = ops.rle_masks([d_counts], [(h, w)], dev)[0] != 0
        gm = ops.rle_masks([g_counts], [(h, w)], dev)[0] != 0
        return torch.stack([(dm & g[None]).sum((1, 2)) for g in gm], 1), dm.sum((1, 2)), gm.sum((1, 2))

    routes = {"iou, bit kernels, end to end": lambda: M.iou(dt, gt, crowd), "iou, dense decode (previous route), end to end": lambda: iou_dense(dt, gt, crowd),
              "  device part: bits from runs + pair popcounts (incl. table upload)": device_bits,
              "  device part: rle_masks x2 + torch and/sum over the ground truths": device_dense}
    ms = {k: [] for k in routes}
    for rep in range(a.warmup + a.reps):
        for k, fn in routes.items():                                     # alternating
            t = timed(fn)
            if rep >= a.warmup:
                ms[k].append(t)
    out += [line(k, v) for k, v in ms.items()]
    names = list(routes)
    ratio = statistics.median(ms[names[1]]) / statistics.median(ms[names[0]])
    ratio_dev = statistics.median(ms[names[3]]) / statistics.median(ms[names[2]])
    out.append(f"dense / bits: end to end {ratio:.2f}x, device parts {ratio_dev:.2f}x")
    cells = 4 * ops.rle_bits_cells([(h, w)])[0]
    out.append(f"bytes written on the device, from the shapes: bits {(nd + ng) * cells + 8 * (nd * ng + nd + ng)} "
               f"({nd + ng} bitmaps of {cells} B + the int64 table); dense {(nd + ng) * h * w * 2 + ng * nd * h * w + 8 * (nd * ng + nd + ng)} "
               f"({nd + ng} uint8 masks and their bool copies of {h * w} B, {ng} bool [D,H,W] intersections + the table)")
    faster = "bit" if ratio >= 1.0 else "dense"
    out.append(f"mask_utils.iou uses the bit route; measured here the {faster} route is the faster one end to end"
               + ("" if faster == "bit" else " -- iou must keep the dense route (see the module)"))

    # ---- (ii) merge
    for name, flag in (("merge of the ground-truth RLEs, union", False), ("merge of the ground-truth RLEs, intersection", True)):
        t = [timed(lambda: M.merge(gt, intersect=flag)) for _ in range(a.warmup + a.reps)][a.warmup:]
        out.append(line(f"{name} ({ng} RLEs)", t))
    out.append(f"bytes written on the device by a merge: {(ng + 1) * cells} bitmap + {cells} counts + {2 * cells} scan (int64) bytes; "
               f"a dense route would write {ng * h * w} mask bytes first")

    # ---- (iii) evaluate_results
    n_img, e_d, e_g = a.eval_images, a.eval_dets, a.eval_gts
    images, annotations, results = [], [], []
    for i in range(n_img):
        p, b = (t.to(dev) for t in make_detections(e_d, h, w, seed=100 + i))
        sc = torch.from_numpy(rng.uniform(0.05, 1.0, e_d).astype(np.float32)).to(dev)
        lb = torch.from_numpy(rng.integers(1, 14, e_d)).to(dev)
        results += E.coco_results([dict(boxes=b, labels=lb, scores=sc, mask_probs=p)], [i], [(h, w)])
        images.append({"id": i, "height": h, "width": w})
        for k in range(e_g):
            poly = garment(rng, h, w, int(rng.integers(40, 300)))
            xs, ys = poly[0::2], poly[1::2]
            bb = [min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)]
            annotations.append({"id": len(annotations) + 1, "image_id": i, "category_id": int(rng.integers(1, 14)), "iscrowd": 0,
                                "bbox": bb, "area": bb[2] * bb[3] * 0.6, "segmentation": [poly]})
    gt_file = {"images": images, "annotations": annotations}
    t = [timed(lambda: E.evaluate_results(gt_file, results, verbose=False)) for _ in range(2 + 10)][2:]
    out.append(line(f"evaluate_results, {n_img} images x ({e_d} detections, {e_g} polygon ground truths), bbox + segm", t))
    t = [timed(lambda: E.evaluate_results(gt_file, results, iou_types=("bbox",), verbose=False)) for _ in range(2 + 10)][2:]
    out.append(line("  the same, bbox only (host)", t))
    anns = [[x for x in annotations if x["image_id"] == i] for i in range(n_img)]
    dets = [[x for x in results if x["image_id"] == i] for i in range(n_img)]
    chunks = ops.budget_chunks([cells * (e_d + e_g) + h * w * e_g] * n_img)
    t = [timed(lambda: [M.results_inter_tables(anns[lo:hi], dets[lo:hi], [(h, w)] * (hi - lo)) for lo, hi in chunks])
         for _ in range(2 + 10)][2:]
    out.append(line(f"  the mask tables alone ({len(chunks)} chunks of at most {ops_masks.RLE_BITS_BUDGET_BYTES >> 20} MiB)", t))
    out.append(f"bytes written on the device per chunk image: {(e_d + e_g) * cells} bitmap bytes + {e_g * h * w} dense ground-truth bytes "
               f"(polygons are rasterised densely, then bit-packed); no dense detection mask ({e_d * h * w} bytes per image) exists")
    text = "\n".join(out) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
