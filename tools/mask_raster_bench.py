#!/usr/bin/env python3
"""Ground-truth masks of one training batch: ``mask_utils.masks_from_annotations`` (annotations up, csrc/seam_masks.hip builds the
uint8 stacks on the device) against the route it replaces (masks built on the host, then copied over).

  (a) masks_from_annotations end to end: host packing + one table upload + the kernels, a host clock around a call that ends in a
      device synchronise; the host packing alone is reported next to it.
  (b) per kernel: not timed here.  Run ``rocprofv3 --kernel-trace --stats -d DIR -- python tools/mask_raster_bench.py --profile``
      (a run of its own: warm-up + calls of (a) only) and read poly_toggle_kernel / poly_scan_kernel / poly_expand_kernel in
      DIR's kernel stats.
  (c) the host route for the same masks: tests/mask_refs.py on the CPU (THIS PROJECT'S NumPy restatement, not pycocotools -- its
      time says nothing about pycocotools' C code and is printed for completeness only), plus the copy of the uint8 stacks from
      pinned memory to the device, timed with device events.  (a) against the copy alone is the fair comparison.
The two routes are alternated in one process after a warm-up, and their masks are compared byte for byte first.

usage: mask_raster_bench.py [--images 8] [--height 800] [--width 1216] [--reps 20] [--warmup 3] [--profile] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import mask_refs as R
from seam_match_rcnn_amd import mask_utils as M
from seam_match_rcnn_amd import ops


def garment(rng, h, w, k):
    """A closed outline of k vertices around a random centre, two decimals per coordinate as DeepFashion2 stores them."""
    th = np.sort(rng.uniform(0, 2 * np.pi, k))
    radius = rng.uniform(0.12, 0.45) * min(h, w)
    r = radius * (0.75 + 0.2 * np.sin(rng.integers(2, 7) * th + rng.uniform(0, 6.28))) + rng.uniform(-3, 3, k)
    cx, cy = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)
    return [float(v) for v in np.round(np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1).reshape(-1), 2)]


def make_batch(n_images, h, w, seed=0):
    """2 to 8 objects per image, 40 to 300 vertices per outline, every fourth object in two parts."""
    rng = np.random.default_rng(seed)
    batch = []
    for _ in range(n_images):
        objs = []
        for j in range(int(rng.integers(2, 9))):
            parts = [garment(rng, h, w, int(rng.integers(40, 301)))]
            if j % 4 == 3:
                parts.append(garment(rng, h, w, int(rng.integers(40, 120))))
            objs.append(parts)
        batch.append(objs)
    return batch


def stats(name, ms):
    return f"{name:<58s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile", action="store_true", help="warm-up and calls of the device route only (for rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (a median of fewer says little)")
    if not torch.cuda.is_available():
        sys.exit("mask_raster_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    h, w = a.height, a.width
    batch = make_batch(a.images, h, w)
    sizes = [(h, w)] * a.images
    n_obj = sum(len(o) for o in batch)

    def device_route():
        out = M.masks_from_annotations(batch, sizes, dev)
        torch.cuda.synchronize()
        return out

    for _ in range(a.warmup):
        device_route()
    if a.profile:
        for _ in range(a.reps):
            device_route()
        return
    _, tables = ops.pack_poly_masks(batch, sizes)
    table_bytes = sum(v.nbytes for v in tables.values() if isinstance(v, np.ndarray))
    t0 = time.perf_counter()
    host = [np.stack([R.poly_mask(p, h, w) for p in objs]) for objs in batch]
    host_ms = (time.perf_counter() - t0) * 1e3
    got = device_route()
    same = all(np.array_equal(g.cpu().numpy(), m) for g, m in zip(got, host))
    pinned = [torch.from_numpy(m).pin_memory() for m in host]
    stack_bytes = sum(m.nbytes for m in host)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(a.warmup):
        [p.to(dev, non_blocking=True) for p in pinned]
        torch.cuda.synchronize()
    t_dev, t_pack, t_copy = [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        device_route()
        t_dev.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ops.pack_poly_masks(batch, sizes)
        t_pack.append((time.perf_counter() - t0) * 1e3)
        e0.record()
        keep = [p.to(dev, non_blocking=True) for p in pinned]
        e1.record()
        torch.cuda.synchronize()
        t_copy.append(e0.elapsed_time(e1))
        del keep
    lines = [
        "command: mask_raster_bench.py" + "".join(f" {x}" for x in sys.argv[1:]),
        f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP {torch.version.hip}",
        f"{a.images} images {h} x {w}, {n_obj} objects (2 to 8 per image), {tables['P']} polygon parts, {tables['V']} vertices, "
        f"{tables['T']} boundary points; {a.warmup} warm-up + {a.reps} timed calls of each route, alternating",
        f"bytes, counted from the shapes: uploaded tables {table_bytes}, workspace {4 * int(tables['part_ws_off'][-1])}, "
        f"uint8 mask stacks {stack_bytes}",
        f"device masks equal the host restatement's, byte for byte: {same}",
        stats("(a) masks_from_annotations, end to end (host clock + sync)", t_dev),
        stats("    of which host packing (ops.pack_poly_masks, CPU)", t_pack),
        stats("(c) copy of the uint8 stacks, pinned memory -> device (events)", t_copy),
        f"(c) host rasterisation by tests/mask_refs.py (this project's NumPy restatement, NOT pycocotools), once: {host_ms:9.1f} ms",
        f"ratio of medians, (a) / copy alone: {statistics.median(t_dev) / statistics.median(t_copy):.2f}x",
        "(b) per kernel: see the rocprofv3 kernel stats of a --profile run",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        sys.exit("the device masks differ from the host restatement")


if __name__ == "__main__":
    main()
