#!/usr/bin/env python3
"""COCO RLE of one image's detections: ``mask_utils.encode_detections`` (csrc/seam_rle.hip, no pasted mask) against the route the
project needed before it, and the dense encoder on a batch of ground-truth masks.  One process, warm-up first, the routes
alternating; device parts are timed with device events, host parts with a host clock (a part that ends in a copy to the host ends
in a synchronise).

  (i)   encode_detections end to end, and the same steps one by one through the C ABI: value + count kernels, prefix sum,
        totals to the host, positions kernel, positions to the host, host diff, compressed strings.
  (ii)  what the parent commit would need: seam_paste_masks_f32 -> threshold -> copy of the uint8 [D,H,W] bytes to the host ->
        host run-length encode + strings.  The host encoder here is THIS PROJECT'S NumPy (a column-major diff), not pycocotools:
        its time says nothing about pycocotools' C code.  The fair lower bound of (ii) is paste + threshold + copy alone, and (i)
        is reported against that bound as well.
  (iii) ops.rle_encode on the ground-truth masks of 8 images (tools/mask_raster_bench.py's batch): the value + count kernels
        against a plain device copy of the same bytes, as achieved GB/s over the mask bytes.
The allocator's peak above the inputs is read from torch for each route.  All routes' strings are compared first.

usage: rle_encode_bench.py [--dets 100] [--gts 8] [--height 800] [--width 1216] [--reps 20] [--warmup 3] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch

from mask_raster_bench import make_batch
from seam_match_rcnn_amd import _native
from seam_match_rcnn_amd import mask_utils as M
from seam_match_rcnn_amd import ops


def make_detections(d, h, w, seed=0):
    """d garment-sized boxes and smooth 28x28 blobs with a noisy rim"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:28, 0:28]
    probs, boxes = [], []
    for _ in range(d):
        bw, bh = rng.uniform(0.1, 0.6) * w, rng.uniform(0.15, 0.8) * h
        x0, y0 = rng.uniform(-0.05 * w, w - 0.8 * bw), rng.uniform(-0.05 * h, h - 0.8 * bh)
        boxes.append([x0, y0, x0 + bw, y0 + bh])
        r = np.hypot((yy - rng.uniform(11, 16)) / rng.uniform(8, 13), (xx - rng.uniform(11, 16)) / rng.uniform(8, 13))
        probs.append(np.clip(1.2 - r + rng.normal(0, 0.05, (28, 28)), 0, 1))
    return torch.from_numpy(np.asarray(probs, np.float32))[:, None], torch.tensor(boxes, dtype=torch.float32)


def host_encode(masks):
    """uint8 [n,h,w] on the host -> counts per object, NumPy"""
    out = []
    for m in masks:
        flat = np.concatenate([[0], (m.T.reshape(-1) != 0).astype(np.int8)])
        out.append(np.diff(np.concatenate([[0], np.flatnonzero(np.diff(flat)), [m.size]])))
    return out


def line(name, ms):
    return f"{name:<66s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"


class Events:
    def __init__(self):
        self.marks = []

    def mark(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append(e)

    def spans(self):
        return [a.elapsed_time(b) for a, b in zip(self.marks, self.marks[1:])]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=8)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.reps < 10:
        ap.error("--reps must be at least 10 (a median of fewer says little)")
    if not torch.cuda.is_available():
        sys.exit("rle_encode_bench.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    lib = _native.lib()
    h, w, d = a.height, a.width, a.dets
    probs, boxes = (t.to(dev) for t in make_detections(d, h, w))
    stream = torch.cuda.current_stream().cuda_stream
    per = int(lib.seam_rle_encode_ws_bytes(h, w)) // 4
    cells = per * d
    last = torch.arange(1, d + 1, device=dev, dtype=torch.int64) * per - 1

    def route_new():
        return M.encode_detections(probs, boxes, (h, w))

    def route_new_steps(t):
        """the steps of ops.rle_encode_paste + mask_utils, timed one by one into the lists of ``t``"""
        ev = Events()
        ev.mark()
        ws = torch.empty((cells,), dtype=torch.int32, device=dev)
        counts = torch.empty((cells,), dtype=torch.int32, device=dev)
        _native.check(lib.seam_rle_encode_paste_f32(probs.data_ptr(), boxes.data_ptr(), d, h, w, ws.data_ptr(), 4 * cells,
                                                    counts.data_ptr(), stream), "encode")
        ev.mark()
        scan = torch.cumsum(counts, 0)
        ends_dev = scan[last]
        ev.mark()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ends = ends_dev.cpu().numpy()
        t["copy_totals"].append((time.perf_counter() - t0) * 1e3)
        total = int(ends[-1])
        ev.mark()
        pos = torch.empty((total,), dtype=torch.int32, device=dev)
        _native.check(lib.seam_rle_positions_paste(d, h, w, ws.data_ptr(), 4 * cells, scan.data_ptr(), pos.data_ptr(), total, stream),
                      "positions")
        ev.mark()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pos = pos.cpu().numpy()
        t["copy_positions"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        pos = pos.astype(np.int64)
        cs = ops.rle_counts_from_positions(pos, ends, [(h, w)] * d)
        t["host_diff"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        strings = M.counts_to_bytes(cs)
        t["host_strings"].append((time.perf_counter() - t0) * 1e3)
        sp = ev.spans()
        t["kernels_values_count"].append(sp[0])
        t["scan"].append(sp[1])
        t["kernel_positions"].append(sp[3])
        return strings, total

    def route_old(t=None, encode=True):
        ev = Events()
        ev.mark()
        bits = (ops.paste_masks(probs, boxes, (h, w))[:, 0] > 0.5).to(torch.uint8)
        ev.mark()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = bits.cpu().numpy()
        copy_ms = (time.perf_counter() - t0) * 1e3
        strings = None
        if encode:
            t0 = time.perf_counter()
            strings = M.counts_to_bytes(host_encode(host))
            if t is not None:
                t["old_host_encode"].append((time.perf_counter() - t0) * 1e3)
        if t is not None:
            t["old_paste_threshold"].append(ev.spans()[0])
            t["old_copy"].append(copy_ms)
        return strings

    def peak_of(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    # ground-truth masks for (iii)
    batch = make_batch(a.gts, h, w)
    sizes = [(h, w)] * a.gts
    lay, tables = ops.pack_poly_masks(batch, sizes)
    flat = ops.mask_flat(lay, dev)
    ops.launch_poly_masks(lay, tables, dev, flat)
    n = len(lay.obj_off)
    hw_host = np.ascontiguousarray(lay.obj_hw, dtype=np.int32)
    cell_off = np.zeros(n + 1, np.int64)
    np.cumsum([int(lib.seam_rle_encode_ws_bytes(int(hh), int(ww))) // 4 for hh, ww in hw_host], out=cell_off[1:])
    gcells = int(cell_off[-1])
    d_hw, d_off, d_cell = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (hw_host, lay.obj_off, cell_off))
    gws = torch.empty((gcells,), dtype=torch.int32, device=dev)
    gct = torch.empty((gcells,), dtype=torch.int32, device=dev)

    def dense_kernels():
        _native.check(lib.seam_rle_encode_masks_u8(flat.data_ptr(), flat.numel(), hw_host.ctypes.data, d_hw.data_ptr(), d_off.data_ptr(),
                                                   d_cell.data_ptr(), gws.data_ptr(), 4 * gcells, gct.data_ptr(), n, stream), "dense")

    # correctness first
    new = [r["counts"] for r in route_new()]
    steps, total = route_new_steps({k: [] for k in ("copy_totals", "copy_positions", "host_diff", "host_strings", "kernels_values_count",
                                                    "scan", "kernel_positions")})
    old = route_old()
    same = new == steps == old
    gt_counts = ops.rle_encode(flat, lay)
    gt_host = host_encode(flat.cpu().numpy().reshape(n, h, w))
    same_gt = all(np.array_equal(x, y) for x, y in zip(gt_counts, gt_host))

    for _ in range(a.warmup):
        route_new()
        route_old()
        dense_kernels()
        flat.clone()
    torch.cuda.synchronize()
    t = {k: [] for k in ("new_e2e", "old_e2e", "old_bound", "copy_totals", "copy_positions", "host_diff", "host_strings",
                         "kernels_values_count", "scan", "kernel_positions", "old_paste_threshold", "old_copy", "old_host_encode",
                         "dense_kernels", "dense_copy", "dense_e2e")}
    for _ in range(a.reps):
        t0 = time.perf_counter()
        route_new()
        t["new_e2e"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        route_old(t)
        t["old_e2e"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        route_old(encode=False)
        t["old_bound"].append((time.perf_counter() - t0) * 1e3)
        route_new_steps(t)
        ev = Events()
        ev.mark()
        dense_kernels()
        ev.mark()
        keep = flat.clone()
        ev.mark()
        torch.cuda.synchronize()
        del keep
        sp = ev.spans()
        t["dense_kernels"].append(sp[0])
        t["dense_copy"].append(sp[1])
        t0 = time.perf_counter()
        ops.rle_encode(flat, lay)
        t["dense_e2e"].append((time.perf_counter() - t0) * 1e3)
    peak_new, peak_old, peak_dense = peak_of(route_new), peak_of(lambda: route_old(encode=False)), peak_of(lambda: ops.rle_encode(flat, lay))
    med = statistics.median
    gb = flat.numel() / 1e9
    lines = [
        "command: rle_encode_bench.py" + "".join(f" {x}" for x in sys.argv[1:]),
        f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP {torch.version.hip}",
        f"one image {h} x {w}, {d} detections, {total} run boundaries in all ({sum(len(s) for s in new)} characters of RLE); "
        f"{a.warmup} warm-up + {a.reps} timed calls of each route, alternating",
        f"bytes, counted from the shapes: pasted fp32 masks {4 * d * h * w}, thresholded bytes copied by (ii) {d * h * w}, "
        f"workspace + counts + scan of (i) {16 * cells}, positions copied by (i) {4 * total}",
        f"all three routes write the same strings: {same}; dense encoder equals the host diff on the ground-truth masks: {same_gt}",
        line("(i)  encode_detections, end to end (host clock, ends in host data)", t["new_e2e"]),
        line("       value + count kernels, with the two clears (events)", t["kernels_values_count"]),
        line("       prefix sum + gather of the totals (events)", t["scan"]),
        line("       positions kernel (events)", t["kernel_positions"]),
        line("       copy of the totals to the host (host clock)", t["copy_totals"]),
        line("       copy of the positions to the host (host clock)", t["copy_positions"]),
        line("       host diff (host clock)", t["host_diff"]),
        line("       host compressed strings, counts_to_bytes (host clock)", t["host_strings"]),
        line("(ii) paste + threshold + copy + host encode, end to end", t["old_e2e"]),
        line("       paste + threshold (events)", t["old_paste_threshold"]),
        line("       copy of the uint8 [D,H,W] bytes to the host (host clock)", t["old_copy"]),
        line("       host encode + strings: this project's NumPy, NOT pycocotools", t["old_host_encode"]),
        line("(ii) lower bound: paste + threshold + copy alone, end to end", t["old_bound"]),
        f"ratio of medians, (ii) / (i): {med(t['old_e2e']) / med(t['new_e2e']):.1f}x; (ii) lower bound / (i): "
        f"{med(t['old_bound']) / med(t['new_e2e']):.1f}x",
        f"allocator peak above the inputs: (i) {peak_new} bytes, (ii) lower bound {peak_old} bytes",
        f"(iii) dense encoder, {n} ground-truth masks of {a.gts} images, {flat.numel()} bytes:",
        line("       value + count kernels, with the two clears (events)", t["dense_kernels"]),
        line("       plain device copy of the same bytes, flat.clone() (events)", t["dense_copy"]),
        line("       ops.rle_encode end to end (host clock, ends in host data)", t["dense_e2e"]),
        f"       achieved over the mask bytes: encoder kernels {gb / (med(t['dense_kernels']) * 1e-3):.0f} GB/s, copy (read + write "
        f"counted once) {gb / (med(t['dense_copy']) * 1e-3):.0f} GB/s; allocator peak of ops.rle_encode {peak_dense} bytes",
    ]
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not (same and same_gt):
        sys.exit("the routes disagree")


if __name__ == "__main__":
    main()
