"""The input stage of a phase-1 training step, timed on the device: the route the loop took until now against
``input_pipeline.prepare_batch``, on the same box, alternating.

Workload: 8 synthetic uint8 images around 800 x 1200 of differing sizes, 5 polygon objects each, every other image flipped; the
model's default transform (min_size 800, max_size 1333).

  parent   host ToTensor (bytes / 255, CHW) + host flip + ``.to(device)`` of the float images + ``targets_to_device`` (masks at
           original size on the device) + device flip of the flipped images' masks + ``model.transform`` (one launch per image:
           the sizes differ) + ``resize_masks_nearest``
  new      ``prepare_batch``: pinned staging of bytes and tables, one copy, one preprocess launch, one mask launch sequence

Each route is timed end to end with a host clock around work that ends in a device synchronise (the stage has host work in it),
after warm-up, the two routes alternating.  The new route is then split: host packing (host clock), the copy (device events) and
the kernels (device events around launches on buffers that are already on the device).  Bytes over the bus are counted from the
shapes.  The results of the two routes are compared with ``torch.equal`` at the timed size.

    python tools/train_input_timing.py --out profiles/train_input.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE_TBS = 6.29          # the device-to-device copy rate measured for SURVEY.md


def make_batch(n=8, objects=5, seed=0):
    rng = np.random.RandomState(seed)
    images, targets = [], []
    for i in range(n):
        h, w = 800 + int(rng.randint(-40, 41)), 1200 + int(rng.randint(-60, 61))
        images.append(torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)))
        segm, boxes = [], []
        for _ in range(objects):
            cx, cy = rng.uniform(0.2 * w, 0.8 * w), rng.uniform(0.2 * h, 0.8 * h)
            ang = np.sort(rng.uniform(0, 2 * np.pi, 24))
            rad = rng.uniform(60, 180, 24)
            xs, ys = np.clip(cx + rad * np.cos(ang), 0, w - 1), np.clip(cy + rad * np.sin(ang), 0, h - 1)
            segm.append([np.stack([xs, ys], 1).reshape(-1).round(2).tolist()])
            boxes.append([xs.min(), ys.min(), xs.max(), ys.max()])
        targets.append(dict(boxes=torch.tensor(boxes, dtype=torch.float32), labels=torch.randint(1, 14, (objects,)),
                            segmentation=segm, size=(h, w), hflip=bool(i % 2)))
    return images, targets


def parent_route(images, targets, device, model):
    from seam_match_rcnn_amd import mask_utils
    from seam_match_rcnn_amd.models.matchrcnn import resize_masks_nearest
    floats = []
    for img, t in zip(images, targets):
        x = img.permute(2, 0, 1).float().div(255)
        floats.append((x.flip(-1) if t["hflip"] else x).contiguous())
    floats = [x.to(device) for x in floats]
    tg = mask_utils.targets_to_device([{k: v for k, v in t.items() if k != "hflip"} for t in targets], device)
    with torch.no_grad():
        x, sizes, orig, padded = model.transform(floats)
    masks = [resize_masks_nearest(t["masks"].flip(-1) if s["hflip"] else t["masks"], z) for t, s, z in zip(tg, targets, sizes)]
    return x, masks


def new_route(images, targets, device, model):
    from seam_match_rcnn_amd.input_pipeline import prepare_batch
    prepared, tg = prepare_batch(images, targets, device, model)
    return prepared.tensor, [t["masks"] for t in tg]


def wall(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def events(fn, reps, inner=1):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return out


def line(name, ms):
    return f"{name:<58s} median {statistics.median(ms):8.3f} ms   min {min(ms):8.3f} ms   max {max(ms):8.3f} ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_input_timing: needs the HIP device (a timing taken elsewhere says nothing)")
    from seam_match_rcnn_amd import mask_utils, ops
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    dev = torch.device("cuda:0")
    model = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14).to(dev).train()
    images, targets = make_batch()
    flips = [t["hflip"] for t in targets]
    lines = ["command: train_input_timing.py --out FILE",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP {torch.version.hip}"]

    xa, ma = parent_route(images, targets, dev, model)
    xb, mb = new_route(images, targets, dev, model)
    same = torch.equal(xa, xb) and all(torch.equal(a, b) for a, b in zip(ma, mb))
    px = sum(i.shape[0] * i.shape[1] for i in images)
    lay, rle_t, poly_t = mask_utils._pack_annotations([t["segmentation"] for t in targets], [t["size"] for t in targets])
    table_bytes = sum(v.nbytes for v in poly_t.values() if isinstance(v, np.ndarray) and v is not poly_t["sel"])
    dense_bytes = sum(len(t["segmentation"]) * t["size"][0] * t["size"][1] for t in targets)
    lines += [f"{len(images)} images {[tuple(i.shape[:2]) for i in images]}, {len(targets[0]['segmentation'])} polygon objects each, "
              f"flips {[int(f) for f in flips]}; batch {tuple(xb.shape)} fp32 ({'space-to-depth' if xb.shape[-1] == 12 else 'NHWC4'}); "
              f"{args.warmup} warm-up + {args.reps} timed calls of each route, alternating",
              f"the two routes give the same batch and the same masks, bit for bit: {same}",
              f"bytes over the bus, counted from the shapes: images parent {12 * px} (fp32 CHW)  new {3 * px} (uint8 HWC): 4.0x fewer",
              f"    annotation tables (both routes) {table_bytes} + 36 per object; the reference's dense uint8 stacks at original size "
              f"would be {dense_bytes}"]

    for _ in range(args.warmup):
        parent_route(images, targets, dev, model)
        new_route(images, targets, dev, model)
    pa, nw = [], []
    for _ in range(args.reps):                                            # alternating, same box
        pa += wall(lambda: parent_route(images, targets, dev, model), 1)
        nw += wall(lambda: new_route(images, targets, dev, model), 1)
    lines += [line("(a) parent route, end to end (host clock + sync)", pa), line("(b) prepare_batch, end to end (host clock + sync)", nw)]

    def iqr(v):
        q = statistics.quantiles(v, n=4)
        return (q[2] - q[0]) / statistics.median(v)
    spread = max(iqr(pa), iqr(nw))
    ratio = statistics.median(nw) / statistics.median(pa)
    lines.append(f"ratio of medians (b) / (a): {ratio:.3f}; run-to-run spread of this run (interquartile range over median, the larger "
                 f"of the two routes): {spread:.3f}; not slower within that spread: {ratio <= 1.0 + spread}")

    # the new route, split
    tr = model.transform
    from seam_match_rcnn_amd.input_pipeline import prepare_images
    prepared = prepare_images(images, dev, model, flips)
    sizes, (hp, wp), s2d = prepared.sizes, prepared.padded, prepared.s2d

    def host_pack():
        ops.stage_u8_batch(images, sizes, hp, wp, flips, dev)
        mask_utils._pack_annotations([t["segmentation"] for t in targets], [t["size"] for t in targets])
    t_pack = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        host_pack()
        t_pack.append(1e3 * (time.perf_counter() - t0))
    stage, n = ops.stage_u8_batch(images, sizes, hp, wp, flips, dev)
    t_copy = events(lambda: stage.to(dev, non_blocking=True), args.reps)
    flat = stage.to(dev)
    off, dims = flat[:8 * n].view(torch.int64), flat[8 * n:28 * n].view(torch.int32).view(n, 5)
    out = torch.empty_like(xb)
    t_img = events(lambda: ops.preprocess_u8_flat(flat, off, dims, hp, wp, s2d, out=out), args.reps, inner=10)
    t_mask = events(lambda: ops.launch_poly_masks_resized(lay, poly_t, sizes, flips, dev), args.reps)
    moved = 3 * px + out.numel() * 4
    gbs = moved / (statistics.median(t_img) * 1e-3) / 1e9
    lines += ["prepare_batch, split (each part run alone):",
              line("    host packing: staging of bytes + annotation tables (host clock)", t_pack),
              line(f"    one copy of {stage.numel()} pinned bytes to the device (events)", t_copy),
              line("    preprocess_u8_batch kernel, one launch (events, 10 launches per sample)", t_img),
              line("    mask launch sequence incl. its table upload (events)", t_mask),
              f"    the image kernel reads {3 * px} and writes {out.numel() * 4} bytes: {gbs:.0f} GB/s, "
              f"{100 * gbs / (1e3 * COPY_RATE_TBS):.1f} % of the measured copy rate ({COPY_RATE_TBS} TB/s)"]
    if gbs < 0.5 * 1e3 * COPY_RATE_TBS:
        lines.append("    the image kernel loses here: it is far from the copy rate (twelve byte loads and twelve divisions per "
                     "resized pixel); it is not the stage's long pole -- the copy is")

    # the parent route's device part for comparison: per-image launches + index selections
    floats = [(i.permute(2, 0, 1).float().div(255).flip(-1) if f else i.permute(2, 0, 1).float().div(255)).contiguous() for i, f in zip(images, flips)]
    t_host = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        [(i.permute(2, 0, 1).float().div(255).flip(-1) if f else i.permute(2, 0, 1).float().div(255)).contiguous() for i, f in zip(images, flips)]
        t_host.append(1e3 * (time.perf_counter() - t0))
    t_h2d = events(lambda: [x.to(dev) for x in floats], args.reps)
    dfl = [x.to(dev) for x in floats]
    with torch.no_grad():
        t_tr = events(lambda: tr(dfl), args.reps)
    lines += ["parent route, split (each part run alone):",
              line("    host ToTensor + flip (host clock)", t_host),
              line("    copies of the float images, pageable memory (events)", t_h2d),
              line("    model.transform, one launch per image (events)", t_tr)]
    parts = statistics.median(t_host) + statistics.median(t_h2d) + statistics.median(t_tr)
    if parts > statistics.median(pa):
        lines.append(f"    UNRELIABLE split: these parts sum to {parts:.3f} ms, more than (a)'s median -- the host part ran alone, later, and "
                     "its time varies by the factor its min and max show; compare the routes by (a) and (b) only")
    text ="\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
