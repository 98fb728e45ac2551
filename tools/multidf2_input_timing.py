"""The input stage of a phase-2 (Multi-DeepFashion2) batch, timed on the device: the eager dataset + the eager route against the
lazy dataset + ``input_pipeline.prepare_batch``, on the same box, alternating.

Workload: a batch of the reference's shape, 2 products x 11 images (one shop image + 10 street images each) of about 600 x 900,
as synthetic PNG files written to a temporary directory from a seed (nothing here reads a real dataset), read back through
``datasets.MultiDF2Dataset.MultiDeepFashion2Dataset(noise=True)``; the model's default transform (min_size 800, max_size 1333).

  eager    ``MultiDeepFashion2Dataset(lazy=False)`` + ``ToTensor()``: per image one ``np.random.randn(h, w, 3)`` and, for the one image
           in four that is noisy, five float64 passes on the host; then ``.to(device)`` of the float images and ``model.transform``.
           This dataset is this project's restatement of the reference's host arithmetic (``MultiDF2Dataset.py:157-167``), not the
           reference itself, which needs torchvision and pycocotools.  (Its dense masks are stubbed out here: phase 2 reads boxes.)
  lazy     ``MultiDeepFashion2Dataset(lazy=True)`` + ``prepare_batch(..., masks="none")``: the decoded bytes, one pinned copy, the
           noise launch (``seam_noise_u8_batch``) and the preprocess launch.

Both include the PNG decode, which is the same work on both routes and is also timed alone.  Each route is timed end to end with a
host clock around work that ends in a device synchronise, after warm-up, the two routes alternating with equal seeds (so both
pick the same images and the same sigmas).  The noise kernel is then timed alone with device events on a staged batch, at the
dataset's mix of sigmas and with every image noisy.  Bytes over the bus are counted from the shapes.

    python tools/multidf2_input_timing.py --out profiles/multidf2_input.txt
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCTS, PER_PRODUCT = 2, 11
COPY_RATE_TBS = 6.29          # the device-to-device copy rate measured for SURVEY.md


def write_dataset(root, seed=0):
    """PRODUCTS products of one shop image and PER_PRODUCT - 1 street images, about 600 x 900, one box each."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    images, annotations, img_id = [], [], 0
    os.makedirs(os.path.join(root, "images"))
    for p in range(PRODUCTS):
        for k in range(PER_PRODUCT):
            img_id += 1
            h, w = 600 + int(rng.randint(-30, 31)), 900 + int(rng.randint(-45, 46))
            # smooth content plus texture: a PNG of pure noise would make the decode slower than any photograph's
            base = rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
            Image.fromarray(base + rng.randint(0, 4, (h, w, 3)).astype(np.uint8)).save(os.path.join(root, "images", f"{img_id}.png"))
            source = "shop" if k == 0 else "user"
            images.append({"id": img_id, "file_name": f"{img_id}.png", "height": h, "width": w, "source": source,
                           "match_desc": {"1": 100 + p}})
            annotations.append({"id": img_id, "image_id": img_id, "category_id": 1, "bbox": [50.0, 40.0, w - 100.0, h - 80.0],
                                "area": float((w - 100) * (h - 80)), "pair_id": 100 + p, "style": 1, "source": source, "iscrowd": 0,
                                "segmentation": [[50.0, 40.0, w - 50.0, 40.0, w - 50.0, h - 40.0, 50.0, h - 40.0]]})
    ann_file = os.path.join(root, "ann.json")
    with open(ann_file, "w") as f:
        json.dump({"images": images, "annotations": annotations, "categories": [{"id": 1, "name": "top"}]}, f)
    return ann_file, os.path.join(root, "images")


def one_batch(dataset, seed):
    """The first batch of a seeded pass, sampled in this process (no workers: the host work is what is measured)."""
    from seam_match_rcnn_amd.datasets.MultiDF2Dataset import get_dataloader
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    return next(iter(get_dataloader(dataset, PRODUCTS * PER_PRODUCT, False, n_products=PRODUCTS)))


def eager_route(dataset, seed, device, model):
    images, targets, _ = one_batch(dataset, seed)
    images = [i.to(device) for i in images]
    with torch.no_grad():
        return model.transform(images)[0], targets


def lazy_route(dataset, seed, device, model):
    from seam_match_rcnn_amd.input_pipeline import prepare_batch
    images, targets, _ = one_batch(dataset, seed)
    prepared, _ = prepare_batch(images, targets, device, model, masks="none")
    return prepared.tensor, targets


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def host(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
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
    return f"{name:<74s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return (q[2] - q[0]) / statistics.median(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multidf2_input_timing: needs the HIP device (a timing taken elsewhere says nothing)")
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.datasets import DF2Dataset
    from seam_match_rcnn_amd.datasets.MultiDF2Dataset import MultiDeepFashion2Dataset
    from seam_match_rcnn_amd.input_pipeline import prepare_images
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    from seam_match_rcnn_amd.transform import ToTensor
    dev = torch.device("cuda:0")
    model = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14).to(dev).eval()
    # the eager form's dense masks are rasterised on the device and phase 2 never reads them: left out of both routes
    DF2Dataset.DeepFashion2Dataset._masks = lambda self, kept, h, w: torch.zeros((len(kept), 1, 1), dtype=torch.uint8)
    lines = ["command: multidf2_input_timing.py --out FILE",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP {torch.version.hip}; "
             f"host threads torch uses: {torch.get_num_threads()}"]
    with tempfile.TemporaryDirectory() as tmp:
        ann_file, root = write_dataset(tmp)
        eager = MultiDeepFashion2Dataset(ann_file, root, ToTensor(), noise=True)
        lazy = MultiDeepFashion2Dataset(ann_file, root, noise=True, lazy=True)

        xa, ta = eager_route(eager, 100, dev, model)
        xb, tb = lazy_route(lazy, 100, dev, model)
        images, targets, _ = one_batch(lazy, 100)
        sig = [t["noise_sigma"] for t in targets]
        px = sum(i.shape[0] * i.shape[1] for i in images)
        same_pick = [t["i"] for t in ta] == [t["i"] for t in tb] and tuple(xa.shape) == tuple(xb.shape)
        clean = [k for k, s in enumerate(sig) if s == 0.0]
        lines += [f"{len(images)} images ({PRODUCTS} products x {PER_PRODUCT}) {sorted({tuple(i.shape[:2]) for i in images})[:3]} ..., "
                  f"{px} pixels; {sum(s > 0 for s in sig)} of them noisy (sigma 0.1) in the batch of seed 100; batch {tuple(xb.shape)} fp32; "
                  f"{args.warmup} warm-up + {args.reps} timed batches of each route, alternating, seeds 100, 101, ...",
                  "the eager dataset is this project's restatement of the reference's host arithmetic, not the reference itself",
                  f"equal seeds pick the same products and the same shapes on both routes: {same_pick}; the noise values differ by "
                  f"design (NumPy's generator on the host, the counter-based one on the device); the images without noise give the "
                  f"same batch rows on both routes, bit for bit: {all(torch.equal(xa[k], xb[k]) for k in clean)} ({len(clean)} rows)",
                  f"bytes over the bus, counted from the shapes: eager {12 * px} (fp32 CHW, one copy per image)  lazy {3 * px + 44 * len(images)} "
                  f"(uint8 HWC + tables, one copy): {12 * px / (3 * px + 44 * len(images)):.2f}x fewer"]

        for k in range(args.warmup):
            eager_route(eager, 50 + k, dev, model)
            lazy_route(lazy, 50 + k, dev, model)
        ea, la = [], []
        for k in range(args.reps):                                           # alternating, same box, equal seeds
            ea.append(wall(lambda: eager_route(eager, 100 + k, dev, model)))
            la.append(wall(lambda: lazy_route(lazy, 100 + k, dev, model)))
        ratio = statistics.median(la) / statistics.median(ea)
        spread = max(iqr(ea), iqr(la))
        lines += [line("(a) eager dataset + .to(device) + model.transform, end to end (host clock + sync)", ea),
                  line("(b) lazy dataset + prepare_batch, end to end (host clock + sync)", la),
                  f"ratio of medians (b) / (a): {ratio:.3f}; run-to-run spread of this run (interquartile range over median, the larger "
                  f"of the two routes): {spread:.3f}; the device route is ahead beyond that spread: {ratio < 1.0 - spread}"]

        # ---- the host side, split
        plain = MultiDeepFashion2Dataset(ann_file, root, noise=False, lazy=True)
        t_decode = host(lambda: one_batch(plain, 100), args.reps)
        arrays = [i.numpy() for i in images]

        def host_noise(image, sigma):                                         # the eager dataset's lines, one image
            draws = np.random.randn(*image.shape)
            if sigma > 0:
                x = image / 255.0
                x += draws * sigma
                x = x * 255.0
                x = np.clip(x, 0, 255.0)
                return np.asarray(x, dtype=np.uint8)
            return image

        def reference_noise(image, sigma):                                    # every step for every image, as the reference does
            x = image / 255.0
            x += np.random.randn(*image.shape) * sigma
            x = x * 255.0
            x = np.clip(x, 0, 255.0)
            return np.asarray(x, dtype=np.uint8)
        t_draw = [v / len(arrays) for v in host(lambda: [np.random.randn(*a.shape) for a in arrays], args.reps)]
        t_clean = [v / len(arrays) for v in host(lambda: [host_noise(a, 0.0) for a in arrays], args.reps)]
        t_noisy = [v / len(arrays) for v in host(lambda: [host_noise(a, 0.1) for a in arrays], args.reps)]
        t_ref = [v / len(arrays) for v in host(lambda: [reference_noise(a, 0.0) for a in arrays], args.reps)]
        lines += ["the host side, split (each part run alone, one process, no workers):",
                  line(f"    PNG decode + targets of the {len(images)} images, either route (lazy dataset, noise=False)", t_decode),
                  line("    eager noise per image: np.random.randn(h, w, 3) alone", t_draw),
                  line("    eager noise per image, sigma 0 (the draws, arithmetic skipped)", t_clean),
                  line("    eager noise per image, sigma 0.1 (the draws + five float64 passes)", t_noisy),
                  line("    the reference's lines per image, sigma 0 (draws + five passes, nothing skipped)", t_ref)]

        # ---- the device side, split
        flips = [False] * len(images)
        prepared = prepare_images(images, dev, model, flips)
        sizes, (hp, wp), s2d = prepared.sizes, prepared.padded, prepared.s2d
        n = len(images)
        seeds = [int(t.get("noise_seed", 0)) for t in targets]
        t_pack = host(lambda: ops.stage_u8_batch(images, sizes, hp, wp, flips, dev, noise=(sig, seeds)), args.reps)
        stage, _ = ops.stage_u8_batch(images, sizes, hp, wp, flips, dev, noise=(sig, seeds))
        t_copy = events(lambda: stage.to(dev, non_blocking=True), args.reps)
        floats = [i.permute(2, 0, 1).float().div(255).contiguous() for i in images]
        t_copy_f = events(lambda: [x.to(dev) for x in floats], args.reps)

        def kernel_time(sigmas):
            st, _ = ops.stage_u8_batch(images, sizes, hp, wp, flips, dev, noise=(sigmas, list(range(1, n + 1))))
            flat = st.to(dev)
            off, dims = flat[:8 * n].view(torch.int64), flat[8 * n:28 * n].view(torch.int32).view(n, 5)
            at = flat.numel() - 16 * n
            s_t, d_t = flat[at:at + 8 * n].view(torch.float64), flat[at + 8 * n:]
            return events(lambda: ops._launch_noise(flat, off, dims, s_t, d_t), args.reps, inner=5), flat, off, dims
        t_mix, flat, off, dims = kernel_time(sig)
        t_all, flat_all, off_all, dims_all = kernel_time([0.1] * n)
        # the same launch with the draws read from memory: no hashes, log, sqrt or cos, and 8 more bytes read per element
        counts = [3 * i.shape[0] * i.shape[1] for i in images]
        given = torch.randn(sum(counts), dtype=torch.float64, device=dev)
        given_off = torch.tensor([sum(counts[:k]) for k in range(n)], dtype=torch.int64, device=dev)
        at_all = flat_all.numel() - 16 * n
        t_given = events(lambda: ops._launch_noise(flat_all, off_all, dims_all, flat_all[at_all:at_all + 8 * n].view(torch.float64),
                                                   flat_all[at_all + 8 * n:], given, given_off), args.reps, inner=5)
        out = torch.empty_like(xb)
        t_pre = events(lambda: ops.preprocess_u8_flat(flat, off, dims, hp, wp, s2d, out=out), args.reps, inner=5)
        noisy_bytes = 3 * sum(i.shape[0] * i.shape[1] for i, s in zip(images, sig) if s > 0)
        all_bytes = 3 * px
        ms_all = statistics.median(t_all)
        draws_s = all_bytes / (ms_all * 1e-3)
        lines += ["the device side, split (each part run alone):",
                  line("    host packing: bytes + tables into the pinned staging buffer (host clock)", t_pack),
                  line(f"    one copy of {stage.numel()} pinned bytes to the device (events)", t_copy),
                  line(f"    eager route's copies: {n} float images, {12 * px} pageable bytes (events)", t_copy_f),
                  line(f"    seam_noise_u8_batch, the batch's own sigmas: {noisy_bytes} noisy bytes (events, 5 launches)", t_mix),
                  line(f"    seam_noise_u8_batch, every image noisy: {all_bytes} bytes (events, 5 launches)", t_all),
                  line("    the same with the draws given (no generator; 8 more bytes read per element)", t_given),
                  line("    seam_preprocess_u8_batch_f32 on the same buffer (events, 5 launches)", t_pre),
                  f"    every image noisy: {draws_s / 1e9:.1f} G draws/s = {draws_s / 1e9:.1f} GB/s read and as much written "
                  f"({100 * 2 * draws_s / (1e12 * COPY_RATE_TBS):.2f} % of the measured copy rate, {COPY_RATE_TBS} TB/s; at that rate the "
                  f"same bytes would take {1e3 * 2 * all_bytes / (1e12 * COPY_RATE_TBS):.4f} ms)",
                  f"    which side binds it: with the draws given, the byte loads and stores and the four float64 operations of the "
                  f"byte expression remain and the launch takes {statistics.median(t_given) / ms_all:.2f} of the time; "
                  + ("the generator's float64 arithmetic (two 64-bit hashes, log, sqrt, cos per byte) is the larger part: the kernel is "
                     "bound by arithmetic, not by its byte traffic" if statistics.median(t_given) < 0.5 * ms_all else
                     "the byte traffic (one-byte loads and stores) is the larger part: the kernel is bound by its memory side"),
                  f"    host time of the eager noise for the batch, from the per-image medians above: "
                  f"{statistics.median(t_clean) * (n - sum(s > 0 for s in sig)) + statistics.median(t_noisy) * sum(s > 0 for s in sig):.1f} ms; "
                  f"the noise launch that replaces it: {statistics.median(t_mix):.3f} ms"]
        if ratio >= 1.0 - spread:
            lines.append("the device route is NOT ahead end to end beyond the spread: see the split -- the decode, the same on both "
                         "routes, is the stage's long pole")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
