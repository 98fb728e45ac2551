"""The input stage of a phase-3 (MovingFashion) batch, timed on the device: the per-frame route of the parent of the fused kernel
against ``input_pipeline.prepare_batch`` on a lazy batch, on the same box, alternating.

Workload: a batch of the reference's shape at the size this tool can hold in one process, 2 products x (1 shop image + 10 decoded
frames of 1080 x 1920), generated from a seed (nothing here reads a video: decode stays on the host on both routes and is not
timed); the model's default transform (min_size 800, max_size 1333).

  per frame   what a caller could do before ``seam_frames_prepare_batch_u8`` existed: every image uploaded on its own, every frame
              through ``frames.prepare_frame`` (what ``frames.prepare_clip`` looped over: one noise launch, two coefficient launches,
              two resampling passes, one workspace and two image allocations per frame), the list through ``model.transform`` (one
              preprocess launch per image).  Written out here, since ``prepare_clip`` now takes the batched launch itself.
  fused       ``prepare_batch(images, targets, device, model, masks="none")`` with the targets of a lazy ``MovingFashionDataset``:
              one pinned copy, the frames launch, the preprocess launch.

Equal seeds on both routes; the prepared uint8 images must be equal byte for byte and the batch tensor equal to
``prepare_images`` of the per-frame images, or the tool stops.  The device part (the frame work alone, images already on the
device) is timed with device events, the whole stage with a host clock around work that ends in a synchronise.  Launches, copies,
bytes over the bus and the intermediate traffic are counted from the shapes and the launchers, not measured.

    python tools/mf_input_timing.py --out profiles/mf_input.txt
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

PRODUCTS, FRAMES_PER_PRODUCT = 2, 10
FRAME_HW, SHOP_HW = (1080, 1920), (800, 600)
TILE = 64                      # FT of csrc/seam_frames.hip


def make_batch(seed):
    """(images, targets) as a lazy MovingFashionDataset hands them over: RGB shop bytes, full-resolution BGR frames."""
    rng = np.random.RandomState(seed)

    def picture(h, w):          # smooth content plus texture
        base = rng.randint(0, 256, (h // 8 + 1, w // 8 + 1, 3)).astype(np.uint8).repeat(8, 0).repeat(8, 1)[:h, :w]
        return torch.from_numpy(base + rng.randint(0, 4, (h, w, 3)).astype(np.uint8))
    images, targets = [], []
    for p in range(PRODUCTS):
        images.append(picture(*SHOP_HW))
        targets.append({"frame_prep": 0, "frame_sigma": 0.0, "boxes": torch.tensor([[0.0, 0.0, SHOP_HW[1], SHOP_HW[0]]]), "tag": 1, "i": p})
        for k in range(FRAMES_PER_PRODUCT):
            images.append(picture(*FRAME_HW))
            targets.append({"frame_prep": 2, "frame_sigma": 0.25 if rng.rand() > 0.75 else 0.05, "frame_seed": int(rng.randint(0, 2 ** 31)),
                            "boxes": torch.tensor([[0.0, 0.0, FRAME_HW[1] // 2, FRAME_HW[0] // 2]]), "tag": 0, "i": p})
    return images, targets


def per_frame_images(images, targets, dev):
    from seam_match_rcnn_amd import frames
    out = []
    for img, t in zip(images, targets):
        img = img.to(dev)                                      # one upload per image
        out.append(frames.prepare_frame(img, True, t["frame_sigma"], t["frame_seed"]) if t["frame_prep"] == 2 else img)
    return out


def per_frame_route(images, targets, dev, model):
    with torch.no_grad():
        return model.transform(per_frame_images(images, targets, dev))[0]


def fused_route(images, targets, dev, model):
    from seam_match_rcnn_amd.input_pipeline import prepare_batch
    return prepare_batch(images, targets, dev, model, masks="none")[0].tensor


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def line(name, ms):
    return f"{name:<78s} median {statistics.median(ms):9.3f} ms   min {min(ms):9.3f} ms   max {max(ms):9.3f} ms"


def iqr(v):
    q = statistics.quantiles(v, n=4)
    return (q[2] - q[0]) / statistics.median(v)


def window(in_size, first, count):
    """Input samples that output samples [first, first + count) of a halved axis read (Pillow's bounds: csrc/seam_frames.hip)."""
    out = in_size // 2
    scale = in_size / out
    support = 2.0 * scale
    lo = max(int((first + 0.5) * scale - support + 0.5), 0)
    hi = min(int((first + count - 0.5) * scale + support + 0.5), in_size)
    return hi - lo


def draws_made(h, w):
    """Noise draws of the fused kernel for one frame: every tile draws its whole input window, halo included."""
    oh, ow = h // 2, w // 2
    rows = sum(window(h, y, min(TILE, oh - y)) for y in range(0, oh, TILE))
    cols = sum(window(w, x, min(TILE, ow - x)) for x in range(0, ow, TILE))
    return 3 * rows * cols


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mf_input_timing: needs the HIP device (a timing taken elsewhere says nothing)")
    from seam_match_rcnn_amd import frames, ops
    from seam_match_rcnn_amd.input_pipeline import prepare_images
    from seam_match_rcnn_amd.models import detection as det

    class Model:
        transform = det.GeneralizedRCNNTransform()

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    model = Model()
    images, targets = make_batch(0)
    n = len(images)
    frame_ids = [k for k, t in enumerate(targets) if t["frame_prep"] == 2]
    lines = ["command: mf_input_timing.py --out FILE",
             f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; HIP {torch.version.hip}",
             f"{n} images: {PRODUCTS} products x (1 shop image {SHOP_HW} RGB + {FRAMES_PER_PRODUCT} frames {FRAME_HW} BGR), sigmas "
             f"{sorted({t['frame_sigma'] for t in targets if t['frame_prep'] == 2})}; {args.warmup} warm-up + {args.reps} timed batches of "
             f"each route, alternating, one process"]

    # ---- equal outputs first
    a_imgs = per_frame_images(images, targets, dev)
    b_imgs, _ = frames.prepare_frames(images, targets, dev)
    assert all(torch.equal(a, b) for a, b in zip(a_imgs, b_imgs)), "the fused launch and the per-frame route give different bytes"
    xb = fused_route(images, targets, dev, model)
    assert torch.equal(xb, prepare_images(a_imgs, dev, model).tensor), "prepare_batch differs from prepare_images of the per-frame images"
    lines.append(f"equal outputs: the {n} prepared uint8 images are equal byte for byte on both routes, and the fused route's batch "
                 f"{tuple(xb.shape)} fp32 equals prepare_images of the per-frame images bit for bit (asserted before timing)")

    # ---- the whole stage, host clock + synchronise
    for _ in range(args.warmup):
        per_frame_route(images, targets, dev, model)
        fused_route(images, targets, dev, model)
    wa, wb = [], []
    for _ in range(args.reps):
        wa.append(wall(lambda: per_frame_route(images, targets, dev, model)))
        wb.append(wall(lambda: fused_route(images, targets, dev, model)))
    r_wall, s_wall = statistics.median(wb) / statistics.median(wa), max(iqr(wa), iqr(wb))
    lines += ["the whole stage (host images in, the model's batch tensor out; host clock around a synchronise):",
              line("    (a) per frame: upload + prepare_frame per frame + the list through model.transform", wa),
              line("    (b) fused: prepare_batch (one pinned copy, frames launch, preprocess launch)", wb),
              f"    ratio of medians (b) / (a): {r_wall:.3f}; run-to-run spread (interquartile range over median, the larger of the two "
              f"routes): {s_wall:.3f}; the fused route is ahead beyond that spread: {r_wall < 1.0 - s_wall}"]

    # ---- the device part: the frame work alone, images on the device already, device events
    on_dev = [i.to(dev) for i in images]
    modes, sigmas, seeds = frames.frame_args(targets)
    st = ops.stage_frames("mf_input_timing", on_dev, modes, sigmas, seeds, dev)

    def a_device():
        for k in frame_ids:
            frames.prepare_frame(on_dev[k], True, sigmas[k], seeds[k])
    for _ in range(args.warmup):
        a_device()
        ops.launch_frames(st)
    da, db = [], []
    for _ in range(args.reps):
        da.append(events(a_device))
        db.append(events(lambda: ops.launch_frames(st)))
    r_dev, s_dev = statistics.median(db) / statistics.median(da), max(iqr(da), iqr(db))
    ahead = r_dev < 1.0 - s_dev
    lines += ["the device part (the frame work of the batch alone, images on the device already; device events around the launches):",
              line(f"    (a) per frame: {len(frame_ids)} x (noise, 2 coefficient, 2 resampling launches; 3 allocations)", da),
              line("    (b) fused: one seam_frames_prepare_batch_u8 launch (one allocation)", db),
              f"    ratio of medians (b) / (a): {r_dev:.3f}; run-to-run spread: {s_dev:.3f}; the fused kernel is ahead beyond that "
              f"spread: {ahead}"]

    # ---- what binds the fused launch: the same launch with the draws read from memory, and with no noise at all
    counts = [images[k].numel() if modes[k] == 2 else 0 for k in range(n)]
    given = torch.randn(sum(counts), dtype=torch.float64, device=dev)
    given_off = torch.tensor([sum(counts[:k]) for k in range(n)], dtype=torch.int64, device=dev)
    out = torch.empty(st.out_bytes, dtype=torch.uint8, device=dev)
    quiet = torch.zeros_like(st.sigma)

    def flat(sig, dr=None, do=None):
        ops.frames_prepare_flat(st.dev, st.in_off, st.dims, sig, st.seed, out, st.out_off, st.max_h, st.max_w, dr, do)
    for _ in range(args.warmup):
        flat(st.sigma, given, given_off)
        flat(quiet)
    dgen = [events(lambda: flat(st.sigma)) for _ in range(args.reps)]
    dgiv = [events(lambda: flat(st.sigma, given, given_off)) for _ in range(args.reps)]
    dqui = [events(lambda: flat(quiet)) for _ in range(args.reps)]
    dcat = [events(lambda: ops.frames_prepare_batch(on_dev, modes, sigmas, seeds)) for _ in range(args.reps)]
    m_gen, m_giv, m_qui = statistics.median(dgen), statistics.median(dgiv), statistics.median(dqui)
    lines += ["what binds the fused launch (the same staged batch and output buffer, device events):",
              line("    the generator's draws (as above, output preallocated)", dgen),
              line("    the draws given: no hashes, log, sqrt or cos; 8 more bytes read per element and halo element", dgiv),
              line("    sigma 0 and no draws: flip + the two resampling passes alone, no float64 arithmetic per element", dqui),
              f"    the generator accounts for {m_gen - m_giv:.3f} ms of the launch's {m_gen:.3f} ({100 * (m_gen - m_giv) / m_gen:.0f} %), the "
              f"float64 byte expression and the draws' loads for {m_giv - m_qui:.3f} ms, and what is left with no noise at all -- byte "
              f"loads, the index divisions, the two passes through LDS, the byte stores, at the three blocks per CU that LDS allows -- "
              f"for {m_qui:.3f} ms ({100 * m_qui / m_gen:.0f} %): "
              + ("the generator's arithmetic is the larger part" if m_gen - m_giv > 0.5 * m_gen else
                 "the generator's arithmetic is NOT the larger part"),
              line(f"    ops.frames_prepare_batch on the {n} device images: + table upload and the torch.cat that joins them", dcat),
              "    the device part above starts from a staged buffer: for images that lie on the device already (frames.prepare_clip) "
              "that join, a read and a write of every input byte, comes on top, as the last line shows"]

    # ---- the rest of the stage, split: what surrounds the frame work on either route
    total = sum(i.numel() for i in images)
    pinned = torch.empty(total, dtype=torch.uint8).pin_memory()
    up_a = [wall(lambda: [i.to(dev) for i in images]) for _ in range(args.reps)]
    up_b = [wall(lambda: ops.stage_frames("mf_input_timing", images, modes, sigmas, seeds, dev)) for _ in range(args.reps)]
    copy_b = [events(lambda: pinned.to(dev, non_blocking=True)) for _ in range(args.reps)]
    pre_a = [events(lambda: model.transform(a_imgs)) for _ in range(args.reps)]
    lines += ["the rest of the stage, split (each part run alone):",
              line(f"    (a) the {n} uploads of pageable host tensors, one per image (host clock + sync)", up_a),
              line("    (b) packing into the pinned staging buffer + the one copy (host clock + sync)", up_b),
              line(f"    (b) the one copy of {total} pinned bytes alone (events)", copy_b),
              line(f"    (a) the list through model.transform: {n} preprocess launches (events)", pre_a),
              f"    packing on the host is (b)'s staging minus its copy, about {statistics.median(up_b) - statistics.median(copy_b):.3f} ms: the "
              f"bytes are written twice on the host side of the fused route (into the staging buffer, then over the bus), and its kernels "
              f"wait for the whole copy, where the per-frame route's kernels run under the next image's upload"]

    # ---- counted from the shapes and the launchers
    fh, fw = FRAME_HW
    f_in = sum(3 * images[k].shape[0] * images[k].shape[1] for k in frame_ids)
    f_half_w = sum(3 * images[k].shape[0] * (images[k].shape[1] // 2) for k in frame_ids)
    f_out = sum(3 * (images[k].shape[0] // 2) * (images[k].shape[1] // 2) for k in frame_ids)
    bus = sum(i.numel() for i in images)
    made = len(frame_ids) * draws_made(fh, fw)
    ms_b = statistics.median(db)
    lines += ["counted from the shapes and the launchers (not measured):",
              f"    launches per batch: per frame {5 * len(frame_ids)} frame launches + {n} preprocess launches = {5 * len(frame_ids) + n}; "
              f"fused 1 + 1 = 2",
              f"    host-to-device copies per batch: per frame {n} (pageable); fused 1 (pinned); bytes over the bus: {bus} image bytes "
              f"on both routes, + {64 * n} table bytes on the fused one",
              f"    intermediate traffic of the frame work: per frame a full-resolution RGB image ({f_in} bytes) and a half-width image "
              f"({f_half_w} bytes) are written and read back, {2 * (f_in + f_half_w)} bytes, besides {f_in} read and {f_out} written; "
              f"fused reads the input windows and writes {f_out} bytes, no intermediate reaches memory",
              f"    noise draws: per frame {f_in} (one per element); fused {made} = {made / f_in:.3f}x (a {TILE} x {TILE} tile draws its "
              f"{window(fw, TILE, TILE)} x {window(fh, TILE, TILE)} input window, halo included)",
              f"    the fused launch makes {made / (ms_b * 1e-3) / 1e9:.1f} G draws/s; it reads {f_in} and writes {f_out} bytes in "
              f"{ms_b:.3f} ms = {(f_in + f_out) / (ms_b * 1e-3) / 1e9:.1f} GB/s, far below the memory system's rate"]
    if not ahead:
        lines.append("the fused kernel's device time is NOT below the per-frame route's beyond the spread: both make one float64 draw "
                     "(two 64-bit hashes, log, sqrt, cos) per element, the fused one more of them for its halos, and that arithmetic, "
                     "not the intermediate traffic the fusion removes, is the suspected bound (see the split above)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
