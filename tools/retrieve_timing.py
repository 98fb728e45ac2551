#!/usr/bin/env python3
"""Time of the tracklet-linking stage of ``retrieval.retrieve`` (GPU box; HIP events), on self-similarity blocks that are already
on the device, as ``ops.pair_scores_blockdiag`` leaves them:

  (a) host    the evaluator's route: the blocks copied to the host, ``evaluator.build_tracklets_batch`` (native host helper), the
              membership (members, lengths, counts) uploaded again -- a device -> host -> device round trip
  (b) device  ``ops.build_tracklets`` (``seam_build_tracklets_f32``, one block per clip), nothing leaves the stream

at two sizes: ``eval`` = 64 clips of 10 frames with 1 to 3 detections each (what an evaluator pass or a batch of short clips
looks like) and ``large`` = one clip of 1000 detections (100 frames of 10).  Descriptors are seeded: a few garment centres plus
noise, so that tracklets link across frames.  Both routes are checked to give the same tracklets before anything is timed.  The
routes alternate in one process -- a, b, a, b -- so the repeats show the run-to-run spread.  Last, one end-to-end ``retrieve``
(host clock around calls that end in the results' copy) on the 128 x 160 test model with synthetic weights: three clips of
three frames, a bank of three products.
Usage: python tools/retrieve_timing.py [--reps N] [out.txt]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import seam_match_rcnn_amd.synth as synth  # noqa: E402
from seam_match_rcnn_amd import evaluator as EV  # noqa: E402
from seam_match_rcnn_amd import ops, retrieval  # noqa: E402

dev = torch.device("cuda:0")
THR = 0.3


def timeit(fn, reps, warm=3):
    """mean ms of one call: HIP events around `reps` calls after `warm` warm-up calls"""
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


def case(seed, frames_per_clip, dets_per_frame, n_clips, centres=6):
    """seeded clips -> (blocks on the device, seg, imgs, scores, device copies)"""
    rng = np.random.default_rng(seed)
    cen = rng.standard_normal((centres, 256))
    imgs, sizes = [], []
    for _ in range(n_clips):
        im = np.concatenate([[f] * int(rng.integers(dets_per_frame[0], dets_per_frame[1] + 1)) for f in range(frames_per_clip)])
        imgs.append(im)
        sizes.append(len(im))
    seg = np.concatenate([[0], np.cumsum(sizes)])
    rows = int(seg[-1])
    x = (cen[rng.integers(0, centres, rows)] + 0.2 * rng.standard_normal((rows, 256))).astype(np.float32)
    w = (rng.standard_normal((2, 256)) * 0.05).astype(np.float32)
    w[1] = -np.abs(w[1])
    b = np.array([-1.0, 1.0], np.float32)
    imgs = np.concatenate(imgs)
    scores = rng.uniform(0.05, 1.0, rows).astype(np.float32)
    d = lambda a: torch.from_numpy(a).to(dev)      # noqa: E731
    blocks = ops.pair_scores_blockdiag(d(x), seg, d(w), d(b))
    return dict(blocks=blocks, seg=seg, imgs=imgs, scores=scores, imgs_d=d(imgs.astype(np.int32)), scores_d=d(scores),
                tables=ops.blockdiag_offsets(seg, dev), max_rows=int(max(sizes)))


def routes(c):
    def host():
        tracks = EV.build_tracklets_batch(c["blocks"].cpu().numpy(), c["seg"], c["imgs"], c["scores"], THR)
        members = np.asarray([m for tr in tracks for t in tr for m in t], dtype=np.int32)
        lens = np.asarray([len(t) for tr in tracks for t in tr], dtype=np.int32)
        ntr = np.asarray([len(tr) for tr in tracks], dtype=np.int32)
        return tracks, [torch.from_numpy(a).to(dev) for a in (members, lens, ntr)]

    def device():
        seg_d, off_d = c["tables"]
        return ops.build_tracklets(c["blocks"], off_d, seg_d, c["imgs_d"], c["scores_d"], THR, max_rows=c["max_rows"])

    return host, device


def lists(out, seg):
    members, lens, ntr, _ = (t.cpu().numpy() for t in out)
    res = []
    for s in range(len(seg) - 1):
        o, tr, mo = int(seg[s]), [], 0
        for k in range(int(ntr[s])):
            tr.append(members[o + mo:o + mo + int(lens[o + k])].tolist())
            mo += int(lens[o + k])
        res.append(tr)
    return res


def test_model():
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.video_matchrcnn_state(5).items()}
    m = videomatchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.transform.min_size, m.transform.max_size = 128, 160
    ims = [[torch.from_numpy(synth.frames(50 + 4 * p + i, 1, 128, 160)[0]) for i in range(4)] for p in range(3)]
    return m, [i[0] for i in ims], [i[1:] for i in ims]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
    if "--reps" in sys.argv:
        args = [a for a in args if a != str(reps)]
    lines = [f"tracklet linking on device-resident self-similarity blocks, threshold {THR}; ms per call (HIP events, 3 warm-up + {reps} "
             f"timed), routes alternating in one process; cap seam_build_tracklets_max_rows() = {ops.build_tracklets_max_rows()}"]
    for name, c in (("eval ", case(1, 10, (1, 3), 64)), ("large", case(2, 100, (10, 10), 1))):
        host, device = routes(c)
        tracks = host()[0]
        assert lists(device(), c["seg"]) == tracks, "the two routes disagree"
        n_tr = sum(len(tr) for tr in tracks)
        res = {k: timeit(fn, reps) for k, fn in (("a1", host), ("b1", device), ("a2", host), ("b2", device))}
        a, b = 0.5 * (res["a1"] + res["a2"]), 0.5 * (res["b1"] + res["b2"])
        spread = max(abs(res["a1"] - res["a2"]), abs(res["b1"] - res["b2"]))
        rows = int(c["seg"][-1])
        lines += [
            f"{name}  {len(c['seg']) - 1} clip(s), {rows} detections, largest clip {c['max_rows']}, {n_tr} tracklets, "
            f"{c['blocks'].numel() * 4 / 1e6:.2f} MB of blocks",
            f"{name}  (a) host    blocks -> host, build_tracklets_batch, membership -> device   {res['a1']:8.3f}   again {res['a2']:8.3f}",
            f"{name}  (b) device  ops.build_tracklets                                           {res['b1']:8.3f}   again {res['b2']:8.3f}",
            f"{name}  spread {spread:.3f} ms; (a) - (b) = {a - b:.3f} ms = {(a - b) / max(spread, 1e-9):.1f} x the spread; (b) / (a) = {b / a:.3f}: "
            + ("(b) is ahead by more than three times the spread" if a - b > 3 * spread
               else "(b) is NOT ahead by more than three times the spread"),
            f"{name}  (b) over the largest clip's serial chain: {b * 1e3 / c['max_rows']:.2f} us per detection joined, launch included (clips run "
            f"in parallel, one block each; inside a block every detection is one seed or one link -- one block-wide selection and one "
            f"barrier each -- plus one selection per tracklet closed)",
        ]
    m, shop, clips = test_model()
    bank = retrieval.build_bank(m, shop)
    for strategy in retrieval.STRATEGIES:
        out = retrieval.retrieve(m, clips, bank, k=3, strategy=strategy)
        for _ in range(2):
            retrieval.retrieve(m, clips, bank, k=3, strategy=strategy)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = 10
        for _ in range(n):
            retrieval.retrieve(m, clips, bank, k=3, strategy=strategy)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / n * 1e3
        lines.append(f"retrieve  end to end, {strategy}: 3 clips x 3 frames 128 x 160 (synthetic weights), bank of {len(bank)}, "
                     f"{sum(len(tm.frames) for c in out for tm in c)} detections in {sum(len(c) for c in out)} tracklets: {ms:.2f} ms per call "
                     f"(host clock, 2 warm-up + {n} timed; the three detector forwards included)")
    print("\n".join(lines))
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
