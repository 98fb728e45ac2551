"""Data-parallel retrieval: clip sharding, RCCL all-gather of the product-descriptor bank,
street-sequence vs. bank match + top-k  (BASELINE.json north_star).

The reference has no counterpart for the collective (its "multi-GPU" is N independent
processes, ref train_movingfashion.py:46-50; the gallery is a Python list concatenated with
NumPy on rank 0, ref evaluate_movingfashion.py:45-47,82,92).  Here:

  * clips are independent            -> rank r owns clips  r, r+W, r+2W, ...   (no collective)
  * gallery products are independent -> rank r *computes* descriptors for products
    [lo_r, hi_r) (each shop image goes through the extractor once, somewhere)
  * the only exchange: every query sequence is matched against EVERY product, so the
    descriptor shards are all-gathered into the full bank [G,256] on every rank -- one
    ``all_gather_into_tensor`` (backend "nccl" == RCCL over xGMI), issued on a side stream so
    it overlaps the street-side trunk / NLB work, then the local pairwise + top-k kernels run.

Everything here works on CPU tensors with the gloo backend too (used by the world_size=2
tests for the sharding / gather logic; the match itself always needs the HIP kernels).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous shard [lo,hi) of n items for ``rank``; the first n % world ranks get one extra."""
    q, r = divmod(n, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def clips_for_rank(n_clips: int, rank: int, world: int) -> List[int]:
    """Round-robin clip ownership: r, r+W, r+2W, ..."""
    return list(range(rank, n_clips, world))


def _world(group=None) -> int:
    return dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1


class BankGather:
    """Handle of an in-flight all-gather of the product bank (``wait()`` -> [G,256]).
    ``events`` (when the gather was issued with ``timed=True`` on a HIP stream): (start, end) events recorded on the
    stream the collective runs on, for ``elapsed_us()`` after a synchronisation."""

    def __init__(self, bank: torch.Tensor, g_total: int, work=None, stream=None, pad_rows: int = 0,
                 sizes: Optional[List[int]] = None, events=None):
        self.bank, self.g_total, self.work, self.stream = bank, g_total, work, stream
        self.pad_rows, self.sizes, self.events = pad_rows, sizes, events

    def wait(self) -> torch.Tensor:
        if self.work is not None:
            self.work.wait()
        if self.stream is not None:
            torch.cuda.current_stream().wait_stream(self.stream)
        if self.sizes is not None:      # ragged shards were padded to the largest: compact
            m = max(self.sizes)
            parts = [self.bank[i * m:i * m + s] for i, s in enumerate(self.sizes)]
            return torch.cat(parts, 0)
        return self.bank

    def elapsed_us(self) -> Optional[float]:
        """Device time of the collective (call after the stream was synchronised); None when not timed."""
        if self.events is None:
            return None
        return 1e3 * self.events[0].elapsed_time(self.events[1])


def _gather_into_tensor(group=None, device_type: str = "cuda") -> bool:
    """Which collective form to issue -- decided from the process group's backend CONFIGURATION and the shard's device type
    (both rank-invariant), so that every rank issues the same call (a per-rank try/except could pair
    ``all_gather_into_tensor`` on one rank with ``all_gather`` on another and deadlock): a CUDA shard in a group whose cuda
    backend is RCCL ("nccl", also as part of "cpu:gloo,cuda:nccl" or a group initialised without an explicit backend) gathers
    into one tensor; anything else (gloo, CPU tests) uses the list form."""
    if device_type != "cuda":
        return False
    try:
        cfg = str(dist.get_backend_config(group)).lower()            # e.g. "cuda:nccl" / "cpu:gloo,cuda:nccl" / "cpu:gloo"
    except (AttributeError, RuntimeError, ValueError):
        cfg = str(dist.get_backend(group)).lower()
    parts = dict(p.split(":", 1) for p in cfg.split(",") if ":" in p)
    return parts.get("cuda", cfg) == "nccl" or cfg == "nccl"


def gather_product_bank(local: torch.Tensor, g_total: int, group=None, side_stream=None, timed: bool = False,
                        force: bool = False) -> BankGather:
    """All-gather the per-rank descriptor shards ``local[g_r,256]`` (g_r from ``shard_range``)
    into the full bank, product order preserved.  Asynchronous: returns a ``BankGather``.

    side_stream: optional ``torch.cuda.Stream``; the collective is enqueued there (after the
    producer of ``local`` on the current stream) so compute on the current stream overlaps it.
    timed: bracket the collective with HIP events on the stream it runs on (``BankGather.elapsed_us``).
    force: issue the collective even in a one-rank process group (exercises the N > 1 code path on a single GPU)."""
    world = _world(group)
    if world == 1 and not (force and dist.is_available() and dist.is_initialized()):
        return BankGather(local, g_total)
    rank = dist.get_rank(group)
    sizes = [shard_range(g_total, r, world)[1] - shard_range(g_total, r, world)[0] for r in range(world)]
    assert local.shape[0] == sizes[rank], (local.shape, sizes, rank)
    m = max(sizes)
    ragged = min(sizes) != m
    src = local.contiguous()
    if ragged:
        pad = local.new_zeros((m, local.shape[1]))
        pad[:src.shape[0]] = src
        src = pad
    bank = local.new_empty((world * m, local.shape[1]))
    into = _gather_into_tensor(group, local.device.type)

    def issue():
        if into:
            return dist.all_gather_into_tensor(bank, src, group=group, async_op=True)
        return dist.all_gather(list(bank.view(world, m, -1).unbind(0)), src, group=group, async_op=True)

    if local.is_cuda and side_stream is not None:
        side_stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side_stream):
            ev = None
            if timed:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            work = issue()
            if timed:
                try:
                    work.wait()         # stream-level wait (no host block): orders the end event behind the collective
                    ev[1].record()
                except RuntimeError:    # a backend without stream-level waits: the gather itself is unaffected, only untimed
                    ev = None
        return BankGather(bank, g_total, work, side_stream, sizes=sizes if ragged else None, events=ev)
    return BankGather(bank, g_total, issue(), None, sizes=sizes if ragged else None)


@torch.no_grad()
def match_sequences(aggregator, x3_1b: torch.Tensor, bank: torch.Tensor, k: int = 20):
    """Aggregated street descriptors [S,256] vs the full bank [G,256] with the aggregator's
    pairwise classifier (ref models/match_head.py:161-162), then score + rank
    (ref evaluate_movingfashion.py:263-269).  -> (x5 [S,G,2], idx [S,k] int64, score [S,k]).
    min(k, G) may not exceed the top-k capacity ``seam_rank_topk_max_k()`` (256): ``ops.rank_topk`` raises ValueError above it
    (no clamp; ``ops.rank_of`` gives positions in the full ranking)."""
    from . import ops
    k = ops._topk_k(k, bank.shape[0], "match_sequences")        # refused before the logits are computed
    x5 = aggregator.pair(x3_1b, bank)
    idx, score = ops.rank_topk(x5, k)
    return x5, idx, score


@torch.no_grad()
def match_sequences_topk(aggregator, x3_1b: torch.Tensor, bank: torch.Tensor, k: int = 20):
    """Same ranking as ``match_sequences`` without materialising the full [S,G,2] logits, for large galleries (configs 3/4:
    G = 20 000 / 50 000): ``ops.pair_topk`` -- banks of >= 8192 products go through the MFMA similarity + fused top-k
    (seam_pair_topk_mfma_f32: candidates from the logit-difference GEMM, exact re-scoring, rounding-error proof), smaller ones
    through query chunks of seam_pair_logits_f32 + seam_rank_topk_f32; bit-identical either way.
    -> (idx [S,k] int64, score [S,k]).  min(k, G) may not exceed ``seam_rank_topk_max_k()`` (256): ``ops.pair_topk`` raises
    ValueError above it, whichever implementation would have run."""
    from . import ops
    return ops.pair_topk(x3_1b, bank, aggregator.last.weight, aggregator.last.bias, min(k, bank.shape[0]))


# ---------------------------------------------------------------------------------------------------
# Evaluator-side retrieval on the device in fp32: the closures of
# evaluate_movingfashion.py:94-121 (NumPy fp16, full argsort per query on the CPU) as kernel calls.
@torch.no_grad()
def compute_distances(street: torch.Tensor, shop: torch.Tensor, w: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """``compute_distances`` / ``compute_selfdist`` (pass shop=street): softmax((shop-street)^2 @ w.T + b)[...,1]
    -> [n_street, n_shop]  (ref evaluate_movingfashion.py:102-107,115-121)."""
    from . import ops
    return ops.match_scores(ops.pair_logits(street, shop, w, b))


@torch.no_grad()
def compute_rank_of(street: torch.Tensor, shop: torch.Tensor, w: torch.Tensor, b: torch.Tensor,
                    target: torch.Tensor) -> torch.Tensor:
    """Rank of the true product of each street descriptor: what the evaluator extracts from
    ``compute_ranking(inds)`` with ``(rankings == shop_prod_index).nonzero()`` (ref :94-100,228,268); the
    top-k accuracies only test ``rank < k`` for k in {1,5,10,20} (ref :15,229-231)."""
    from . import ops
    return ops.rank_of(ops.pair_logits(street, shop, w, b), target.to(torch.int64))


# ---------------------------------------------------------------------------------------------------
# Retrieval on an unlabelled video: a product bank from shop images, then detector -> self-similarity -> device tracklet linker ->
# per-tracklet descriptor -> exact top-k against the bank, for every clip of a call ("Retrieval on an unlabelled
# video").  The evaluator follows ONE tracklet per product, chosen by ground-truth boxes; here every tracklet is answered.
STRATEGIES = ("aggr_desc", "avg_desc")


@dataclass
class ProductBank:
    """The gallery ``retrieve`` ranks against: one row per shop image that gave a box."""
    match: torch.Tensor                 # [G,256] match_predictor descriptors (``match_features``) -- ranked by "avg_desc"
    aggr: torch.Tensor                  # [G,256] temporal_aggregator descriptors of the same boxes -- ranked by "aggr_desc"
    boxes: torch.Tensor                 # [G,4] the box each row was taken from (original-image pixels)
    scores: torch.Tensor                # [G] its confidence
    keys: list = field(default_factory=list)        # [G] caller's product keys
    missing: list = field(default_factory=list)     # keys of the images that gave no box at the score threshold

    def __len__(self) -> int:
        return int(self.match.shape[0])

    def to(self, device) -> "ProductBank":
        return ProductBank(self.match.to(device), self.aggr.to(device), self.boxes.to(device), self.scores.to(device),
                           list(self.keys), list(self.missing))

    def save(self, path) -> None:
        """CPU tensors through ``torch.save``."""
        torch.save({"format": 1, "match": self.match.cpu(), "aggr": self.aggr.cpu(), "boxes": self.boxes.cpu(),
                    "scores": self.scores.cpu(), "keys": list(self.keys), "missing": list(self.missing)}, path)

    @staticmethod
    def load(path, device=None) -> "ProductBank":
        d = torch.load(path, map_location="cpu", weights_only=True)
        if d.get("format") != 1:
            raise ValueError(f"ProductBank.load: {path} is not a saved ProductBank")
        bank = ProductBank(d["match"], d["aggr"], d["boxes"], d["scores"], list(d["keys"]), list(d["missing"]))
        return bank if device is None else bank.to(device)

    def extend(self, other: "ProductBank") -> "ProductBank":
        """Append ``other``'s rows (moved to this bank's device), keys and missing keys; returns self."""
        dev = self.match.device
        self.match = torch.cat([self.match, other.match.to(dev)])
        self.aggr = torch.cat([self.aggr, other.aggr.to(dev)])
        self.boxes = torch.cat([self.boxes, other.boxes.to(dev)])
        self.scores = torch.cat([self.scores, other.scores.to(dev)])
        self.keys = list(self.keys) + list(other.keys)
        self.missing = list(self.missing) + list(other.missing)
        return self


@dataclass
class TrackletMatch:
    """One tracklet of a clip and its ranking.  The per-member lists are in ascending frame order."""
    frames: List[int]                   # frame index inside the clip of every member
    detections: List[int]               # index of the member inside its frame's model output
    boxes: torch.Tensor                 # [m,4] (host)
    scores: torch.Tensor                # [m] detection confidences (host)
    product_idx: torch.Tensor           # [k] int64 rows of the bank, best first (host)
    product_keys: list                  # [k] bank.keys of those rows
    match_scores: torch.Tensor          # [k] softmax match score of those rows (host)


def _model_device(model) -> torch.device:
    return next(model.parameters()).device


@torch.no_grad()
def build_bank(model, images, keys=None, device=None, score_threshold: float = 0.0, step: int = 11) -> ProductBank:
    """Shop images -> ``ProductBank``: the model runs over chunks of ``step`` images; of every image the largest-area detection at
    or above ``score_threshold`` is kept (first maximum; the rule of evaluate_movingfashion.py:39-45 that
    ``evaluator.collect_descriptors`` follows, whose shop rows these are), an image without one goes to ``missing``.
    ``keys`` default to the image positions."""
    images = list(images)
    keys = list(range(len(images))) if keys is None else list(keys)
    if len(keys) != len(images):
        raise ValueError("build_bank: one key per image is needed")
    device = _model_device(model) if device is None else torch.device(device)
    agg = model.roi_heads.temporal_aggregator
    one_i, zero_l = torch.ones(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64)
    match, aggr, boxes, scores, kept, missing = [], [], [], [], [], []
    for x in range(0, len(images), step):
        for key, o in zip(keys[x:x + step], model([im.to(device) for im in images[x:x + step]])):
            keep0 = o["scores"] >= score_threshold
            if not bool(keep0.any()):
                missing.append(key)
                continue
            bs = o["boxes"][keep0]
            maxind = int(((bs[:, 2] - bs[:, 0]) * (bs[:, 3] - bs[:, 1])).argmax())
            aggr.append(agg(o["roi_features"][maxind].unsqueeze(0), one_i, zero_l)[1])
            match.append(o["match_features"][maxind].unsqueeze(0))
            boxes.append(bs[maxind].unsqueeze(0))
            scores.append(o["scores"][keep0][maxind].reshape(1))
            kept.append(key)
    if not kept:
        z = torch.zeros((0, 256), device=device)
        return ProductBank(z, z.clone(), torch.zeros((0, 4), device=device), torch.zeros((0,), device=device), [], missing)
    return ProductBank(torch.cat(match), torch.cat(aggr).reshape(len(kept), -1), torch.cat(boxes), torch.cat(scores), kept, missing)


@torch.no_grad()
def retrieve(model, clips, bank: ProductBank, k: int = 20, score_threshold: float = 0.0, tracking_threshold: float = 0.3,
             strategy: str = "aggr_desc", step: int = 11, min_track_len: int = 1) -> List[List[TrackletMatch]]:
    """Which products of ``bank`` does each garment of each clip show?  -> per clip a list of ``TrackletMatch`` in the linker's
    creation order (most confident seed first), tracklets shorter than ``min_track_len`` dropped, ``[]`` for a clip without a kept
    detection.

    ``clips``: a sequence of clips; a clip is what the model takes -- a sequence of float ``[3,H,W]`` or uint8 ``[H,W,3]`` frames,
    run through the detector in chunks of ``step``, or one ``PreparedImages`` (one forward).  Every detection with a score >=
    ``score_threshold`` is kept.  Then, for all clips together: one ``seam_pair_scores_blockdiag_f32`` launch (self-similarity of
    the ``match_features`` with the match predictor's classifier), one ``seam_build_tracklets_f32`` launch (the evaluator's greedy
    linking at ``tracking_threshold``, on the device), and per tracklet

    * ``"aggr_desc"``: its members' aggregator descriptors in ascending frame order through NLB Mode B (one call for all
      tracklets), ranked against ``bank.aggr`` with the aggregator's classifier;
    * ``"avg_desc"``: the mean of its members' ``match_features``, ranked against ``bank.match`` with the match predictor's;

    both through ``ops.pair_topk`` (exact top-k; min(k, len(bank)) <= 256).  These are the evaluator's AGGR DESC and AVG DESC,
    through the same code (``evaluator.aggregate_sequences`` / ``average_sequences``).

    Host synchronisations beyond the model's own: ONE to size the tracklet tables (the linker's output and the kept rows come back
    in one copy; the kept detections are compacted on the device, so nothing is read back before the linker) and ONE for the
    results.  Only when some clip has more detections than the linker's cap (``ops.build_tracklets_max_rows()``) are the kept
    counts read back first, to refuse the call before anything is launched.

    Refused with ValueError before any launch: an unknown strategy, an empty bank, a k beyond ``ops.pair_topk``'s capacity, and a
    clip whose kept detections exceed the linker's cap."""
    import numpy as np
    from . import evaluator as EV
    from . import ops
    from .models.detection import PreparedImages
    if strategy not in STRATEGIES:
        raise ValueError(f"retrieve: unknown strategy {strategy!r} (one of {', '.join(STRATEGIES)})")
    if len(bank) == 0:
        raise ValueError("retrieve: the product bank is empty")
    k = ops._topk_k(k, len(bank), "pair_topk")
    dev = _model_device(model)
    bank = bank.to(dev)
    heads = model.roi_heads
    agg, last = heads.temporal_aggregator, heads.match_predictor.last
    clips = list(clips)

    # ---- the detector, clip by clip; every detection becomes one row (frame, index inside the frame's output)
    scores, boxes, mfeat, roi_of_clip, frame_of, det_of, bounds = [], [], [], [], [], [], [0]
    for clip in clips:
        if isinstance(clip, PreparedImages):
            outs = model(clip)
        else:
            ims = [im.to(dev) for im in clip]
            outs = [o for x in range(0, len(ims), step) for o in model(ims[x:x + step])]
        rois = []
        for f, o in enumerate(outs):
            n = int(o["scores"].shape[0])
            scores.append(o["scores"]); boxes.append(o["boxes"]); mfeat.append(o["match_features"]); rois.append(o["roi_features"])
            frame_of += [f] * n
            det_of += list(range(n))
        roi_of_clip.append(rois)
        bounds.append(len(frame_of))
    N = bounds[-1]
    result: List[List[TrackletMatch]] = [[] for _ in clips]
    if N == 0:
        return result
    counts = np.diff(bounds)
    frame_of, det_of = np.asarray(frame_of), np.asarray(det_of)
    scores_all, boxes_all, mf_all = torch.cat(scores), torch.cat(boxes), torch.cat(mfeat)

    # ---- the kept rows first, in their order, without reading their number back: seg / out_off are formed on the device
    keep = scores_all >= score_threshold
    order = torch.sort((~keep).to(torch.uint8), stable=True)[1]
    csum = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), keep.cumsum(0)])
    seg_d = csum[torch.as_tensor(bounds, dtype=torch.int64, device=dev)].to(torch.int32)
    cap = ops.build_tracklets_max_rows()
    if int(counts.max()) > cap:
        for c, n in enumerate(seg_d.diff().cpu().tolist()):
            if n > cap:
                raise ValueError(f"retrieve: clip {c} keeps {n} detections, more than the tracklet linker's cap of {cap}; "
                                 "use a higher score_threshold")
    max_rows = min(int(counts.max()), cap)
    n_d = seg_d.diff().to(torch.int64)
    off_d = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), (n_d * n_d).cumsum(0)])
    x = mf_all[order].contiguous()
    imgs_d = torch.as_tensor(frame_of, dtype=torch.int32, device=dev)[order].contiguous()
    blocks = ops.pair_scores_blockdiag_device(x, seg_d, off_d, int((counts.astype(np.int64) ** 2).sum()), max_rows,
                                              last.weight.detach(), last.bias.detach())
    members, track_len, n_tracks, _ = ops.build_tracklets(blocks, off_d, seg_d, imgs_d, scores_all[order].contiguous(),
                                                          tracking_threshold, max_rows=max_rows)
    # ---- synchronisation 1: the tracklets and the kept rows
    host = torch.cat([seg_d, n_tracks, track_len, members, order.to(torch.int32)]).cpu().numpy()
    C = len(clips)
    seg_h, ntr = host[:C + 1], host[C + 1:2 * C + 1]
    lens_h, mem_h, order_h = host[2 * C + 1:2 * C + 1 + N], host[2 * C + 1 + N:2 * C + 1 + 2 * N], host[2 * C + 1 + 2 * N:]

    seqs = []           # (clip, kept rows of the tracklet in ascending frame order)
    for c in range(C):
        o, mo = int(seg_h[c]), 0
        for t in range(int(ntr[c])):
            ln = int(lens_h[o + t])
            rows = o + mem_h[o + mo:o + mo + ln].astype(np.int64)
            mo += ln
            if ln >= min_track_len:
                seqs.append((c, rows[np.argsort(frame_of[order_h[rows]], kind="stable")]))
    if not seqs:
        return result
    seg_q = np.concatenate([[0], np.cumsum([len(r) for _, r in seqs])])
    q_rows = np.concatenate([r for _, r in seqs])
    q_d = torch.as_tensor(q_rows, dtype=torch.int64, device=dev)
    if strategy == "aggr_desc":
        # the aggregator's trunk over every clip's kept detections, as collect_descriptors runs it
        parts = []
        for c in range(C):
            lo, hi = int(seg_h[c]), int(seg_h[c + 1])
            if hi > lo:
                local = torch.as_tensor(order_h[lo:hi].astype(np.int64) - bounds[c], device=dev)
                parts.append(agg.trunk(torch.cat(roi_of_clip[c])[local]))
        desc = EV.aggregate_sequences(agg, torch.cat(parts)[q_d], seg_q, bank.aggr[:1])
        idx, sc = ops.pair_topk(desc.contiguous(), bank.aggr, agg.last.weight, agg.last.bias, k)
    else:
        desc = EV.average_sequences(x[q_d].contiguous(), torch.as_tensor(seg_q, dtype=torch.int32, device=dev))
        idx, sc = ops.pair_topk(desc, bank.match, last.weight, last.bias, k)
    # ---- synchronisation 2: the results (one copy; float64 holds the indices and the fp32 values exactly)
    orig_d = order[q_d]
    P, Q = len(seqs), len(q_rows)
    out = torch.cat([idx.to(torch.float64).reshape(-1), sc.to(torch.float64).reshape(-1),
                     boxes_all[orig_d].to(torch.float64).reshape(-1), scores_all[orig_d].to(torch.float64)]).cpu()
    idx_h = out[:P * k].to(torch.int64).view(P, k)
    sc_h = out[P * k:2 * P * k].to(torch.float32).view(P, k)
    box_h = out[2 * P * k:2 * P * k + 4 * Q].to(torch.float32).view(Q, 4)
    det_sc_h = out[2 * P * k + 4 * Q:].to(torch.float32)
    for j, (c, rows) in enumerate(seqs):
        orig = order_h[rows]
        lo, hi = int(seg_q[j]), int(seg_q[j + 1])
        result[c].append(TrackletMatch(frames=frame_of[orig].tolist(), detections=det_of[orig].tolist(), boxes=box_h[lo:hi],
                                       scores=det_sc_h[lo:hi], product_idx=idx_h[j], product_keys=[bank.keys[i] for i in idx_h[j].tolist()],
                                       match_scores=sc_h[j]))
    return result
