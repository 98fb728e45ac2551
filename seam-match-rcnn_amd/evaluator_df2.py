"""Multi-DeepFashion2 retrieval evaluation on the device in fp32.

Counterpart of ``evaluate()`` in the reference's evaluate_multiDF2.py:16-327: descriptor collection (:26-114), the six
rankings per product (:157-274) and the accuracy tables (:278-325).  The reference copies every frame's detections to the host,
runs a pycocotools IoU there, scans the GT rows in Python and keeps its tables as NumPy fp16.  Here:

    per-frame GT selection (:43-57,75-89)      -> seam_gt_select_f32, one launch + one copy per product (all its images)
    compute_ranking(...) == shop_prod_index    -> seam_pair_logits_f32 + seam_rank_of_f32
    compute_distances / AVG & MAX DISTANCE     -> seam_match_scores_f32 + seam_score_reduce_seg_f32 + seam_rank_of_scores_f32
    AVG DESC                                   -> seam_score_reduce_seg_f32 + seam_rank_of_f32
    AGGR DESC                                  -> TemporalAggregationNLB Mode B (seam_nlb_attnpool_f32) + seam_rank_of_f32

and the ranking stage is batched over products as ``evaluator.evaluate_tables`` does.

Reference behaviours kept on purpose: the model runs in chunks of 6 images; the product's GT row is searched in the SHOP image's
``styles`` / ``pair_ids`` for every image, the loop bounded by that image's GT count (not found -> -1 = the last row);
``first_n_withvideo`` is tested after ``count_products`` advances; the product loop is ``range(count_street)``, not the kept
products; the shop detection is taken at its position in the thresholded list but read from the full output (:61-67);
``total_querys = count_street * frames_per_product``; a maximum-distance hit also counts as "maxscore" per product.  Where the
reference dies with an IndexError (GT search past the shop's lists, an image without GT boxes) or on ``torch.cat([])`` (a
product without any kept street frame), a ValueError names the product and the frame.

Deliberate deviations (as in the MovingFashion evaluator): fp32 tables instead of the reference's fp16 (:116-124); ties rank the
lower gallery index first instead of following NumPy's unstable reversed argsort; ``strategy`` other than "best_match" /
"best_box_only" is rejected (this protocol keeps one detection per frame, so both give the same report).
"""
from __future__ import annotations

import copy
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops
from .evaluator import K_THRESHOLDS
from .input_pipeline import apply_noise

STEP = 6                                # images per model call (:35)
STRATEGIES = ("best_match", "best_box_only")


def _as_list(v) -> list:
    return v.tolist() if isinstance(v, torch.Tensor) else list(v)


def resolve_gt_row(styles, pair_ids, style: int, pair_id: int, n_rows: int, where: str = "") -> int:
    """evaluate_multiDF2.py:55-60,88-92: the first row r < ``n_rows`` (the image's own GT count) with styles[r] == style and
    pair_ids[r] == pair_id, looked up in the SHOP image's lists for every image; -1 (= the image's last row) when there is none.
    Where the scan runs past the shop's lists the reference raises IndexError: ValueError here, naming the image."""
    styles, pair_ids = _as_list(styles), _as_list(pair_ids)
    for r in range(n_rows):
        if r >= len(styles) or r >= len(pair_ids):
            raise ValueError(f"evaluate: {where}: GT row {r} of {n_rows} has no entry in the shop image's styles / pair_ids "
                             f"({len(styles)} rows) while searching for style {style}, pair_id {pair_id}")
        if styles[r] == style and pair_ids[r] == pair_id:
            return r
    return -1


@dataclass
class DF2Tables:
    """What evaluate_multiDF2.py:116-124 builds from its per-detection tuples: descriptors on the device (fp32), bookkeeping on
    the host."""
    shop_mat: torch.Tensor              # [Ns,256] match_features of each product's chosen shop detection
    shop_aggr: torch.Tensor             # [Ns,256] temporal_aggregator(roi, [1], [0])[1] of the same detection (:62-64)
    shop_prods: np.ndarray              # [Ns] product index (count_products - 1)
    shop_keys: list                     # [Ns] targets[0]["i"]
    shop_sel: np.ndarray                # [Ns] the detection index the reference reads (its position in the kept list, :57,62)
    street_mat: torch.Tensor            # [Nq,256] match_features of each kept street frame's chosen detection
    street_aggr: torch.Tensor           # [Nq,256] temporal_aggregator(rois, 0, 0)[3][1:] (:103-110)
    street_prods: np.ndarray            # [Nq]
    street_imgs: np.ndarray             # [Nq] street frame index (0 = the first image after the shop image)
    street_sel: np.ndarray              # [Nq] chosen detection index in the frame's full output
    street_scores: np.ndarray           # [Nq]
    street_boxes: torch.Tensor          # [Nq,4]
    w: torch.Tensor                     # [2,256] match_predictor.last.weight (output[0]["w"])
    b: torch.Tensor                     # [2]
    count_street: int = 0
    count_products: int = 0


@torch.no_grad()
def collect_descriptors(model, data_loader, device, score_threshold: float = 0.1, first_n_withvideo: Optional[int] = None,
                        use_gt: bool = False) -> DF2Tables:
    """evaluate_multiDF2.py:26-114: run the model over (shop image, street frames...) batches in chunks of 6, pick in every image
    the kept detection that best overlaps the product's GT box (one seam_gt_select_f32 launch per product) and gather the
    descriptors of the chosen detections.  A batch whose targets carry ``"noise_sigma"`` goes through
    ``input_pipeline.apply_noise`` first."""
    agg = model.roi_heads.temporal_aggregator
    shop_mat, shop_aggr, shop_prods, shop_keys, shop_sel = [], [], [], [], []
    s_mat, s_aggr, s_prod, s_img, s_sel, s_score, s_box = [], [], [], [], [], [], []
    w = b = None
    count_products = count_street = 0
    for batch in data_loader:
        images, targets_in = batch[0], batch[1]
        count_products += 1
        product = count_products - 1
        if any("noise_sigma" in t for t in targets_in):     # a lazy MultiDeepFashion2Dataset: its noise, on the device
            images, targets_in = apply_noise(images, targets_in, device)
        images = [im.to(device) for im in images]
        targets = [{k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in t.items()} for t in targets_in]
        targets = [{k: (v.float() if k == "boxes" else v) for k, v in t.items()} for t in targets]
        if use_gt:
            targets2 = copy.deepcopy(targets)
            output = [o for x in range(0, len(images), STEP) for o in model(images[x:x + STEP], targets=targets2[x:x + STEP])]
        else:
            output = [o for x in range(0, len(images), STEP) for o in model(images[x:x + STEP])]

        # ---- GT rows on the host (shapes and the shop image's lists only), the selection for every image in one launch
        key = targets[0]["i"]
        style, pair_id = [int(x) for x in key.split("_")]
        gt = [t["boxes"].reshape(-1, 4) for t in targets]
        rows, row_err = [], []
        for n, g in enumerate(gt):
            try:
                rows.append(resolve_gt_row(targets_in[0].get("styles", ()), targets_in[0].get("pair_ids", ()), style, pair_id,
                                           g.shape[0], f"product {product} ({key!r}), " + ("shop image" if n == 0 else f"street frame {n - 1}")))
                row_err.append(None)
            except ValueError as e:
                rows.append(0)
                row_err.append(e)
        det_off = np.cumsum([0] + [o["scores"].shape[0] for o in output])
        gt_off = np.cumsum([0] + [g.shape[0] for g in gt])
        sel = ops.gt_select(torch.cat([o["boxes"].reshape(-1, 4) for o in output]).float(),
                            torch.cat([o["scores"].reshape(-1) for o in output]).float(), det_off,
                            torch.cat(gt), gt_off, torch.as_tensor(rows, dtype=torch.int32).to(device), score_threshold)
        sel_idx, sel_pos, status = torch.stack(sel).cpu().numpy()

        def check(n):
            what = f"product {product} ({key!r}), " + ("shop image" if n == 0 else f"street frame {n - 1}")
            if row_err[n] is not None:
                raise row_err[n]
            if status[n] != 0:          # the reference: IndexError on iou[prodind] (:57,89)
                raise ValueError(f"evaluate: {what} has no ground-truth box to match" if status[n] == 1 else
                                 f"evaluate: {what}: GT row {rows[n]} outside its {gt[n].shape[0]} GT boxes")

        kept = (sel_idx >= 0) | (status != 0)
        if not kept[0]:                 # (:42-43) nothing above the threshold in the shop image: the product is skipped
            continue
        check(0)
        if w is None:
            w, b = output[0]["w"].detach(), output[0]["b"].detach()
        pos = int(sel_pos[0])           # the position in the kept list indexes the FULL output (:57,61-67)
        shop_aggr.append(agg(output[0]["roi_features"][pos:pos + 1], torch.ones(1, dtype=torch.int32),
                             torch.zeros(1, dtype=torch.int64))[1].reshape(1, -1))
        shop_mat.append(output[0]["match_features"][pos:pos + 1])
        shop_prods.append(product)
        shop_keys.append(key)
        shop_sel.append(pos)
        if first_n_withvideo is not None and count_products >= first_n_withvideo:
            continue
        count_street += 1
        feats = []
        for i, o in enumerate(output[1:]):
            if not kept[i + 1]:
                continue
            check(i + 1)
            d = int(sel_idx[i + 1])
            s_mat.append(o["match_features"][d:d + 1])
            s_score.append(o["scores"][d:d + 1])
            s_box.append(o["boxes"][d:d + 1].reshape(1, 4))
            s_prod.append(product)
            s_img.append(i)
            s_sel.append(d)
            feats.append(o["roi_features"][d:d + 1])
        if not feats:                   # the reference fails on torch.cat([]) (:99)
            raise ValueError(f"evaluate: product {product} ({key!r}) has a shop detection but no street frame with a detection "
                             f"scoring >= {score_threshold}")
        feats = torch.cat(feats, 0)
        n = feats.shape[0]
        seq = agg(feats, torch.zeros(n, dtype=torch.int32), torch.zeros(n, dtype=torch.int64))[3][1:]
        s_aggr.append(seq.reshape(-1, seq.shape[-1]))
    if not shop_mat or not s_mat:
        raise ValueError("evaluate: no product has a shop detection and a street frame above the score threshold")
    return DF2Tables(
        shop_mat=torch.cat(shop_mat).float(), shop_aggr=torch.cat(shop_aggr).float(), shop_prods=np.asarray(shop_prods),
        shop_keys=shop_keys, shop_sel=np.asarray(shop_sel), street_mat=torch.cat(s_mat).float(), street_aggr=torch.cat(s_aggr).float(),
        street_prods=np.asarray(s_prod), street_imgs=np.asarray(s_img), street_sel=np.asarray(s_sel),
        street_scores=torch.cat(s_score).cpu().numpy(), street_boxes=torch.cat(s_box), w=w, b=b, count_street=count_street,
        count_products=count_products)


_TABLES = ("frame", "max_per_image", "avg_desc", "aggr_desc", "avg_dist", "max_dist", "max_score")
_PRINTED = (("frame", ""), ("avg_desc", " Product Avg Desc"), ("aggr_desc", " Product Aggr Desc"), ("avg_dist", " Product Avg Dist"),
            ("max_dist", " Product Max Dist"), ("max_score", " Product Max Score"))


@dataclass
class DF2Report:
    k_thresholds: Sequence[int]
    counts: Dict[str, np.ndarray] = field(default_factory=dict)     # name -> hits per k threshold
    count_street: int = 0
    frames_per_product: int = 0
    frame_ranks: List[int] = field(default_factory=list)            # all_ranks_list (:190)
    per_product: Dict = field(default_factory=dict)                 # accs_per_product (:170-177,266-272)
    tables: Optional[DF2Tables] = None                              # what ``evaluate`` collected (chosen detections included)

    def accuracy(self, name: str) -> np.ndarray:
        denom = self.count_street * self.frames_per_product if name == "frame" else self.count_street
        return self.counts[name] / max(denom, 1)

    def summary(self):
        """(ret1, ret2, ret3) as the reference returns them (:279-289,327)."""
        return (float(self.accuracy("frame")[0]), float(self.accuracy("avg_desc")[0]), float(self.accuracy("aggr_desc")[0]))

    def tables_text(self) -> str:
        """The six tables and the rank quartiles exactly as the reference prints them (:276-310).  (No products prints nan where the
        reference raises ZeroDivisionError.)"""
        lines = []
        for name, title in _PRINTED:
            denom = self.count_street * self.frames_per_product if name == "frame" else self.count_street
            for k, hits in zip(self.k_thresholds, self.counts[name]):
                lines.append("Top-%d Retrieval Accuracy%s: %1.4f" % (k, title, int(hits) / denom if denom else float("nan")))
            lines.append("*" * 50)
        ranks = np.asarray(self.frame_ranks)
        lines.append(f"Rank median: {np.median(ranks)}; rank 1st quartile: {np.percentile(ranks, 25)}; "
                     f"rank 3rd quartile: {np.percentile(ranks, 75)}")
        return "\n".join(lines) + "\n"

    def perf_rows(self) -> np.ndarray:
        """The 8 x len(k) block of logs_mdf2/<time>.csv (:312-322): rows 0-3 = per-frame, mean-rank, avg-desc and aggr-desc
        accuracies in percent, rows 4-7 zero."""
        perf = np.zeros((8, len(self.k_thresholds)))
        perf[0] = np.asarray(self.counts["frame"], dtype=np.float32) / (self.count_street * self.frames_per_product)
        for row, name in ((1, "max_per_image"), (2, "avg_desc"), (3, "aggr_desc")):
            perf[row] = np.asarray(self.counts[name], dtype=np.float32) / self.count_street
        return perf * 100

    def save_artifacts(self, directory: str = ".") -> None:
        """``accs_per_product_10frame_df2.pth`` (:274) and ``logs_mdf2/<time>.csv`` (:320-322)."""
        import os
        import time
        torch.save(self.per_product, os.path.join(directory, "accs_per_product_10frame_df2.pth"))
        os.makedirs(os.path.join(directory, "logs_mdf2"), exist_ok=True)
        np.savetxt(os.path.join(directory, "logs_mdf2", str(time.time()) + ".csv"), self.perf_rows(), fmt="%02.2f", delimiter="\t")


def check_strategy(strategy: str) -> str:
    if strategy not in STRATEGIES:
        raise ValueError(f"evaluate: strategy must be one of {STRATEGIES}, got {strategy!r}")
    return strategy


@torch.no_grad()
def evaluate_tables(t: DF2Tables, temporal_aggregator, k_thresholds: Sequence[int] = K_THRESHOLDS, frames_per_product: int = 3,
                    strategy: str = "best_match", max_pairs_per_pass: int = 1 << 25) -> DF2Report:
    """evaluate_multiDF2.py:157-272 on device-resident tables, batched over products: per pass (as many products as fit
    ``max_pairs_per_pass`` (query, shop) pairs) the per-frame ranks, the distance rows and their mean / max, AVG DESC and AGGR DESC
    (Mode B over S = #products sequences) are one launch each and one device -> host copy."""
    check_strategy(strategy)        # one detection per (product, frame): best_box_only's argmax over it is that detection
    ks = np.asarray(k_thresholds)
    rep = DF2Report(k_thresholds=tuple(k_thresholds), count_street=t.count_street, frames_per_product=frames_per_product)
    for name in _TABLES:
        rep.counts[name] = np.zeros(len(ks), dtype=np.int64)
    dev = t.shop_mat.device
    aggr_w, aggr_b = temporal_aggregator.last.weight.detach(), temporal_aggregator.last.bias.detach()
    G = t.shop_mat.shape[0]

    first_shop = {}
    for i, pr in enumerate(t.shop_prods.tolist()):
        first_shop.setdefault(pr, i)
    order = np.lexsort((t.street_imgs, t.street_prods))       # by product, then frame (np.unique(street_imgs) order, :165)
    sp_sorted = t.street_prods[order]
    todo = []
    for p in range(t.count_street):                          # (:161-162) NOT a loop over the kept products
        if p not in first_shop:
            continue
        lo, hi = np.searchsorted(sp_sorted, p, "left"), np.searchsorted(sp_sorted, p, "right")
        if hi == lo:
            raise ValueError(f"evaluate: product {p} has no street detections")
        todo.append((p, first_shop[p], order[lo:hi]))

    def idx(a):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int64, device=dev)

    pos = 0
    while pos < len(todo):
        batch, nq = [], 0
        while pos < len(todo) and (not batch or (nq + len(todo[pos][2])) * max(G, 1) <= max_pairs_per_pass):
            batch.append(todo[pos])
            nq += len(todo[pos][2])
            pos += 1
        P = len(batch)
        seg = np.cumsum([0] + [len(d) for _, _, d in batch])
        q_all = np.concatenate([d for _, _, d in batch])
        q_d = idx(q_all)
        shop_idx = np.asarray([si for _, si, _ in batch])
        target_p = idx(shop_idx)
        target_q = idx(np.repeat(shop_idx, np.diff(seg)))
        queries = t.street_mat[q_d].contiguous()
        logits = ops.pair_logits(queries, t.shop_mat, t.w, t.b)
        frame_rank_d = ops.rank_of(logits, target_q)                                      # compute_ranking (:143-149,168-170)
        distances = ops.match_scores(logits)                                              # compute_distances (:151-156,177)
        del logits
        seg_d = torch.as_tensor(seg, dtype=torch.int32, device=dev)
        avg_rank_d = ops.rank_of(ops.pair_logits(ops.score_reduce_segments(queries, seg_d, "mean"), t.shop_mat, t.w, t.b), target_p)
        both = torch.cat([ops.score_reduce_segments(distances, seg_d, "mean"), ops.score_reduce_segments(distances, seg_d, "max")])
        dist_rank_d = ops.rank_of_scores(both, target_p.repeat(2))
        tmax = int(np.diff(seg).max())
        seq = torch.zeros((1 + tmax, P, t.street_aggr.shape[1]), device=dev)
        trow = np.concatenate([1 + np.arange(n) for n in np.diff(seg)])
        tcol = np.repeat(np.arange(P), np.diff(seg))
        seq[idx(trow), idx(tcol)] = t.street_aggr[q_d]
        mask = torch.as_tensor(np.arange(1 + tmax)[None, :] > np.diff(seg)[:, None], device=dev)
        desc = temporal_aggregator(None, None, None, x3_1_seq=seq, x3_1_mask=mask, x3_2=t.shop_aggr[:1])[0][:P]
        aggr_rank_d = ops.rank_of(ops.pair_logits(desc.contiguous(), t.shop_aggr, aggr_w, aggr_b), target_p)
        ranks = torch.cat([frame_rank_d, avg_rank_d, dist_rank_d, aggr_rank_d]).cpu().numpy()
        frame_rank_all, avg_rank = ranks[:nq], ranks[nq:nq + P]
        dist_rank, aggr_rank = ranks[nq + P:nq + 3 * P], ranks[nq + 3 * P:]

        for j, (p, shop_index, dets) in enumerate(batch):
            per = {k: np.zeros(len(ks), dtype=np.int64) for k in ("sfmr", "seamrcnn", "bmfm", "avgdist", "maxdist", "maxscore")}

            def hit(name, rank, *keys):
                h = (rank < ks).astype(np.int64)
                rep.counts[name] += h
                for k in keys:
                    per[k] += h

            frame_rank = frame_rank_all[seg[j]:seg[j + 1]]
            for r in frame_rank:
                hit("frame", r, "sfmr")
            hit("max_per_image", int(np.mean(frame_rank)))                                # (:184-188)
            rep.frame_ranks += [int(r) for r in frame_rank]
            hit("aggr_desc", int(aggr_rank[j]), "seamrcnn")
            hit("avg_desc", int(avg_rank[j]), "bmfm")
            hit("avg_dist", int(dist_rank[j]), "avgdist")
            hit("max_dist", int(dist_rank[P + j]), "maxscore", "maxdist")                 # (:256-262)
            hit("max_score", int(frame_rank[int(np.argmax(t.street_scores[dets]))]))      # (:264-270)
            rep.per_product[t.shop_keys[shop_index]] = {
                "sfmr": per["sfmr"] / frames_per_product, "seamrcnn": per["seamrcnn"] / 1.0, "bmfm": per["bmfm"] / 1.0,
                "avgdist": per["avgdist"] / 1.0, "maxdist": per["maxdist"] / 1.0, "maxscore": per["maxscore"] / 1.0}
    return rep


@torch.no_grad()
def evaluate(model, data_loader, device, strategy: str = "best_match", score_threshold: float = 0.1,
             k_thresholds: Sequence[int] = K_THRESHOLDS, frames_per_product: int = 3, tracking_threshold: float = 0.7,
             first_n_withvideo: Optional[int] = None, use_gt: bool = False, return_report: bool = False, verbose: bool = True,
             artifacts_dir: Optional[str] = None):
    """Same signature and return value (ret1, ret2, ret3) as the reference's ``evaluate`` (evaluate_multiDF2.py:16-18,327);
    ``tracking_threshold`` is accepted and unused, as there.  ``verbose`` prints the tables as the reference does (:276-310);
    ``artifacts_dir`` (e.g. ".") also writes ``accs_per_product_10frame_df2.pth`` and ``logs_mdf2/<time>.csv`` there -- the
    reference always writes them into the working directory; here that is opt-in."""
    check_strategy(strategy)
    tables = collect_descriptors(model, data_loader, device, score_threshold, first_n_withvideo, use_gt)
    rep = evaluate_tables(tables, model.roi_heads.temporal_aggregator, k_thresholds, frames_per_product, strategy)
    rep.tables = tables
    if verbose:
        print(rep.tables_text(), end="")
    if artifacts_dir is not None:
        rep.save_artifacts(artifacts_dir)
    return (rep.summary(), rep) if return_report else rep.summary()
