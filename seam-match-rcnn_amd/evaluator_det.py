"""Box and mask average precision of the detector, COCO style, as DeepFashion2 scores it: 10 IoU thresholds, three area
ranges, at most 100 detections per image.

The reference has no detector evaluation (its evaluators measure retrieval only), and neither pycocotools nor torchvision
is a dependency here, so the protocol is restated in this file from the published COCO procedure (``COCOeval.evaluateImg``
/ ``accumulate`` / ``summarize``).  It has NOT been pinned against pycocotools itself: the tests pin it against an
independent float64 restatement (tests/det_eval_refs.py) and against hand-checked known answers.
``coco_results`` writes a run's detections as the entries of a COCO results file (boxes as xywh, masks as compressed RLE encoded on
the device): with it, a machine that has pycocotools can make that comparison.

Where the work runs:

    mask intersections [K,G], mask areas [K]  -> ``ops.mask_inter`` (seam_mask_inter_f32) straight from the 28x28
                                                 probabilities, the boxes and the uint8 ground-truth masks: no pasted
                                                 [K,1,H,W] mask exists (``model.paste_masks = False``)
    ground-truth pixel counts                 -> one torch reduction
    everything else                           -> host, NumPy float64, on a few hundred numbers per image

Each ``update`` brings all its device tables to the host in ONE copy.  Box IoU never touches the device, so a bbox-only
evaluator works on CPU tensors.

Deliberate choices: box IoU follows pycocotools' ``bbIou`` (xywh with w, h subtracted in fp32 and then widened to double;
a crowd ground truth divides by the detection's area); mask IoU is ``inter / (det_area + gt_pixels - inter)`` in float64
(crowd: ``inter / det_area``) and a zero denominator gives 0, where RLE arithmetic would divide by zero.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from . import ops

IOU_THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, 101)
AREA_RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))      # all, small, medium, large
AREA_NAMES = ("all", "small", "medium", "large")


class _HostFetch:
    """Collects the tensors an ``update`` needs on the host; device tensors travel together, as one float64 vector in one
    copy (fp32 boxes and scores, int32 counts and the labels of a detector are all exact in float64)."""

    def __init__(self):
        self._slots, self._dev, self._host = [], [], None

    def add(self, t: torch.Tensor) -> int:
        t = t.detach()
        if t.is_cuda:
            self._slots.append((len(self._dev), tuple(t.shape)))
            self._dev.append(t.reshape(-1).to(torch.float64))
        else:
            self._slots.append((None, t.to(torch.float64).numpy()))
        return len(self._slots) - 1

    def run(self) -> None:
        if self._dev:
            sizes = [int(t.numel()) for t in self._dev]
            flat = torch.cat(self._dev).cpu().numpy()          # the update's one device-to-host copy
            self._host = np.split(flat, np.cumsum(sizes)[:-1])

    def get(self, slot: int) -> np.ndarray:
        where, what = self._slots[slot]
        return what if where is None else self._host[where].reshape(what)


def _xywh(boxes: np.ndarray):
    """xyxy (fp32 values) -> x, y, w, h in float64 with w and h subtracted in fp32, as pycocotools' callers do."""
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 4).astype(np.float32)
    return (b[:, 0].astype(np.float64), b[:, 1].astype(np.float64),
            (b[:, 2] - b[:, 0]).astype(np.float64), (b[:, 3] - b[:, 1]).astype(np.float64))


def _box_iou_xywh(dx, dy, dw, dh, gx, gy, gw, gh, crowd: np.ndarray) -> np.ndarray:
    """pycocotools' ``bbIou`` on float64 x, y, w, h columns: [D] against [G] -> [D,G]."""
    dx, dy, dw, dh = (np.asarray(v, dtype=np.float64)[:, None] for v in (dx, dy, dw, dh))
    gx, gy, gw, gh = (np.asarray(v, dtype=np.float64)[None, :] for v in (gx, gy, gw, gh))
    iw = np.minimum(dx + dw, gx + gw) - np.maximum(dx, gx)
    ih = np.minimum(dy + dh, gy + gh) - np.maximum(dy, gy)
    inter = iw * ih
    union = np.where(crowd[None, :], np.broadcast_to(dw * dh, inter.shape), dw * dh + gw * gh - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / union
    return np.where((iw <= 0) | (ih <= 0), 0.0, iou)


def _box_iou(det: np.ndarray, gt: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    return _box_iou_xywh(*_xywh(det), *_xywh(gt), crowd)


def _mask_iou(inter: np.ndarray, det_area: np.ndarray, gt_pix: np.ndarray, crowd: np.ndarray) -> np.ndarray:
    inter = inter.astype(np.float64)
    den = np.where(crowd[None, :], np.broadcast_to(det_area[:, None], inter.shape), det_area[:, None] + gt_pix[None, :] - inter)
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / den
    return np.where(den == 0, 0.0, iou)


def _load_json(doc):
    """A parsed JSON document, or the path of one."""
    if isinstance(doc, (str, bytes)) or hasattr(doc, "__fspath__"):
        import json
        with open(doc) as f:
            return json.load(f)
    return doc


def _match(ious: List[List[float]], gt_ignore: List[bool], gt_crowd: List[bool]):
    """COCOeval.evaluateImg's greedy matching: ious[d][g] with the detections in score order and the ground truths ordered
    non-ignored first -> (matched [T,D] bool, matched-to-ignored [T,D] bool)."""
    nd, ng = len(ious), len(gt_ignore)
    matched = np.zeros((len(IOU_THRESHOLDS), nd), dtype=bool)
    ignored = np.zeros((len(IOU_THRESHOLDS), nd), dtype=bool)
    if ng == 0:
        return matched, ignored
    for ti, t in enumerate(IOU_THRESHOLDS):
        taken = [False] * ng
        for di in range(nd):
            row = ious[di]
            best, m = min(float(t), 1 - 1e-10), -1
            for gi in range(ng):
                if taken[gi] and not gt_crowd[gi]:
                    continue
                if m > -1 and not gt_ignore[m] and gt_ignore[gi]:
                    break
                if row[gi] < best:
                    continue
                best, m = row[gi], gi
            if m > -1:
                matched[ti, di] = True
                ignored[ti, di] = gt_ignore[m]
                taken[m] = True
    return matched, ignored


class DetectionEvaluator:
    """COCO-style AP / AR over the images fed to ``update``.

    outputs: one dict per image with ``boxes`` [K,4] xyxy in original-image pixels, ``labels`` [K], ``scores`` [K] and, for
    "segm", ``mask_probs`` [K,1,28,28] (``model.paste_masks = False``; read by ``ops.mask_inter``) or pasted ``masks``
    [K,1,H,W] (thresholded at > 0.5 with torch ops: the slow route, kept so that any model output works).
    targets: one dict per image with ``boxes`` [n,4] xyxy, ``labels`` [n], for "segm" ``masks`` uint8 [n,H,W], optionally
    ``area`` [n] and ``iscrowd`` [n].

    After ``summarize``: ``precision[iou_type]`` [T,R,K,A,M], ``recall[iou_type]`` [T,K,A,M] (-1 = no ground truth in that
    cell) and ``categories``, the sorted distinct ground-truth labels; detections of any other label are never evaluated."""

    def __init__(self, iou_types: Sequence[str] = ("bbox", "segm"), max_dets: Sequence[int] = (1, 10, 100)):
        iou_types = tuple(iou_types)
        if not iou_types or any(t not in ("bbox", "segm") for t in iou_types):
            raise ValueError("iou_types must be drawn from 'bbox' and 'segm'")
        max_dets = tuple(int(m) for m in max_dets)
        if len(max_dets) != 3 or min(max_dets) < 1 or list(max_dets) != sorted(max_dets):
            raise ValueError("max_dets must be three ascending positive integers")
        self.iou_types, self.max_dets = iou_types, max_dets
        self.images: List[dict] = []
        self.precision: Dict[str, np.ndarray] = {}
        self.recall: Dict[str, np.ndarray] = {}
        self.stats: Dict[str, List[float]] = {}
        self.categories: List[int] = []

    # ------------------------------------------------------------------------------------------ per batch
    def update(self, outputs, targets) -> None:
        outputs, targets = list(outputs), list(targets)
        if len(outputs) != len(targets):
            raise ValueError("one target dict per output dict is needed")
        fetch, slots = _HostFetch(), []
        for out, tgt in zip(outputs, targets):
            s = {k: fetch.add(out[k]) for k in ("boxes", "labels", "scores")}
            s.update({"gt_" + k: fetch.add(tgt[k]) for k in ("boxes", "labels", "area", "iscrowd") if k in tgt})
            if "segm" in self.iou_types:
                inter, det_area, gt_pix = self._mask_tables(out, tgt)
                s.update(inter=fetch.add(inter), det_area=fetch.add(det_area), gt_pix=fetch.add(gt_pix))
            slots.append(s)
        fetch.run()
        for s in slots:
            v = {k: fetch.get(i) for k, i in s.items()}
            gt_boxes = v["gt_boxes"].reshape(-1, 4)
            ng = gt_boxes.shape[0]
            crowd = v["gt_iscrowd"].reshape(-1) != 0 if "gt_iscrowd" in v else np.zeros(ng, dtype=bool)
            _, _, gw, gh = _xywh(gt_boxes)
            _, _, dw, dh = _xywh(v["boxes"])
            rec = dict(labels=v["labels"].reshape(-1).astype(np.int64), scores=v["scores"].reshape(-1),
                       gt_labels=v["gt_labels"].reshape(-1).astype(np.int64), gt_crowd=crowd,
                       gt_area=v["gt_area"].reshape(-1) if "gt_area" in v else gw * gh, iou={}, area={})
            nd = rec["labels"].shape[0]
            if not (len(rec["scores"]) == len(dw) == nd and len(rec["gt_labels"]) == len(rec["gt_area"]) == len(crowd) == ng):
                raise ValueError("boxes, labels, scores (and area, iscrowd) of an image must have one row per instance")
            if "bbox" in self.iou_types:
                rec["iou"]["bbox"] = _box_iou(v["boxes"], gt_boxes, crowd)
                rec["area"]["bbox"] = dw * dh
            if "segm" in self.iou_types:
                rec["iou"]["segm"] = _mask_iou(v["inter"].reshape(nd, ng), v["det_area"].reshape(-1), v["gt_pix"].reshape(-1),
                                               crowd)
                rec["area"]["segm"] = v["det_area"].reshape(-1)
            self.images.append(rec)

    def update_results(self, gt, results) -> None:
        """Score a saved COCO results file: ``gt`` is a COCO-format dict (or the path of its JSON) with ``images`` (``id``,
        ``height``, ``width``) and ``annotations`` (``image_id``, ``category_id``, ``bbox`` xywh, ``area``, ``iscrowd``,
        ``segmentation`` as polygons, uncompressed or compressed RLE); ``results`` is a list as ``coco_results`` writes it (or
        its path).  Every image of ``gt`` gets the record ``update`` builds -- an image without results counts its ground
        truths -- in the order of ``gt["images"]``; a result for an unknown image id raises ValueError.  Boxes: ``bbIou`` on the
        stored xywh values, detection area ``w*h``.  Masks: the detections' RLEs become bitmaps straight from their run lists,
        ground-truth polygons are rasterised (``mask_utils.masks_from_annotations``) and bit-packed by the encoder's values
        stage, and one pair-intersection launch serves as many images as ``ops_masks.RLE_BITS_BUDGET_BYTES`` holds (one host copy
        each); the detection area is the mask's popcount.  No model and no dense detection mask is involved."""
        from . import mask_utils as M
        gt, results = _load_json(gt), _load_json(results)
        images = list(gt["images"])
        index = {im["id"]: i for i, im in enumerate(images)}
        if len(index) != len(images):
            raise ValueError("update_results: image ids must be distinct")
        anns, dets = [[] for _ in images], [[] for _ in images]
        for a in gt.get("annotations", []):
            if a["image_id"] not in index:
                raise ValueError(f"update_results: annotation for unknown image id {a['image_id']!r}")
            anns[index[a["image_id"]]].append(a)
        for r in results:
            if r["image_id"] not in index:
                raise ValueError(f"update_results: result for unknown image id {r['image_id']!r}")
            dets[index[r["image_id"]]].append(r)
        need = [k for t, k in (("bbox", "bbox"), ("segm", "segmentation")) if t in self.iou_types]
        for r in results:
            if any(k not in r for k in need):
                raise ValueError(f"update_results: a result of image {r['image_id']!r} lacks {need}")
        sizes = [(int(im["height"]), int(im["width"])) for im in images]
        recs = []
        for a_i, d_i in zip(anns, dets):
            crowd = np.asarray([int(a.get("iscrowd", 0)) != 0 for a in a_i], dtype=bool)
            gbox = np.asarray([a["bbox"] for a in a_i], dtype=np.float64).reshape(-1, 4)
            rec = dict(labels=np.asarray([r["category_id"] for r in d_i], dtype=np.int64),
                       scores=np.asarray([r["score"] for r in d_i], dtype=np.float64),
                       gt_labels=np.asarray([a["category_id"] for a in a_i], dtype=np.int64), gt_crowd=crowd,
                       gt_area=np.asarray([a["area"] if "area" in a else a["bbox"][2] * a["bbox"][3] for a in a_i], dtype=np.float64),
                       iou={}, area={})
            if "bbox" in self.iou_types:
                dbox = np.asarray([r["bbox"] for r in d_i], dtype=np.float64).reshape(-1, 4)
                rec["iou"]["bbox"] = _box_iou_xywh(*(dbox[:, k] for k in range(4)), *(gbox[:, k] for k in range(4)), crowd)
                rec["area"]["bbox"] = dbox[:, 2] * dbox[:, 3]
            recs.append(rec)
        if "segm" in self.iou_types:
            cells = ops.rle_bits_cells(sizes)
            costs = [4 * c * (len(d_i) + len(a_i)) + h * w * sum(isinstance(a["segmentation"], (list, tuple)) for a in a_i)
                     for c, (h, w), a_i, d_i in zip(cells, sizes, anns, dets)]
            for lo, hi in ops.budget_chunks(costs):
                tables = M.results_inter_tables(anns[lo:hi], dets[lo:hi], sizes[lo:hi])
                for rec, (inter, d_area, g_pix) in zip(recs[lo:hi], tables):
                    rec["iou"]["segm"] = _mask_iou(inter, d_area.astype(np.float64), g_pix.astype(np.float64), rec["gt_crowd"])
                    rec["area"]["segm"] = d_area.astype(np.float64)
        self.images.extend(recs)

    @staticmethod
    def _mask_tables(out, tgt):
        """-> (inter [K,G], det_area [K], gt_pixels [G]) on the outputs' device."""
        src = out["mask_probs"] if "mask_probs" in out else out["masks"]
        gt = tgt["masks"]
        if gt.dim() != 3:
            raise ValueError("targets['masks'] must be [n,H,W]")
        gt = gt.to(src.device)
        if gt.dtype != torch.uint8:
            gt = (gt != 0).to(torch.uint8)
        gt = gt.contiguous()
        gt_pix = (gt != 0).sum((1, 2))
        if "mask_probs" in out:
            inter, det_area = ops.mask_inter(src, out["boxes"].to(torch.float32), gt)
            return inter, det_area, gt_pix
        m = src.reshape(src.shape[0], *src.shape[-2:]) > 0.5
        if tuple(m.shape[1:]) != tuple(gt.shape[1:]) and gt.shape[0]:
            raise ValueError("pasted masks and ground-truth masks differ in size")
        cols = [(m & (g != 0)[None]).sum((1, 2)) for g in gt]
        inter = torch.stack(cols, 1) if cols else torch.zeros((m.shape[0], 0), dtype=torch.int64, device=m.device)
        return inter, m.sum((1, 2)), gt_pix

    # ------------------------------------------------------------------------------------------ the protocol
    def _evaluate_image(self, rec, iou_type, cat, a):
        """One image, category and area range -> (scores [D], matched [T,D], ignored [T,D], non-ignored ground truths), with
        the detections in score order, or None when the image has neither."""
        g_idx = np.flatnonzero(rec["gt_labels"] == cat)
        d_idx = np.flatnonzero(rec["labels"] == cat)
        if g_idx.size == 0 and d_idx.size == 0:
            return None
        d_idx = d_idx[np.argsort(-rec["scores"][d_idx], kind="stable")][:self.max_dets[-1]]
        lo, hi = AREA_RANGES[a]
        g_area, g_crowd = rec["gt_area"][g_idx], rec["gt_crowd"][g_idx]
        g_ign = g_crowd | (g_area < lo) | (g_area > hi)
        order = np.argsort(g_ign, kind="stable")
        g_idx, g_ign, g_crowd = g_idx[order], g_ign[order], g_crowd[order]
        ious = rec["iou"][iou_type][np.ix_(d_idx, g_idx)]
        matched, ignored = _match(ious.tolist(), g_ign.tolist(), g_crowd.tolist())
        d_area = rec["area"][iou_type][d_idx]
        ignored |= ~matched & ((d_area < lo) | (d_area > hi))[None, :]
        return rec["scores"][d_idx], matched, ignored, int((~g_ign).sum())

    def _accumulate(self, iou_type):
        T, R, K, A, M = len(IOU_THRESHOLDS), len(RECALL_THRESHOLDS), len(self.categories), len(AREA_RANGES), len(self.max_dets)
        precision = -np.ones((T, R, K, A, M))
        recall = -np.ones((T, K, A, M))
        for k, cat in enumerate(self.categories):
            for a in range(A):
                per_image = [e for e in (self._evaluate_image(rec, iou_type, cat, a) for rec in self.images) if e is not None]
                npig = sum(e[3] for e in per_image)
                if npig == 0:
                    continue
                for m, max_det in enumerate(self.max_dets):
                    scores = np.concatenate([e[0][:max_det] for e in per_image]) if per_image else np.zeros(0)
                    order = np.argsort(-scores, kind="stable")
                    matched = np.concatenate([e[1][:, :max_det] for e in per_image], axis=1)[:, order]
                    ignored = np.concatenate([e[2][:, :max_det] for e in per_image], axis=1)[:, order]
                    tp = np.cumsum(matched & ~ignored, axis=1).astype(np.float64)
                    fp = np.cumsum(~matched & ~ignored, axis=1).astype(np.float64)
                    for t in range(T):
                        rc = tp[t] / npig
                        pr = tp[t] / (tp[t] + fp[t] + np.spacing(1))
                        recall[t, k, a, m] = rc[-1] if rc.size else 0.0
                        pr = np.maximum.accumulate(pr[::-1])[::-1]             # non-increasing from the right
                        at = np.searchsorted(rc, RECALL_THRESHOLDS, side="left")
                        q = np.zeros(R)
                        q[at < rc.size] = pr[at[at < rc.size]]
                        precision[t, :, k, a, m] = q
        return precision, recall

    def summarize(self, verbose: bool = True) -> Dict[str, List[float]]:
        self.categories = sorted({int(c) for rec in self.images for c in rec["gt_labels"]})
        last = len(self.max_dets) - 1

        def mean(cells):
            cells = cells[cells > -1]
            return float(cells.mean()) if cells.size else -1.0

        for iou_type in self.iou_types:
            precision, recall = self._accumulate(iou_type)
            self.precision[iou_type], self.recall[iou_type] = precision, recall
            t50 = int(np.argmin(np.abs(IOU_THRESHOLDS - 0.5))), int(np.argmin(np.abs(IOU_THRESHOLDS - 0.75)))
            rows = [("AP", None, 0, last), ("AP", t50[0], 0, last), ("AP", t50[1], 0, last),
                    ("AP", None, 1, last), ("AP", None, 2, last), ("AP", None, 3, last),
                    ("AR", None, 0, 0), ("AR", None, 0, 1), ("AR", None, 0, 2),
                    ("AR", None, 1, last), ("AR", None, 2, last), ("AR", None, 3, last)]
            stats = []
            for kind, t, a, m in rows:
                tsel = slice(None) if t is None else slice(t, t + 1)
                stats.append(mean(precision[tsel, :, :, a, m] if kind == "AP" else recall[tsel, :, a, m]))
            self.stats[iou_type] = stats
            if verbose:
                print(f"IoU metric: {iou_type}")
                for (kind, t, a, m), s in zip(rows, stats):
                    title = "Average Precision" if kind == "AP" else "Average Recall"
                    iou = "0.50:0.95" if t is None else f"{IOU_THRESHOLDS[t]:0.2f}"
                    print(f" {title:<18} ({kind}) @[ IoU={iou:<9} | area={AREA_NAMES[a]:>6s} | "
                          f"maxDets={self.max_dets[m]:>3d} ] = {s:0.3f}")
        return {t: list(self.stats[t]) for t in self.iou_types}


def coco_results(outputs, image_ids, sizes, label_to_category=None, iou_types: Sequence[str] = ("bbox", "segm")) -> List[dict]:
    """The detections of a batch as the entries of a COCO results file (what pycocotools' ``loadRes`` and the DeepFashion2
    tooling read): per detection ``image_id``, ``category_id``, ``score`` and, by ``iou_types``, ``bbox`` = [x, y, w, h] (w and h
    subtracted in fp32, as ``_xywh``) and ``segmentation`` = {"size": [h, w], "counts": <ascii str>}, the compressed RLE of the
    mask thresholded at > 0.5.  ``outputs``: one dict per image as ``DetectionEvaluator.update`` takes them -- ``mask_probs``
    (``model.paste_masks = False``) are encoded without a pasted mask (``mask_utils.encode_detections``), pasted ``masks``
    [K,1,H,W] through ``mask_utils.encode``; ``sizes[i] = (h, w)`` of image i; ``label_to_category``: mapping (or sequence)
    from the model's labels to the dataset's category ids, identity when None.  The list holds plain ``int``, ``float`` and
    ``str`` only: ``json.dump(results, f)`` writes the file."""
    from . import mask_utils
    iou_types = tuple(iou_types)
    if not iou_types or any(t not in ("bbox", "segm") for t in iou_types):
        raise ValueError("iou_types must be drawn from 'bbox' and 'segm'")
    outputs, image_ids, sizes = list(outputs), list(image_ids), list(sizes)
    if not len(outputs) == len(image_ids) == len(sizes):
        raise ValueError("one image id and one size per output dict are needed")
    results = []
    for out, image_id, size in zip(outputs, image_ids, sizes):
        fetch = _HostFetch()
        slots = {k: fetch.add(out[k]) for k in ("boxes", "labels", "scores")}
        rles = None
        if "segm" in iou_types:                                   # the encoder's copies first, then the image's one table copy
            h, w = int(size[0]), int(size[1])
            if "mask_probs" in out:
                rles = mask_utils.encode_detections(out["mask_probs"], out["boxes"], (h, w))
            else:
                m = out["masks"]
                m = m.reshape(m.shape[0], *m.shape[-2:])
                if tuple(m.shape[1:]) != (h, w):
                    raise ValueError(f"pasted masks of {tuple(m.shape[1:])} on an image of {(h, w)}")
                rles = mask_utils.encode((m > 0.5).to(torch.uint8)) if m.shape[0] else []
        fetch.run()
        boxes = fetch.get(slots["boxes"]).reshape(-1, 4)
        labels = fetch.get(slots["labels"]).reshape(-1).astype(np.int64)
        scores = fetch.get(slots["scores"]).reshape(-1)
        if not (len(labels) == len(scores) == len(boxes)) or (rles is not None and len(rles) != len(boxes)):
            raise ValueError("boxes, labels, scores (and masks) of an image must have one row per detection")
        x, y, bw, bh = _xywh(boxes)
        image_id = image_id.item() if hasattr(image_id, "item") else image_id
        for k in range(len(labels)):
            cat = int(labels[k]) if label_to_category is None else label_to_category[int(labels[k])]
            r = {"image_id": image_id, "category_id": int(cat), "score": float(scores[k])}
            if "bbox" in iou_types:
                r["bbox"] = [float(x[k]), float(y[k]), float(bw[k]), float(bh[k])]
            if rles is not None:
                r["segmentation"] = {"size": list(rles[k]["size"]), "counts": rles[k]["counts"].decode("ascii")}
            results.append(r)
    return results


def evaluate(model, data_loader, device, iou_types: Sequence[str] = ("bbox", "segm"), verbose: bool = True,
             return_report: bool = False):
    """Box and mask AP of ``model`` over the phase-1 loader of the reference (train_matchrcnn.py's ``(images, targets)`` or
    ``(images, targets, ids)`` batches; targets: ``boxes`` xyxy in original pixels, ``labels`` int64, ``masks`` uint8
    [n,H,W], optionally ``area`` and ``iscrowd``).  The model runs in ``eval()`` under ``no_grad`` with
    ``paste_masks = False`` (restored afterwards, also when the loader raises): no pasted mask is ever written.
    -> {"bbox": [12 floats], "segm": [12 floats]} in COCO's order; with ``return_report`` also the evaluator."""
    ev = DetectionEvaluator(iou_types)
    if hasattr(model, "eval"):
        model.eval()
    own = getattr(model, "__dict__", {})
    had, old = "paste_masks" in own, own.get("paste_masks")
    model.paste_masks = False
    try:
        with torch.no_grad():
            for batch in data_loader:
                images, targets = batch[0], batch[1]
                outputs = model([im.to(device) for im in images])
                ev.update(outputs, targets)
    finally:
        if had:
            model.paste_masks = old
        else:
            del model.paste_masks
    stats = ev.summarize(verbose=verbose)
    return (stats, ev) if return_report else stats


def evaluate_results(gt, results, iou_types: Sequence[str] = ("bbox", "segm"), verbose: bool = True, return_report: bool = False):
    """Box and mask AP of a saved COCO results file against a COCO annotation file (dicts / lists or paths, as
    ``DetectionEvaluator.update_results`` takes them): run the detector once, keep ``coco_results``' JSON, score it later.
    -> {"bbox": [12 floats], "segm": [12 floats]} in COCO's order; with ``return_report`` also the evaluator."""
    ev = DetectionEvaluator(iou_types)
    ev.update_results(gt, results)
    stats = ev.summarize(verbose=verbose)
    return (stats, ev) if return_report else stats
