"""Synthetic Multi-DeepFashion2 retrieval datasets for the DF2 evaluator parity tests (test infrastructure).

The reference's ``evaluate(model, data_loader, device, ...)`` (evaluate_multiDF2.py:16-327) consumes a model that returns one dict
per image (``scores, boxes, match_features, roi_features, w, b``) and a loader of ``(images, targets, ids)`` triples -- image 0 is
the product's shop picture, the rest its street frames; every target carries the image's GT ``boxes`` (xyxy) with their
``styles`` / ``pair_ids`` and the product key ``i = "<style>_<pair_id>"``.  This module builds such loaders with CANNED detections
(the geometry of tests/eval_scenarios.py: descriptors on axis 0 at the product's coordinate plus a drift, distractors far out
on axis 1, the same classifier and aggregator), so that the DF2 logic after the detector -- GT-row lookup, IoU choice of the
detection, the six rankings, the counters -- runs identically through the imported reference (tests/golden/make_df2_eval_golden.py)
and the device evaluator.

Every image holds 2-3 garments side by side (GT rows), the product's garment in one of them.  Detection kinds:
``true`` (the product's garment, small jitter), ``dup`` (the same garment, loose box), ``lure`` (the most confident box of the
image, shifted half a garment off: low IoU, far descriptor), ``off`` (a box outside every garment: IoU 0, descriptor of the
product), ``other`` (another garment: IoU 0 with the product's, far descriptor), ``low`` (below any threshold used here).
"""
from __future__ import annotations

import numpy as np
import torch

import eval_scenarios as ES
from eval_scenarios import FAR_BOX, SPACING, _desc, _jit, _roi, aggregator_state, classifier   # noqa: F401

STYLE0, PAIR0 = 3, 100          # product p: style STYLE0 + p % 3, pair_id PAIR0 + p
SLOT_W, SLOT_H = 150, 260


def _slot_box(p, img, slot):
    x = 30 + 170 * slot + (p * 5 + img * 3) % 11
    y = 40 + (p * 7 + img) % 13
    return np.asarray([x, y, x + SLOT_W, y + SLOT_H], np.float32)


def _frac(p, f):
    return 0.2 + 0.01 * ((p + 2 * f) % 5 - 2)


def _det(seed, tag, kind, score, a0, gt_box, p):
    if kind == "true":
        box, a1, roi = gt_box + _jit(seed, tag, 6.0), 0.0, (seed, tag, p, None, 0.0)
    elif kind == "dup":
        box, a1, roi = gt_box + _jit(seed, tag, 30.0), 0.35, (seed, tag, p, None, 0.0)
    elif kind == "lure":
        box, a1, roi = gt_box + np.asarray([110, 20, 110, 20], np.float32) + _jit(seed, tag, 4.0), 9.0, (seed, tag, (p + 11) % 23, None, 0.0)
    elif kind == "off":
        box, a1, roi = np.asarray([40, 330, 160, 470], np.float32) + _jit(seed, tag, 4.0), 0.0, (seed, tag, p, None, 0.0)
    elif kind in ("other", "low"):
        box, a1, roi = FAR_BOX + _jit(seed, tag, 10.0), 9.0, (seed, tag, (p + 7) % 23, None, 0.0)
    else:
        raise KeyError(kind)
    return dict(score=np.float32(score), box=box.astype(np.float32), match=_desc(seed, "df2_" + tag, SPACING * a0, a1), roi=roi)


def _image(seed, p, img, rows, prod_row, dets, a0):
    """rows: [(style, pair_id)] of the image's garments (slot = row); prod_row: the row holding the product's garment (its box is
    what the detections are placed around); dets: [(kind, score)]."""
    gts = np.stack([_slot_box(p, img, s) for s in range(len(rows))]) if rows else np.zeros((0, 4), np.float32)
    out = []
    for d, (kind, score) in enumerate(dets):
        tag = f"p{p}_i{img}_d{d}"
        out.append(_det(seed, tag, kind, score, a0 + 0.002 * d, gts[prod_row] if rows else _slot_box(p, img, 0), p))
    return dict(gts=gts, styles=[r[0] for r in rows], pair_ids=[r[1] for r in rows], dets=out)


def _me(p):
    return (STYLE0 + p % 3, PAIR0 + p)


def _other(p, k):
    return (1 + (p + k) % 2, 500 + 7 * p + k)


def _sc(p, f, d=0):
    return 0.9 - 0.013 * f - 0.0007 * p - 0.21 * d


def scenario(name):
    """-> dict(products=[dict(key, images=[image...])], params, seed, name)"""
    prods = []
    if name == "A":       # IoU vs score, every-IoU-0 frames, the last-row rule, an empty street frame, drifts for every k threshold
        seed, g, t = 81, 34, 3
        drift = [0, 0, 1, 0, 2, 3, 0, 5, 1, 10, 0, 2, 4, 0, 9] + [0] * (g - 15)
        for p in range(g):
            me, slot = _me(p), p % 3
            rows = [_other(p, k) for k in range(3)]
            rows[slot] = me
            shop_rows = list(rows)
            if p in (5, 17):                             # the product is missing from the shop's list: -1 = the LAST row everywhere
                shop_rows[slot] = _other(p, 9)
            images = [_image(seed, p, 0, shop_rows, slot if p not in (5, 17) else 2, [("true", 0.95), ("other", 0.6)], float(p))]
            for f in range(t):
                a0 = p + drift[p] + _frac(p, f)
                dets = [("true", _sc(p, f)), ("dup", _sc(p, f, 1))]
                if p % 4 == 1:
                    dets.insert(0, ("lure", 0.98))       # most confident, low IoU: the IoU decides
                if p % 7 == 3 and f == 1:
                    dets = [("low", 0.05), ("off", 0.5), ("other", 0.8)]      # every IoU 0: the first kept one is taken
                if p == 6 and f == 2:
                    dets = [("low", 0.05), ("low", 0.02)]                      # nothing above the threshold: frame skipped
                images.append(_image(seed, p, 1 + f, shop_rows if p in (5, 17) else rows,
                                     slot if p not in (5, 17) else 2, dets, a0))
            prods.append(dict(key="%d_%d" % me, images=images))
        params = dict(score_threshold=0.1, frames_per_product=t, first_n_withvideo=None, use_gt=False)
    elif name == "B":     # a product skipped at its shop image, gallery-only products, use_gt, 8 street frames (chunks of 6)
        seed, g, t = 83, 26, 8
        for p in range(g):
            me, slot = _me(p), (p + 1) % 2
            rows = [_other(p, 0), _other(p, 1)]
            rows[slot] = me
            shop_dets = [("true", 0.92), ("dup", 0.4)]
            if p in (2, 9):
                shop_dets = [("true", 0.08), ("dup", 0.05)]                    # nothing kept: skipped, count_products still advances
            if p == 4:
                shop_dets = [("low", 0.05), ("dup", 0.7), ("true", 0.6)]       # kept position 1 read from the FULL list: the dup
            images = [_image(seed, p, 0, rows, slot, shop_dets, float(p))]
            for f in range(t):
                a0 = p + (p % 6) + 2.15 * (f % 4 == 0 and p % 6 > 0) + _frac(p, f)
                dets = [("dup", _sc(p, f, 1)), ("true", _sc(p, f))]
                if f == 4 and p % 3 == 0:
                    dets.append(("lure", 0.99))
                images.append(_image(seed, p, 1 + f, rows, slot, dets, a0))
            prods.append(dict(key="%d_%d" % me, images=images))
        params = dict(score_threshold=0.1, frames_per_product=t, first_n_withvideo=17, use_gt=True)
    elif name == "C":     # threshold 0.5; street frames with fewer GT rows than the shop's product row (-> last row)
        seed, g, t = 87, 22, 4
        for p in range(g):
            me = _me(p)
            shop_rows = [_other(p, 0), _other(p, 1), me] if p % 2 else [me, _other(p, 1)]
            prow = len(shop_rows) - 1 if p % 2 else 0
            images = [_image(seed, p, 0, shop_rows, prow, [("other", 0.7), ("true", 0.9), ("low", 0.3)], float(p))]
            for f in range(t):
                a0 = p + ((p * 3) % 7) + _frac(p, f)
                if p % 2 and f % 2:
                    rows, r = [_other(p, 3), me], 1                           # shop row 2 >= 2 GT rows: -1 -> the last row (here: me)
                elif p % 2:
                    rows, r = [me, _other(p, 4), _other(p, 5)], 0              # shop row 2 is another garment here: the scan stops
                else:                                                          # at row 2 without a match -> -1 -> row 2
                    rows, r = [me, _other(p, 6)], 0
                dets = [("lure", 0.97), ("true", _sc(p, f)), ("low", 0.45), ("dup", 0.55)]
                if p % 2 and not f % 2:
                    dets = [("true", 0.8), ("other", 0.6), ("dup", 0.51)]    # the product sits in row 0, the scan picks row 2
                images.append(_image(seed, p, 1 + f, rows, r, dets, a0))
            prods.append(dict(key="%d_%d" % me, images=images))
        params = dict(score_threshold=0.5, frames_per_product=t, first_n_withvideo=None, use_gt=False)
    else:
        raise KeyError(name)
    return dict(products=prods, params=params, seed=seed, name=name)


NAMES = ("A", "B", "C")


def build(name, device="cpu"):
    """-> (loader, canned, params); loader[i] = (images, targets, ids); images are 1-element tensors holding the image id that
    ``canned[id]`` (a dict of torch tensors on `device`) answers for."""
    sc = scenario(name)
    w, b = classifier(sc["seed"])
    loader, canned, nxt = [], {}, 0
    for p in sc["products"]:
        images, targets, ids = [], [], []
        for img in p["images"]:
            dets = img["dets"]
            images.append(torch.tensor([float(nxt)]))
            canned[nxt] = dict(
                scores=torch.from_numpy(np.asarray([d["score"] for d in dets], np.float32)).to(device),
                boxes=torch.from_numpy(np.stack([d["box"] for d in dets])).to(device),
                labels=torch.ones(len(dets), dtype=torch.int64, device=device),
                match_features=torch.from_numpy(np.stack([d["match"] for d in dets])).to(device),
                roi_features=torch.from_numpy(np.stack([_roi(*d["roi"]) for d in dets])).to(device),
                w=torch.from_numpy(w).to(device), b=torch.from_numpy(b).to(device))
            targets.append(dict(boxes=torch.from_numpy(img["gts"].copy()), styles=torch.tensor(img["styles"], dtype=torch.int64),
                                pair_ids=torch.tensor(img["pair_ids"], dtype=torch.int64), i=p["key"]))
            ids.append(nxt)
            nxt += 1
        loader.append((images, targets, ids))
    return loader, canned, sc["params"]


def loader_digest(loader, canned) -> str:
    """sha256 over everything the evaluator reads (targets and canned outputs, in loader order)."""
    import hashlib
    h = hashlib.sha256()
    for images, targets, _ in loader:
        for im, t in zip(images, targets):
            c = canned[int(round(float(im.reshape(-1)[0])))]
            for k in ("scores", "boxes", "match_features", "roi_features", "w", "b"):
                h.update(np.ascontiguousarray(c[k].detach().cpu().numpy()).tobytes())
            for k in ("boxes", "styles", "pair_ids"):
                h.update(np.ascontiguousarray(t[k].numpy()).tobytes())
            h.update(t["i"].encode())
    return h.hexdigest()


class CannedModel(ES.CannedModel):
    """``model(images, targets=None)`` returns the canned dicts and records the chunk sizes and whether targets came along."""

    def __init__(self, canned, temporal_aggregator):
        super().__init__(canned, temporal_aggregator)
        self.calls = []

    def __call__(self, images, targets=None):
        self.calls.append((len(images), targets is not None and len(targets) == len(images)))
        return super().__call__(images, targets)
