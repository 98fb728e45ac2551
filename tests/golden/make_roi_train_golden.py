#!/usr/bin/env python3
"""Golden vectors of the RoI heads' match branch, captured by running the reference's own ``filter_proposals`` and
``MatchLossPreTrained`` (models/match_head.py:441-504 of the reference checkout) on the seeded cases of
``tests/roi_train_refs.golden_cases``.

Run:  python tests/golden/make_roi_train_golden.py [REFERENCE_DIR]        (default ../reference next to the repository)

``models/match_head.py`` imports ``pycocotools.mask`` at module level and uses one symbol of it, ``iou``; it is given the
public definition of pycocotools' ``bbIou`` (maskApi.c: boxes read as xywh, double, intersection / union, 0 where the
overlap is empty; iscrowd 0) [COCO], as make_df2_eval_golden.py does.  The reference module and its ``nlb`` import are
the real ones.

What is stored (outputs only), per case c and image i: ``c/rows_i`` the kept row indices, ``c/matched_i`` the kept
matched GT indices, ``c/types`` the types built like the reference (:428-433), ``c/logits`` the logits the loss was given
(seeded), ``c/loss`` its value and ``c/dlogits`` its gradient.
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import roi_train_refs as RR                           # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")


def import_reference():
    pm = types.ModuleType("pycocotools.mask")
    pm.iou = lambda dt, gt, iscrowd: RR.bb_iou_xywh(dt, gt) if len(dt) and len(gt) else []
    pc = types.ModuleType("pycocotools")
    pc.mask = pm
    sys.modules["pycocotools"], sys.modules["pycocotools.mask"] = pc, pm
    sys.path.insert(0, REF)
    from models.match_head import MatchLossPreTrained, filter_proposals
    return filter_proposals, MatchLossPreTrained


def main():
    filter_proposals, MatchLossPreTrained = import_reference()
    out = {}
    for name, imgs in RR.golden_cases():
        props = [torch.from_numpy(im["props"]) for im in imgs]
        gts = [torch.from_numpy(im["gt"]) for im in imgs]
        mids = [torch.from_numpy(im["matched"]) for im in imgs]
        # row identity rides along as the "features": feature row j of image i holds its global row number
        counts = [len(p) for p in props]
        feats = torch.arange(sum(counts), dtype=torch.float32)[:, None]
        kept_p, kept_f, kept_m = filter_proposals(list(props), feats, gts, list(mids))
        off = np.cumsum([0] + counts[:-1])
        tys = []
        for i, (p, im) in enumerate(zip(kept_p, imgs)):
            tys += [1] * len(p) if im["sources"][0] == 1 else [0] * len(p)
        tys = torch.IntTensor(tys)
        rows = kept_f[:, 0].to(torch.int64).numpy()
        start = 0
        for i, p in enumerate(kept_p):
            out[f"{name}/rows_{i}"] = rows[start:start + len(p)] - off[i]
            out[f"{name}/matched_{i}"] = kept_m[i].numpy()
            start += len(p)
        g = torch.Generator().manual_seed(7)
        ns, nh = int((tys == 0).sum()), int((tys == 1).sum())
        logits = (torch.randn((ns, nh, 2), generator=g) * (6.0 if name == "three_gt" else 2.0)).requires_grad_(True)   # three_gt: loss > 1, halved
        loss = MatchLossPreTrained()(logits, kept_p, gts, [torch.from_numpy(im["pair_ids"]) for im in imgs],
                                     [torch.from_numpy(im["styles"]) for im in imgs], tys, kept_m)
        if logits.numel():
            loss.backward()
            dl = logits.grad.numpy()
        else:
            dl = np.zeros(logits.shape, np.float32)
        out[f"{name}/types"] = tys.numpy().astype(np.int64)
        out[f"{name}/logits"] = logits.detach().numpy()
        out[f"{name}/loss"] = np.asarray(float(loss.detach()), np.float64)
        out[f"{name}/dlogits"] = dl
    np.savez_compressed(os.path.join(HERE, "roi_train_golden.npz"), **out)
    print("wrote", len(out), "arrays")


if __name__ == "__main__":
    main()
