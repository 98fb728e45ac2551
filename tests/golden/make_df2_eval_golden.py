#!/usr/bin/env python3
"""Golden vectors of the Multi-DeepFashion2 evaluator, captured by running the reference's own ``evaluate()``
(evaluate_multiDF2.py:16-327 of the reference checkout) on the canned-detector scenarios of tests/eval_df2_scenarios.py.

Run:  python tests/golden/make_df2_eval_golden.py [REFERENCE_DIR]        (default ../reference next to the repository)

``evaluate_multiDF2`` imports pycocotools, the DF2 dataset module, the detector and the transforms at module level; ``evaluate()``
itself uses exactly one symbol of them, ``pycocotools.mask.iou`` (:54,87).  So the modules it never touches are empty stand-ins in
``sys.modules``, and ``pycocotools.mask.iou`` is given the public definition of pycocotools' ``bbIou`` (maskApi.c: xywh boxes in
double, intersection / (area_dt + area_gt - intersection), 0 where the overlap is empty; iscrowd 0) [COCO].  ``models.match_head``
and ``models.nlb`` are the REAL reference modules, so ``model.roi_heads.temporal_aggregator`` is the reference's
``TemporalAggregationNLB`` with the repository's synthetic weights.  ``evaluate()`` runs in a temporary working directory (it
writes ``accs_per_product_10frame_df2.pth`` and ``logs_mdf2/*.csv``).

What is stored (outputs only): per scenario what it printed, the CSV it wrote, the per-product dict, ``ret``, and -- read out of
the frame with ``sys.setprofile`` -- the seven hit-counter vectors, ``all_ranks_list``, ``count_street`` / ``count_products`` /
``total_querys``, the shop bookkeeping (product index, key, the chosen ``maxind`` at the aggregator call) and the street
bookkeeping (product, frame, chosen ``maxind``, score), plus the sha256 of the loader it ran on.

Before a scenario is accepted it must be DECIDED: every score the true product's score is compared with (per-frame, average
descriptor, aggregated descriptor, average / maximum distance) differs from it by more than 0.5 % relative (10 half-ulps of fp16),
and no true product's score is below 1e-6 -- the rule of make_eval_golden.py, restated here in float64 NumPy -- so that the
reference's fp16 tables and fp32 tables cannot rank differently.
"""
import contextlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import eval_df2_scenarios as DS                     # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else os.path.join(os.path.dirname(ROOT), "reference")


def bb_iou(dt, gt, iscrowd):
    """pycocotools.mask.iou on xywh boxes (maskApi.c bbIou) [COCO, public definition]: o[d, g] for dt[d], gt[g]."""
    dt, gt = np.asarray(dt, np.float64), np.asarray(gt, np.float64)
    m, n = len(dt), len(gt)
    if m == 0 or n == 0:
        return []
    assert len(iscrowd) == n
    o = np.zeros((m, n))
    for g in range(n):
        G = gt[g]
        ga = G[2] * G[3]
        for d in range(m):
            D = dt[d]
            da = D[2] * D[3]
            w = min(D[2] + D[0], G[2] + G[0]) - max(D[0], G[0])
            if w <= 0:
                continue
            h = min(D[3] + D[1], G[3] + G[1]) - max(D[1], G[1])
            if h <= 0:
                continue
            i = w * h
            o[d, g] = i / (da if iscrowd[g] else da + ga - i)
    return o


def import_reference_evaluate():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    pm = mod("pycocotools.mask", iou=bb_iou)
    mod("pycocotools", mask=pm)
    sys.path.insert(0, REF)
    import models                                   # noqa: F401  (the real package: match_head, nlb)
    # the three imports below serve only the script's __main__ section; evaluate() never touches them
    mod("datasets.MultiDF2Dataset", MultiDeepFashion2Dataset=None, get_dataloader=None)
    mod("datasets", MultiDF2Dataset=sys.modules["datasets.MultiDF2Dataset"])
    mod("models.video_matchrcnn", videomatchrcnn_resnet50_fpn=None)
    mod("stuffs.transform")
    mod("stuffs", transform=sys.modules["stuffs.transform"])
    import evaluate_multiDF2 as EM
    from models.match_head import TemporalAggregationNLB
    return EM, TemporalAggregationNLB


COUNTERS = ["k_accs", "k_accs_avg", "k_accs_avg_desc", "k_accs_aggr_desc", "k_accs_avg_dist", "k_accs_max_dist", "k_accs_max_score"]
SCALARS = ["count_street", "count_products", "total_querys"]
PER_PRODUCT = ("sfmr", "seamrcnn", "bmfm", "avgdist", "maxdist", "maxscore")


def _find_evaluate(frame):
    while frame is not None:
        if frame.f_code.co_name == "evaluate" and frame.f_code.co_filename.endswith("evaluate_multiDF2.py"):
            return frame
        frame = frame.f_back
    return None


def run_reference(EM, agg, name):
    loader, canned, params = DS.build(name)
    digest = DS.loader_digest(loader, canned)       # before the run: on the CPU the reference turns the GT boxes into xywh in place
    model = DS.CannedModel(canned, agg)
    grabbed, shop_calls = {}, []

    def prof(frame, event, arg):
        if frame.f_code.co_name == "forward" and event == "call" and frame.f_code.co_filename.endswith("match_head.py"):
            types_ = frame.f_locals.get("types")
            ev = _find_evaluate(frame.f_back)
            if ev is not None and types_ is not None and int(types_[0]) == 1:       # the shop descriptor call (:61-63)
                shop_calls.append((int(ev.f_locals["count_products"]) - 1, int(ev.f_locals["maxind"])))
        if event == "return" and frame.f_code.co_name == "evaluate" and frame.f_code.co_filename.endswith("evaluate_multiDF2.py"):
            grabbed.update(frame.f_locals)

    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        os.chdir(tmp)
        try:
            sys.setprofile(prof)
            with contextlib.redirect_stdout(io.StringIO()) as out, contextlib.redirect_stderr(io.StringIO()), np.errstate(all="ignore"):
                ret = EM.evaluate(model, loader, torch.device("cpu"), **params)
        finally:
            sys.setprofile(None)
            os.chdir(cwd)
        per_product = torch.load(os.path.join(tmp, "accs_per_product_10frame_df2.pth"), weights_only=False)
        csvs = sorted(os.listdir(os.path.join(tmp, "logs_mdf2")))
        csv_text = open(os.path.join(tmp, "logs_mdf2", csvs[0])).read()
    g = {"ret": np.asarray(ret, np.float64), "perf_csv": np.asarray(csv_text), "stdout": np.asarray(out.getvalue()),
         "loader_sha256": np.asarray(digest)}
    for k in COUNTERS:
        g[k] = np.asarray(grabbed[k], np.int64)
    for k in SCALARS:
        g[k] = np.asarray(int(grabbed[k]), np.int64)
    g["all_ranks_list"] = np.asarray(grabbed["all_ranks_list"], np.int64).reshape(-1)
    g["shop_prods"] = np.asarray(grabbed["shop_prods"], np.int64)
    g["shop_keys"] = np.asarray([str(x) for x in grabbed["shop_datais"]])
    assert [p for p, _ in shop_calls] == g["shop_prods"].tolist()
    g["shop_maxind"] = np.asarray([m for _, m in shop_calls], np.int64)
    sd = grabbed["street_descrs"]
    g["street_prods"] = np.asarray([x[1] for x in sd], np.int64)
    g["street_imgs"] = np.asarray([x[2] for x in sd], np.int64)
    g["street_maxind"] = np.asarray([x[3] for x in sd], np.int64)
    g["street_scores"] = np.asarray([x[4] for x in sd], np.float64)
    keys = list(per_product)
    g["per_product_keys"] = np.asarray([str(k) for k in keys])
    for f in PER_PRODUCT:
        g["per_product_" + f] = np.stack([np.asarray(per_product[k][f], np.float64) for k in keys])
    return g, grabbed, params


def _scores(q, gal, w, b):
    """softmax((gal - q)^2 @ w.T + b)[..., 1] in float64, q [Q,D] -> [Q,G]."""
    raw = ((gal[None] - q[:, None]) ** 2) @ w.T + b
    raw = raw - raw.max(-1, keepdims=True)
    e = np.exp(raw)
    return e[..., 1] / e.sum(-1)


def margins(grabbed, agg):
    """(kind, relative gap of the true product's score to the nearest other score) for every ranking the reference decides, plus
    ("true_score", s)."""
    out = []

    def log(kind, row, t):
        gap = np.abs(np.delete(row, t) - row[t]).min()
        out.append((kind, float(gap / max(abs(row[t]), 1e-30))))
        out.append(("true_score", float(row[t])))

    f64 = lambda a: np.asarray(a, np.float64)              # noqa: E731
    shop, street = f64(grabbed["shop_mat"]), f64(grabbed["street_mat"])
    w, b = f64(grabbed["w"]), f64(grabbed["b"])
    aw, ab = f64(grabbed["aggrW"]), f64(grabbed["aggrB"])
    shop_aggr = f64(grabbed["shop_aggregated_descrs"]).reshape(len(shop), -1)
    street_aggr = np.asarray(grabbed["street_aggr_feats"], np.float32)
    shop_prods, street_prods = np.asarray(grabbed["shop_prods"]), np.asarray(grabbed["street_prods"])
    for p in range(int(grabbed["count_street"])):
        if p not in shop_prods:
            continue
        t = int(np.flatnonzero(shop_prods == p)[0])
        inds = np.flatnonzero(street_prods == p)
        dist = _scores(street[inds], shop, w, b)
        for row in dist:
            log("frame", row, t)
        log("avg_desc", _scores(street[inds].mean(0)[None], shop, w, b)[0], t)
        log("avg_dist", dist.mean(0), t)
        log("max_dist", dist.max(0), t)
        seq = torch.zeros((1 + len(inds), 1, street_aggr.shape[1]))
        seq[1:, 0] = torch.from_numpy(street_aggr[inds])
        with torch.no_grad():
            desc = agg(None, None, None, x3_1_seq=seq, x3_1_mask=torch.zeros((1, 1 + len(inds)), dtype=torch.bool),
                       x3_2=torch.from_numpy(shop_aggr[t].astype(np.float32)))[0][0].numpy()
        log("aggr_desc", _scores(f64(desc)[None], shop_aggr, aw, ab)[0], t)
    return out


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps (numpy stamps every member with the current time), so that a second run
    writes the same bytes."""
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    torch.set_grad_enabled(False)
    torch.set_num_threads(8)
    EM, TA = import_reference_evaluate()
    agg = TA().eval()
    agg.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in DS.aggregator_state().items()})
    store = {}
    for name in DS.NAMES:
        g, grabbed, params = run_reference(EM, agg, name)
        m = margins(grabbed, agg)
        least_score = min(v for k, v in m if k == "true_score")
        m = [(k, v) for k, v in m if k != "true_score"]
        worst = min(v for _, v in m)
        print(f"scenario {name}: ret = {g['ret']}, count_street {int(g['count_street'])} of {int(g['count_products'])} products, "
              f"frame ranks {g['all_ranks_list'].tolist()}")
        print("  " + "  ".join(f"{k} {g[k].tolist()}" for k in COUNTERS))
        print(f"  least decided comparison: {worst:.4f} relative ({len(m)} rankings; kinds: "
              f"{ {k: round(min(v for kk, v in m if kk == k), 4) for k in sorted(set(k for k, _ in m))} })")
        print(f"  smallest score of a true product: {least_score:.3e}")
        assert worst > 5e-3, f"scenario {name} is not decided under fp16: least margin {worst}"
        assert least_score > 1e-6, f"scenario {name}: a true product's score ({least_score}) is not representable in fp16"
        for k, v in g.items():
            store[f"{name}_{k}"] = v
    path = os.path.join(HERE, "eval_df2_golden.npz")
    save_npz(path, store)
    print("wrote", path, f"{os.path.getsize(path)} bytes, {len(store)} arrays")


if __name__ == "__main__":
    main()
