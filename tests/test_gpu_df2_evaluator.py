"""Multi-DeepFashion2 evaluator on the device: the drop-in ``evaluate`` against the reference's own run
(tests/golden/eval_df2_golden.npz), seam_gt_select_f32 against a float64 NumPy restatement of pycocotools' bbIou + np.argmax, and a
small run of the real model."""
import contextlib
import io
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import ROOT, to_torch

pytestmark = pytest.mark.gpu

COUNTS = {"frame": "k_accs", "max_per_image": "k_accs_avg", "avg_desc": "k_accs_avg_desc", "aggr_desc": "k_accs_aggr_desc",
          "avg_dist": "k_accs_avg_dist", "max_dist": "k_accs_max_dist", "max_score": "k_accs_max_score"}
PER_PRODUCT = ("sfmr", "seamrcnn", "bmfm", "avgdist", "maxdist", "maxscore")


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def df2_golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "eval_df2_golden.npz")))


def _aggregator():
    import eval_df2_scenarios as DS
    from seam_match_rcnn_amd.models.match_head import TemporalAggregationNLB
    ta = TemporalAggregationNLB()
    ta.load_state_dict(to_torch(DS.aggregator_state()))
    return ta.to(dev()).eval()


def _run(name, strategy="best_match"):
    import eval_df2_scenarios as DS
    from seam_match_rcnn_amd import evaluator_df2 as EV
    loader, canned, params = DS.build(name, device=dev())
    model = DS.CannedModel(canned, _aggregator())
    buf = io.StringIO()
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(buf):
        ret, rep = EV.evaluate(model, loader, dev(), strategy=strategy, return_report=True, artifacts_dir=tmp, **params)
        saved = torch.load(os.path.join(tmp, "accs_per_product_10frame_df2.pth"), weights_only=False)
        csv = open(os.path.join(tmp, "logs_mdf2", os.listdir(os.path.join(tmp, "logs_mdf2"))[0])).read()
    return ret, rep, buf.getvalue(), csv, saved, model, params


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_device_evaluate_matches_reference_evaluate(name, df2_golden):
    """The drop-in evaluate() reproduces the reference's own run: printed tables and CSV verbatim, the seven counter vectors, every
    per-frame rank, count_street, ret, the per-product dict, and the detection chosen in every shop image and street frame."""
    g = df2_golden
    ret, rep, out, csv, saved, model, params = _run(name)
    assert out == str(g[f"{name}_stdout"])
    assert csv == str(g[f"{name}_perf_csv"])
    for ours, ref in COUNTS.items():
        np.testing.assert_array_equal(rep.counts[ours], g[f"{name}_{ref}"], err_msg=f"{name}: {ours}")
    assert rep.frame_ranks == g[f"{name}_all_ranks_list"].tolist()
    t = rep.tables
    assert t.count_street == int(g[f"{name}_count_street"]) and t.count_products == int(g[f"{name}_count_products"])
    np.testing.assert_allclose(ret, g[f"{name}_ret"], rtol=0, atol=1e-12)
    for got in (saved, rep.per_product):
        assert [str(k) for k in got] == g[f"{name}_per_product_keys"].tolist()
        for f in PER_PRODUCT:
            np.testing.assert_allclose(np.stack([v[f] for v in got.values()]), g[f"{name}_per_product_{f}"], rtol=0, atol=1e-12)
    assert t.shop_prods.tolist() == g[f"{name}_shop_prods"].tolist()
    assert [str(k) for k in t.shop_keys] == g[f"{name}_shop_keys"].tolist()
    assert t.shop_sel.tolist() == g[f"{name}_shop_maxind"].tolist()
    assert t.street_prods.tolist() == g[f"{name}_street_prods"].tolist()
    assert t.street_imgs.tolist() == g[f"{name}_street_imgs"].tolist()
    assert t.street_sel.tolist() == g[f"{name}_street_maxind"].tolist()
    np.testing.assert_array_equal(t.street_scores.astype(np.float64), g[f"{name}_street_scores"])
    # chunks of 6 images per model call; with use_gt the (copied) targets travel along
    n_img = [len(images) for images, _, _ in loader_of(name)]
    assert [c for c, _ in model.calls] == [min(6, n - x) for n in n_img for x in range(0, n, 6)]
    assert all(has == params["use_gt"] for _, has in model.calls)


def loader_of(name):
    import eval_df2_scenarios as DS
    return DS.build(name)[0]


@pytest.mark.parametrize("name", ["A", "B"])
def test_best_box_only_gives_the_same_report(name):
    ret_a, rep_a, out_a, csv_a, _, _, _ = _run(name, "best_match")
    ret_b, rep_b, out_b, csv_b, _, _, _ = _run(name, "best_box_only")
    assert out_a == out_b and csv_a == csv_b and ret_a == ret_b
    assert rep_a.frame_ranks == rep_b.frame_ranks
    for k in rep_a.counts:
        np.testing.assert_array_equal(rep_a.counts[k], rep_b.counts[k])


# ---- seam_gt_select_f32 against NumPy ----------------------------------------------------------------------------------------

def _xywh(b):
    b = np.asarray(b, np.float32).reshape(-1, 4).copy()
    b[:, 2] = b[:, 2] - b[:, 0]                  # fp32, as the reference does it in NumPy
    b[:, 3] = b[:, 3] - b[:, 1]
    return b.astype(np.float64)


def bb_iou_row(gt, dets):
    """pycocotools bbIou of one GT box against every detection, float64 (iscrowd 0)."""
    G, D = _xywh(gt)[0], _xywh(dets)
    w = np.fmin(G[2] + G[0], D[:, 2] + D[:, 0]) - np.fmax(G[0], D[:, 0])
    h = np.fmin(G[3] + G[1], D[:, 3] + D[:, 1]) - np.fmax(G[1], D[:, 1])
    inter = w * h
    with np.errstate(all="ignore"):
        iou = inter / ((G[2] * G[3] + D[:, 2] * D[:, 3]) - inter)
    return np.where((w <= 0) | ((w > 0) & (h <= 0)), 0.0, iou)


def ref_select(boxes, scores, det_off, gts, gt_off, rows, thr):
    n = len(rows)
    out = np.zeros((3, n), np.int64)
    for i in range(n):
        d0, d1, g0, g1 = det_off[i], det_off[i + 1], gt_off[i], gt_off[i + 1]
        kept = np.flatnonzero(scores[d0:d1] >= np.float32(thr))
        ng, r = g1 - g0, int(rows[i])
        if r < 0:
            r += ng
        if kept.size == 0:
            out[:, i] = (-1, -1, 0)
        elif ng == 0:
            out[:, i] = (-1, -1, 1)
        elif not 0 <= r < ng:
            out[:, i] = (-1, -1, 2)
        else:
            iou = bb_iou_row(gts[g0 + r], boxes[d0:d1][kept])
            pos = int(np.argmax(iou))
            out[:, i] = (kept[pos], pos, 0)
    return out


def _device_select(boxes, scores, det_off, gts, gt_off, rows, thr):
    from seam_match_rcnn_amd import ops
    d = dev()
    sel = ops.gt_select(torch.from_numpy(boxes).to(d), torch.from_numpy(scores).to(d), det_off, torch.from_numpy(gts).to(d), gt_off,
                        torch.from_numpy(np.asarray(rows, np.int32)).to(d), thr)
    return torch.stack(sel).cpu().numpy().astype(np.int64)


def _random_batch(rng, n, max_det, big_every=0):
    counts, gcounts, boxes, scores, gts, rows = [], [], [], [], [], []
    for i in range(n):
        k = int(rng.integers(0, max_det + 1))
        if big_every and i % big_every == 0:
            k = int(rng.integers(100, 180))
        if i % 11 == 5:
            k = 0                                                          # no detection at all
        ng = int(rng.integers(1, 5)) if i % 13 != 7 else 0
        xy = rng.uniform(0, 400, (k, 2))
        wh = rng.uniform(5, 200, (k, 2))
        b = np.concatenate([xy, xy + wh], 1)
        if k > 2 and i % 9 == 4:
            b[1] = b[1][[2, 3, 0, 1]]                                      # a negative-extent box, not clamped
        s = rng.uniform(0, 1, k)
        if i % 7 == 2:
            s *= 0.1                                                       # everything below the threshold
        gxy = rng.uniform(0, 400, (ng, 2))
        g = np.concatenate([gxy, gxy + rng.uniform(20, 250, (ng, 2))], 1)
        r = int(rng.integers(-1, ng)) if ng else -1
        if i % 17 == 3:
            r = ng                                                         # out of range (past the end)
        if i % 17 == 8:
            r = -ng - 1                                                    # out of range (before the start)
        counts.append(k), gcounts.append(ng), boxes.append(b), scores.append(s), gts.append(g), rows.append(r)
    det_off = np.cumsum([0] + counts)
    gt_off = np.cumsum([0] + gcounts)
    return (np.concatenate(boxes).astype(np.float32).reshape(-1, 4), np.concatenate(scores).astype(np.float32), det_off,
            np.concatenate(gts).astype(np.float32).reshape(-1, 4), gt_off, np.asarray(rows, np.int32))


@pytest.mark.parametrize("n,max_det,big_every,seed", [(300, 40, 10, 1), (4096, 24, 97, 2)])
def test_gt_select_matches_numpy(n, max_det, big_every, seed):
    """Ragged batches: empty images, images with nothing above the threshold, 100+ detections, images without GT boxes,
    out-of-range rows, negative-extent boxes; the 4096-image batch is the at-scale case."""
    rng = np.random.default_rng(seed)
    batch = _random_batch(rng, n, max_det, big_every)
    for thr in (0.1, 0.7):
        want = ref_select(*batch, thr)
        got = _device_select(*batch, thr)
        np.testing.assert_array_equal(got, want)
        assert (want[2] == 1).any() and (want[2] == 2).any() and (want[0] == -1).any() and (want[1] > 0).any()


def test_gt_select_near_ties_follow_float64():
    """Detections one fp32 ulp apart around the GT box: their IoUs differ in float64 but many collapse (or reorder) in fp32.  The
    kernel must take float64's first maximum, not fp32's."""
    rng = np.random.default_rng(7)
    n, k = 64, 160
    boxes, gts, differs = [], [], 0
    for i in range(n):
        g = np.asarray([300.0 + i, 200.0, 700.0 + i, 650.0], np.float32)
        steps = rng.integers(-3, 4, (k, 4)).astype(np.float32)
        b = g + steps * np.spacing(g)
        iou64 = bb_iou_row(g, b)
        gf, bf = _xywh(g).astype(np.float32)[0], _xywh(b).astype(np.float32)
        w32 = np.fmin(gf[2] + gf[0], bf[:, 2] + bf[:, 0]) - np.fmax(gf[0], bf[:, 0])
        h32 = np.fmin(gf[3] + gf[1], bf[:, 3] + bf[:, 1]) - np.fmax(gf[1], bf[:, 1])
        i32 = w32 * h32
        iou32 = i32 / ((gf[2] * gf[3] + bf[:, 2] * bf[:, 3]) - i32)
        differs += int(np.argmax(iou32) != np.argmax(iou64))
        boxes.append(b), gts.append(g)
    assert differs > 0                                  # the construction does produce fp32 / fp64 disagreements
    batch = (np.concatenate(boxes), np.full(n * k, 0.9, np.float32), np.arange(n + 1) * k, np.stack(gts), np.arange(n + 1),
             np.zeros(n, np.int32))
    np.testing.assert_array_equal(_device_select(*batch, 0.1), ref_select(*batch, 0.1))


def test_gt_select_exact_ties_take_the_first():
    g = np.asarray([[100, 100, 300, 300]], np.float32)
    dup = np.asarray([120, 110, 310, 290], np.float32)
    far = np.asarray([500, 500, 600, 600], np.float32)
    # image 0: the same box at kept positions 1, 3 and across the 64-lane stride (70, 130); image 1: every IoU 0 -> first kept;
    # image 2: a mirrored pair with identical IoU
    b0 = np.tile(far, (140, 1))
    b0[[3, 10, 70, 130]] = dup
    s0 = np.full(140, 0.9, np.float32)
    s0[[0, 1, 2]] = [0.05, 0.9, 0.01]                  # kept subsequence starts at index 1
    b1 = np.tile(far, (5, 1))
    s1 = np.asarray([0.0, 0.2, 0.9, 0.3, 0.8], np.float32)
    b2 = np.asarray([[100, 100, 200, 300], [200, 100, 300, 300], [150, 100, 250, 300]], np.float32)
    s2 = np.asarray([0.5, 0.5, 0.5], np.float32)
    b2[2] = far
    batch = (np.concatenate([b0, b1, b2]), np.concatenate([s0, s1, s2]), np.asarray([0, 140, 145, 148]), np.concatenate([g, g, g]),
             np.asarray([0, 1, 2, 3]), np.zeros(3, np.int32))
    got = _device_select(*batch, 0.1)
    np.testing.assert_array_equal(got, ref_select(*batch, 0.1))
    assert got[:, 0].tolist() == [3, 1, 0] and got[:, 1].tolist() == [1, 0, 0] and got[:, 2].tolist() == [0, 0, 0]


def test_gt_select_rejects_offsets_outside_the_tables():
    from seam_match_rcnn_amd import ops
    d = dev()
    b = torch.zeros((3, 4), device=d)
    s = torch.ones(3, device=d)
    r = torch.zeros(1, dtype=torch.int32, device=d)
    for det_off, gt_off in (([0, 4], [0, 3]), ([0, 3], [0, 4]), ([1, 3], [0, 3]), ([0, 3, 3], [0, 3])):
        with pytest.raises(ValueError):
            ops.gt_select(b, s, det_off, b, gt_off, r, 0.1)


# ---- the real model ------------------------------------------------------------------------------------------------------------

class _Recorder:
    """The real model, with every image's output kept for the comparison."""

    def __init__(self, model):
        self.model, self.roi_heads, self.outputs = model, model.roi_heads, []

    def __call__(self, images, targets=None):
        out = self.model(images, targets=targets)
        self.outputs += out
        return out


def test_real_model_small_run():
    """Synthetic videomatchrcnn_resnet50_fpn weights, 128x160 frames, 3 products of a shop image + 2 street frames: the evaluator
    finishes, and the collected shop / street descriptors are the model's own match_features rows at the detections the
    NumPy restatement of the selection picks."""
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd import evaluator_df2 as EV
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    model = videomatchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    model.load_state_dict(to_torch(synth.video_matchrcnn_state(5)))
    model = model.to(dev()).eval()
    model.transform.min_size, model.transform.max_size = 128, 160
    loader = []
    for p in range(3):
        imgs = [torch.from_numpy(synth.frames(40 + 3 * p + f, 1, 128, 160)[0]) for f in range(3)]
        tg = [dict(boxes=torch.tensor([[10.0 + 5 * f, 12.0, 90.0 + 7 * p, 110.0], [60.0, 30.0, 150.0, 120.0]]),
                   styles=torch.tensor([1, 2]), pair_ids=torch.tensor([7 + p, 50]), i=f"1_{7 + p}") for f in range(3)]
        loader.append((imgs, tg, list(range(3))))
    rec = _Recorder(model)
    with contextlib.redirect_stdout(io.StringIO()):
        ret, rep = EV.evaluate(rec, loader, dev(), score_threshold=0.0, frames_per_product=2, return_report=True)
    assert len(ret) == 3 and all(np.isfinite(ret))
    t = rep.tables
    outs = rec.outputs
    assert len(outs) == 9
    for i, p in enumerate(t.shop_prods.tolist()):
        o = outs[3 * p]
        torch.testing.assert_close(t.shop_mat[i], o["match_features"][int(t.shop_sel[i])], rtol=0, atol=0)
    for j, (p, f) in enumerate(zip(t.street_prods.tolist(), t.street_imgs.tolist())):
        o = outs[3 * p + 1 + f]
        torch.testing.assert_close(t.street_mat[j], o["match_features"][int(t.street_sel[j])], rtol=0, atol=0)
    # the choices are the restatement's: all kept (threshold 0), the product's GT row is row 0
    for n, o in enumerate(outs):
        b, s = o["boxes"].float().cpu().numpy(), o["scores"].float().cpu().numpy()
        want = ref_select(b, s, np.asarray([0, len(s)]), loader[n // 3][1][n % 3]["boxes"].numpy(), np.asarray([0, 2]),
                          np.zeros(1, np.int32), 0.0)
        if n % 3 == 0 and n // 3 in t.shop_prods.tolist():
            assert int(t.shop_sel[t.shop_prods.tolist().index(n // 3)]) == int(want[1, 0])
        elif n % 3:
            hit = [j for j, (p, f) in enumerate(zip(t.street_prods, t.street_imgs)) if p == n // 3 and f == n % 3 - 1]
            if hit:
                assert int(t.street_sel[hit[0]]) == int(want[0, 0])
