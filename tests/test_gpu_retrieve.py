"""retrieval.build_bank / retrieve on the model and loader of test_evaluate_end_to_end_drop_in_model (synthetic weights, three
products of one shop image and three frames, all 128 x 160) against the evaluator's own pieces on the same data."""
import numpy as np
import pytest
import torch

import seam_match_rcnn_amd.synth as synth
from conftest import to_torch

pytestmark = pytest.mark.gpu

K = 3       # == the bank's size: every rank is below k


class World:
    pass


@pytest.fixture(scope="module")
def world():
    from seam_match_rcnn_amd import evaluator as EV
    from seam_match_rcnn_amd import retrieval as R
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    w = World()
    w.dev = torch.device("cuda:0")
    m = videomatchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    m.load_state_dict(to_torch(synth.video_matchrcnn_state(5)))
    w.model = m = m.to(w.dev).eval()
    m.transform.min_size, m.transform.max_size = 128, 160
    w.loader = []
    for p in range(3):
        images = [torch.from_numpy(synth.frames(50 + 4 * p + i, 1, 128, 160)[0]) for i in range(4)]
        targets = [dict(source=1 + (p % 2), i=100 + p)] + [dict(tracklet=[10. + 5 * i, 12., 90. + 5 * i, 100.]) for i in range(3)]
        w.loader.append((images, targets))
    w.tables = EV.collect_descriptors(m, w.loader, w.dev, score_threshold=0.0)
    w.bank = R.build_bank(m, [im[0] for im, _ in w.loader], keys=[100, 101, 102])
    w.clips = [im[1:] for im, _ in w.loader]
    w.single = {s: [R.retrieve(m, [c], w.bank, k=K, strategy=s)[0] for c in w.clips] for s in R.STRATEGIES}
    return w


def _evaluator_tracklets(w, p):
    """The evaluator's view of product p: its detections, their tracklets (build_tracklets on the tables), each tracklet in
    ascending frame order as (frame, index inside the frame) pairs, and the tracklet the evaluator follows."""
    from seam_match_rcnn_amd import evaluator as EV
    from seam_match_rcnn_amd import ops
    t = w.tables
    dets = np.flatnonzero(t.street_prods == p)
    imgs, scores = t.street_imgs[dets], t.street_scores[dets]
    dets_d = torch.as_tensor(dets, device=w.dev)
    mine = t.street_mat[dets_d]
    sim = ops.match_scores(ops.pair_logits(mine, mine, t.w, t.b)).cpu().numpy()
    tracks = EV.build_tracklets(sim, imgs, scores, 0.3)
    first = {f: int(np.flatnonzero(imgs == f)[0]) for f in np.unique(imgs)}        # score_threshold 0: a frame's rows are its output
    ordered = [np.asarray(tr)[np.argsort(imgs[tr], kind="stable")] for tr in tracks]
    pairs = [[(int(imgs[i]), int(i - first[imgs[i]])) for i in tr] for tr in ordered]
    boxes = t.street_boxes[dets_d]
    best, best_iou = 0, -np.inf
    for ti, members in enumerate(tracks):
        gt = t.tracklets_gt[torch.as_tensor(imgs[members], device=w.dev)]
        iou = float(ops.box_iou(boxes[torch.as_tensor(members, device=w.dev)], gt).cpu().numpy().max(-1).sum())
        if iou > best_iou:
            best, best_iou = ti, iou
    return dets, ordered, pairs, best


def _pairs(tm):
    return list(zip(tm.frames, tm.detections))


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.frames == y.frames and x.detections == y.detections and x.product_keys == y.product_keys
        assert torch.equal(x.boxes, y.boxes) and torch.equal(x.scores, y.scores)
        assert torch.equal(x.product_idx, y.product_idx) and torch.equal(x.match_scores, y.match_scores)


def test_build_bank_equals_the_evaluators_shop_rows_bit_for_bit(world):
    w = world
    assert w.bank.keys == [100, 101, 102] and w.bank.missing == [] and len(w.bank) == 3
    assert torch.equal(w.bank.match, w.tables.shop_mat)
    assert torch.equal(w.bank.aggr, w.tables.shop_aggr)
    assert w.bank.boxes.shape == (3, 4) and w.bank.scores.shape == (3,)


@pytest.mark.parametrize("strategy", ["aggr_desc", "avg_desc"])
def test_tracklets_are_the_evaluators(world, strategy):
    w = world
    for p in range(3):
        _, _, pairs, _ = _evaluator_tracklets(w, p)
        got = w.single[strategy][p]
        assert [_pairs(tm) for tm in got] == pairs
        for tm in got:
            assert tm.boxes.shape == (len(tm.frames), 4) and tm.scores.shape == (len(tm.frames),)
            assert tm.product_idx.shape == (K,) and tm.match_scores.shape == (K,)
            assert tm.product_keys == [w.bank.keys[i] for i in tm.product_idx.tolist()]
            assert sorted(tm.frames) == tm.frames and bool((tm.match_scores[:-1] >= tm.match_scores[1:]).all())


def test_aggr_desc_equals_match_sequences_topk_by_hand(world):
    """The same sequence by hand: the frames through the model, the aggregator's trunk over the clip's detections, the tracklet's
    rows in frame order through Mode B, ``match_sequences_topk`` against the bank."""
    from seam_match_rcnn_amd import retrieval as R
    w = world
    agg = w.model.roi_heads.temporal_aggregator
    with torch.no_grad():
        for p in range(3):
            outs = w.model([im.to(w.dev) for im in w.clips[p]])
            start = np.concatenate([[0], np.cumsum([o["scores"].shape[0] for o in outs])])
            descr = agg.trunk(torch.cat([o["roi_features"] for o in outs]))
            for tm in w.single["aggr_desc"][p]:
                rows = torch.as_tensor([int(start[f] + d) for f, d in _pairs(tm)], device=w.dev)
                seq = torch.zeros((1 + len(rows), 1, 256), device=w.dev)
                seq[1:, 0] = descr[rows]
                mask = torch.zeros((1, 1 + len(rows)), dtype=torch.bool, device=w.dev)
                x3_1b = agg(None, None, None, x3_1_seq=seq, x3_1_mask=mask, x3_2=w.bank.aggr[:1])[0][:1]
                idx, sc = R.match_sequences_topk(agg, x3_1b.contiguous(), w.bank.aggr, K)
                assert torch.equal(idx[0].cpu(), tm.product_idx) and torch.equal(sc[0].cpu(), tm.match_scores)
                assert torch.equal(torch.cat([o["boxes"] for o in outs])[rows].cpu(), tm.boxes)


def test_followed_tracklet_ranks_the_true_product_where_the_evaluator_does(world):
    """For the tracklet the evaluator follows (largest IoU with its ground truth), the evaluator's AGGR DESC / AVG DESC rank r of
    the true product, whenever below k, is where ``retrieve`` lists that product -- for k = 3 (always) and k = 1 (rank 0 only).  The
    ranks formed here from the evaluator's pieces are checked against the evaluator's own report."""
    from seam_match_rcnn_amd import evaluator as EV
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd import retrieval as R
    w, t = world, world.tables
    agg = w.model.roi_heads.temporal_aggregator
    aw, ab = agg.last.weight.detach(), agg.last.bias.detach()
    ranks = {"aggr_desc": [], "avg_desc": []}
    firsts = {s: [R.retrieve(w.model, [c], w.bank, k=1, strategy=s)[0] for c in w.clips] for s in R.STRATEGIES}
    for p in range(3):
        dets, ordered, pairs, best = _evaluator_tracklets(w, p)
        rows = torch.as_tensor(dets[ordered[best]], device=w.dev)
        target = torch.tensor([p], dtype=torch.int64, device=w.dev)
        seg = np.array([0, len(rows)])
        desc = EV.aggregate_sequences(agg, t.street_aggr[rows], seg, t.shop_aggr[:1])
        r_aggr = int(ops.rank_of(ops.pair_logits(desc.contiguous(), t.shop_aggr, aw, ab), target).cpu())
        avg = EV.average_sequences(t.street_mat[rows].contiguous(), torch.as_tensor(seg, dtype=torch.int32, device=w.dev))
        r_avg = int(ops.rank_of(ops.pair_logits(avg, t.shop_mat, t.w, t.b), target).cpu())
        for strategy, r in (("aggr_desc", r_aggr), ("avg_desc", r_avg)):
            ranks[strategy].append(r)
            tm = [x for x in w.single[strategy][p] if _pairs(x) == pairs[best]]
            assert len(tm) == 1
            assert r < K and int(tm[0].product_idx[r]) == p and tm[0].product_keys[r] == 100 + p
            one = [x for x in firsts[strategy][p] if _pairs(x) == pairs[best]]
            assert len(one) == 1 and one[0].product_idx.shape == (1,)
            if r < 1:
                assert int(one[0].product_idx[0]) == p
            assert torch.equal(one[0].product_idx, tm[0].product_idx[:1])
    rep = EV.evaluate_tables(t, agg, k_thresholds=(1, 2, 3), frames_per_product=3)
    for strategy in ranks:
        want = sum((np.asarray([r]) < np.array([1, 2, 3])).astype(np.int64) for r in ranks[strategy])
        assert (rep.counts[strategy] == want).all(), (strategy, ranks[strategy], rep.counts[strategy])


@pytest.mark.parametrize("strategy", ["aggr_desc", "avg_desc"])
def test_three_clips_in_one_call_equal_three_calls(world, strategy):
    from seam_match_rcnn_amd import retrieval as R
    w = world
    together = R.retrieve(w.model, w.clips, w.bank, k=K, strategy=strategy)
    assert len(together) == 3
    for a, b in zip(together, w.single[strategy]):
        assert len(a) > 0
        _same(a, b)


def test_threshold_above_every_score_gives_nothing(world):
    from seam_match_rcnn_amd import retrieval as R
    w = world
    assert R.retrieve(w.model, w.clips, w.bank, k=K, score_threshold=2.0) == [[], [], []]
    assert R.retrieve(w.model, [], w.bank, k=K) == []
    # min_track_len drops the short tracklets and keeps the others as they were
    longest = max(len(tm.frames) for tm in w.single["aggr_desc"][0])
    got = R.retrieve(w.model, w.clips[:1], w.bank, k=K, min_track_len=longest)[0]
    _same(got, [tm for tm in w.single["aggr_desc"][0] if len(tm.frames) >= longest])


def test_saved_and_loaded_bank_gives_the_same_results(world, tmp_path):
    from seam_match_rcnn_amd import retrieval as R
    w = world
    path = str(tmp_path / "bank.pt")
    w.bank.save(path)
    bank = R.ProductBank.load(path, w.dev)
    assert bank.keys == w.bank.keys and torch.equal(bank.match, w.bank.match) and torch.equal(bank.aggr, w.bank.aggr)
    for strategy in R.STRATEGIES:
        _same(R.retrieve(w.model, w.clips[:1], bank, k=K, strategy=strategy)[0], w.single[strategy][0])
    cpu_bank = R.ProductBank.load(path)           # a bank on the host is moved to the model's device
    assert not cpu_bank.match.is_cuda
    _same(R.retrieve(w.model, w.clips[:1], cpu_bank, k=K)[0], w.single["aggr_desc"][0])
