"""CPU: the test-side restatement of the RoI-heads training branch (``roi_train_refs.py``) and the product's host-side
match bookkeeping (``models/matchrcnn.py``: ``filter_positive_rows``, ``match_targets``) against outputs of the reference's
own ``filter_proposals`` / ``MatchLossPreTrained`` (``tests/golden/roi_train_golden.npz``), plus self-checks of the
detector-side restatement on cases with known answers."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import roi_train_refs as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "roi_train_golden.npz")))


def _case_inputs(imgs):
    return ([torch.from_numpy(im["props"]) for im in imgs], [torch.from_numpy(im["gt"]) for im in imgs],
            [torch.from_numpy(im["matched"]) for im in imgs])


@pytest.mark.parametrize("case", [c[0] for c in RR.golden_cases()])
def test_filter_and_match_loss_restatement_matches_reference(gold, case):
    imgs = dict(RR.golden_cases())[case]
    props, gts, mids = _case_inputs(imgs)
    kp, km, rows = RR.filter_proposals(props, gts, mids)
    for i in range(len(imgs)):
        assert np.array_equal(rows[i].numpy(), gold[f"{case}/rows_{i}"])
        assert np.array_equal(km[i].numpy(), gold[f"{case}/matched_{i}"])
    types = torch.cat([torch.full((len(p),), int(im["sources"][0] == 1), dtype=torch.int32) for p, im in zip(kp, imgs)])
    assert np.array_equal(types.numpy(), gold[f"{case}/types"])
    logits = torch.from_numpy(gold[f"{case}/logits"]).clone().requires_grad_(True)
    loss = RR.match_loss(logits, [torch.from_numpy(im["pair_ids"]) for im in imgs],
                         [torch.from_numpy(im["styles"]) for im in imgs], types, km)
    ref = float(gold[f"{case}/loss"])
    if np.isnan(ref):
        assert torch.isnan(loss)
        return
    assert float(loss.detach()) == pytest.approx(ref, rel=1e-6)
    loss.backward()
    np.testing.assert_allclose(logits.grad.numpy(), gold[f"{case}/dlogits"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("case", [c[0] for c in RR.golden_cases()])
def test_product_host_bookkeeping_matches_reference(gold, case):
    from seam_match_rcnn_amd.models.matchrcnn import filter_positive_rows, match_targets
    imgs = dict(RR.golden_cases())[case]
    pairs, styles, types = [], [], []
    for i, im in enumerate(imgs):
        rows = filter_positive_rows(im["props"], im["gt"])
        assert np.array_equal(rows, gold[f"{case}/rows_{i}"])
        mi = im["matched"][rows]
        pairs.append(im["pair_ids"][mi])
        styles.append(im["styles"][mi])
        types.append(np.full(len(rows), int(im["sources"][0] == 1)))
    types = np.concatenate(types)
    gts = match_targets(np.concatenate(pairs), np.concatenate(styles), types)
    logits = torch.from_numpy(gold[f"{case}/logits"])
    assert gts.shape == tuple(logits.shape[:2])
    ref = float(gold[f"{case}/loss"])
    if gts.size == 0:
        assert np.isnan(ref)
        return
    loss = F.cross_entropy(logits.reshape(-1, 2), torch.from_numpy(gts.reshape(-1)))
    loss = loss / 2 if loss > 1.0 else loss
    assert float(loss) == pytest.approx(ref, rel=1e-6)


def test_golden_covers_the_cases_the_issue_names(gold):
    cases = dict(RR.golden_cases())
    n_gts = {len(im["gt"]) for imgs in cases.values() for im in imgs}
    assert {1, 3, 9} <= n_gts
    n_pos = {len(im["props"]) for imgs in cases.values() for im in imgs}
    assert 1 in n_pos and max(n_pos) >= 12
    assert float(gold["three_gt/loss"]) > 1.0 / 2          # the halved case: the raw loss was above 1
    assert np.isnan(gold["street_only/loss"])
    assert set(gold["one_gt/types"].tolist()) == {0, 1}


def test_matcher_sampler_encode_known_answers():
    gt = torch.tensor([[0., 0., 10., 10.], [0., 0., 10., 10.], [50., 50., 60., 70.]])
    gl = torch.tensor([3, 4, 5])
    cand = torch.tensor([[0., 0., 10., 10.],     # IoU 1 with GT 0 and GT 1: the first wins
                         [0., 0., 10., 5.],      # IoU exactly 0.5: foreground
                         [0., 0., 10., 4.],      # 0.4: background
                         [50., 50., 60., 70.],
                         [200., 200., 210., 210.]])
    labels, matched, vals = RR.match(cand, gt, gl)
    assert labels.tolist() == [3, 3, 0, 5, 0] and matched.tolist() == [0, 0, 0, 2, 0]
    assert float(vals[1]) == 0.5
    keys = torch.tensor([0.9, 0.1, 0.5, 0.1, 0.5])
    assert RR.sample_by_keys(labels, keys, batch=3, pos_max=2).tolist() == [1, 2, 3]     # pos {0,1,3} -> {1,3}; neg tie: 2 before 4
    t = RR.encode(gt[[0]], torch.tensor([[0., 0., 10., 10.]]))
    assert torch.equal(t, torch.zeros(1, 4))


def test_sampler_takes_the_smallest_keys_lower_index_on_ties():
    labels = torch.tensor([0, 1, 0, 1, 0, 0, 1])
    keys = torch.tensor([0.3, 0.2, 0.3, 0.2, 0.1, 0.3, 0.2])
    # positives {1,3,6} all key 0.2 -> the first two; negatives: 4 (0.1), then 0 and 2 (0.3, lower indices)
    assert RR.sample_by_keys(labels, keys, batch=5, pos_max=2).tolist() == [0, 1, 2, 3, 4]


def test_detector_losses_and_projection_known_answers():
    logits = torch.zeros(4, 3)
    labels = torch.tensor([0, 1, 2, 0])
    br = torch.zeros(4, 12)
    tg = torch.zeros(4, 4)
    tg[1, 0] = 1.0                 # |d| = 1 >= beta: 1 - beta/2
    tg[2, 1] = 0.05                # |d| < beta: 0.5 d^2 / beta
    lc, lb = RR.fastrcnn_loss(logits, br, labels, tg)
    assert float(lc) == pytest.approx(np.log(3.0))
    assert float(lb) == pytest.approx(((1 - 0.5 / 9) + 0.5 * 0.05 ** 2 * 9) / 4)
    m = np.zeros((1, 40, 60), np.uint8)
    m[0, 10:30, 20:50] = 1
    t = RR.project_masks(m, np.array([[22., 12., 48., 28.]]), np.array([0]))
    assert np.allclose(t, 1.0)
    t = RR.project_masks(m, np.array([[0., 0., 15., 8.]]), np.array([0]))
    assert np.allclose(t, 0.0)
    t = RR.project_masks(m, np.array([[0., 0., 60., 40.]]), np.array([0]))         # 3 x 2 samples per bin
    assert 0.0 < t.mean() < 1.0 and t.shape == (1, 28, 28)
    sub = torch.arange(2 * 14 * 14 * 8, dtype=torch.float64).reshape(2, 14, 14, 8)
    maps = RR.sub_pixel_to_maps(sub, torch.tensor([1, 0]))
    assert float(maps[0, 3, 5]) == float(sub[0, 1, 2, (1 * 2 + 1) * 2 + 1])
    assert float(maps[1, 2, 4]) == float(sub[1, 1, 2, 0])
