"""Test-side restatement of the reference's RoI-heads training branch (ref models/matchrcnn.py:96-167,333-472 with
torchvision's roi_heads helpers, and models/match_head.py:441-504), written from the public definitions in plain torch /
NumPy on the CPU:

- ``box_iou_f32`` / ``match``: torchvision box_iou in fp32 (its expression order, no +1) and Matcher(0.5, 0.5,
  allow_low_quality_matches=False): max over the GT boxes, the first one on ties, background below 0.5 (label 0,
  matched index clamped to 0);
- ``sample_by_keys``: BalancedPositiveNegativeSampler(512, 0.25) with the product's key rule (the num_pos positives and
  num_neg negatives with the smallest (key, index)), returned in ascending order like ``nonzero(pos | neg)``;
- ``encode``: BoxCoder((10, 10, 5, 5)).encode in fp32;
- ``fastrcnn_loss`` / ``maskrcnn_loss``: the two detector losses (float64 autograd through these gives the gradients);
  ``project_masks``: roi_align(gt_masks[:, None], rois, 28, 1.0, sampling_ratio=-1, aligned=False) in float64;
- ``filter_proposals`` and ``match_loss``: the reference's match branch, quirks included.

``tests/test_roi_train_references.py`` checks the last two against outputs of the reference's own code
(``tests/golden/roi_train_golden.npz``, written by ``tests/golden/make_roi_train_golden.py``).
"""
import numpy as np
import torch
import torch.nn.functional as F

F32, F64 = torch.float32, torch.float64


# ------------------------------------------------------------------------------ select_training_samples
def box_iou_f32(gt: torch.Tensor, props: torch.Tensor) -> torch.Tensor:
    gt, props = gt.to(F32), props.to(F32)
    area1 = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
    area2 = (props[:, 2] - props[:, 0]) * (props[:, 3] - props[:, 1])
    lt = torch.max(gt[:, None, :2], props[:, :2])
    rb = torch.min(gt[:, None, 2:], props[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def match(cand: torch.Tensor, gt: torch.Tensor, gt_labels: torch.Tensor):
    """-> (labels int64 [n], matched int64 [n] (clamped), iou max fp32 [n])."""
    q = box_iou_f32(gt, cand)                                # [G, n]
    vals, idx = q.max(dim=0)
    # torch.max's index on ties is not documented: take the first maximum explicitly
    first = (q == vals[None]).to(torch.int64).argmax(dim=0)
    idx = torch.where(torch.isnan(vals), idx, first)
    bg = vals < 0.5
    labels = gt_labels[idx].clone()
    labels[bg] = 0
    matched = idx.clone()
    matched[bg] = 0
    return labels, matched, vals


def sample_by_keys(labels: torch.Tensor, keys: torch.Tensor, batch: int = 512, pos_max: int = 128) -> torch.Tensor:
    pos = torch.nonzero(labels >= 1).view(-1)
    neg = torch.nonzero(labels == 0).view(-1)
    num_pos = min(pos.numel(), pos_max)
    num_neg = min(neg.numel(), batch - num_pos)

    def smallest(ind, k):
        if k == 0:
            return ind[:0]
        kv = keys[ind].to(F64).numpy()
        order = np.lexsort((ind.numpy(), kv))               # by key, then by index
        return ind[torch.from_numpy(order[:k])]
    sel = torch.cat([smallest(pos, num_pos), smallest(neg, num_neg)])
    return torch.sort(sel).values


def encode(gt: torch.Tensor, props: torch.Tensor, weights=(10.0, 10.0, 5.0, 5.0)) -> torch.Tensor:
    wx, wy, ww, wh = weights
    ex_w = props[:, 2] - props[:, 0]
    ex_h = props[:, 3] - props[:, 1]
    ex_cx = props[:, 0] + 0.5 * ex_w
    ex_cy = props[:, 1] + 0.5 * ex_h
    gw = gt[:, 2] - gt[:, 0]
    gh = gt[:, 3] - gt[:, 1]
    gcx = gt[:, 0] + 0.5 * gw
    gcy = gt[:, 1] + 0.5 * gh
    return torch.stack([wx * (gcx - ex_cx) / ex_w, wy * (gcy - ex_cy) / ex_h,
                        ww * torch.log(gw / ex_w), wh * torch.log(gh / ex_h)], 1)


def select_training_samples(proposals, gt_boxes, gt_labels, keys, batch=512, pos_max=128):
    """Per image (CPU fp32): proposals [k,4], gt [g,4], labels [g], keys [k+g] -> list of dicts
    (idx, labels, matched, boxes, targets)."""
    out = []
    for p, g, gl, key in zip(proposals, gt_boxes, gt_labels, keys):
        if g.shape[0] == 0:
            raise ValueError("No ground-truth boxes available for one of the images during training")
        cand = torch.cat([p.to(F32), g.to(F32)])
        labels, matched, _ = match(cand, g, gl)
        idx = sample_by_keys(labels, key[:cand.shape[0]], batch, pos_max)
        out.append(dict(idx=idx, labels=labels[idx], matched=matched[idx], boxes=cand[idx],
                        targets=encode(g.to(F32)[matched[idx]], cand[idx])))
    return out


# ------------------------------------------------------------------------------ detector losses
def fastrcnn_loss(class_logits, box_regression, labels, targets):
    classification_loss = F.cross_entropy(class_logits, labels)
    pos = torch.where(labels > 0)[0]
    n = class_logits.shape[0]
    br = box_regression.reshape(n, -1, 4)
    d = br[pos, labels[pos]] - targets[pos]
    a = d.abs()
    beta = 1.0 / 9
    box_loss = torch.where(a < beta, 0.5 * a ** 2 / beta, a - 0.5 * beta).sum() / labels.numel()
    return classification_loss, box_loss


def project_masks(gt_masks: np.ndarray, boxes: np.ndarray, matched: np.ndarray, M: int = 28) -> np.ndarray:
    """roi_align(gt_masks[:, None], [matched | boxes], (M, M), 1.0, sampling_ratio=-1, aligned=False) in float64."""
    out = np.zeros((len(boxes), M, M))
    for k, (b, mi) in enumerate(zip(np.asarray(boxes, np.float64), matched)):
        m = gt_masks[int(mi)].astype(np.float64)
        H, W = m.shape
        rw, rh = max(b[2] - b[0], 1.0), max(b[3] - b[1], 1.0)
        bw, bh = rw / M, rh / M
        gw, gh = int(np.ceil(rw / M)), int(np.ceil(rh / M))
        cnt = max(gw * gh, 1)
        iy, ix = np.arange(gh) + 0.5, np.arange(gw) + 0.5
        for ph in range(M):
            y = b[1] + ph * bh + iy * bh / gh
            for pw in range(M):
                x = b[0] + pw * bw + ix * bw / gw
                Y, X = np.meshgrid(y, x, indexing="ij")
                ok = ~((Y < -1) | (Y > H) | (X < -1) | (X > W))
                Y, X = np.maximum(Y, 0), np.maximum(X, 0)
                yl, xl = Y.astype(np.int64), X.astype(np.int64)
                yc, xc = yl >= H - 1, xl >= W - 1
                yl = np.where(yc, H - 1, yl)
                xl = np.where(xc, W - 1, xl)
                Y = np.where(yc, yl, Y)
                X = np.where(xc, xl, X)
                yh, xh = np.where(yc, yl, yl + 1), np.where(xc, xl, xl + 1)
                ly, lx = Y - yl, X - xl
                hy, hx = 1 - ly, 1 - lx
                v = hy * hx * m[yl, xl] + hy * lx * m[yl, xh] + ly * hx * m[yh, xl] + ly * lx * m[yh, xh]
                out[k, ph, pw] = (v * ok).sum() / cnt
    return out


def max_grid(boxes, M: int = 28) -> int:
    """The largest adaptive sampling grid (samples per bin) of ``project_masks`` over these boxes."""
    b = np.asarray(boxes, np.float64)
    rw, rh = np.maximum(b[:, 2] - b[:, 0], 1.0), np.maximum(b[:, 3] - b[:, 1], 1.0)
    return int((np.ceil(rw / M) * np.ceil(rh / M)).max())


def target_error(boxes, H: int, W: int, M: int = 28) -> float:
    """Bound on |fp32 target - float64 target| of a 0/1 mask: the fp32 sum of up to ``max_grid`` samples, plus the rounding of
    the sample coordinates (a few ulp of the largest coordinate; a bilinear 0/1 map moves by at most 1 per pixel)."""
    span = max(float(np.abs(np.asarray(boxes, np.float64)).max()), float(H), float(W))
    return (max_grid(boxes, M) + 8 * span) * 2.0 ** -24


def sub_pixel_to_maps(logits_sub: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """[P,14,14,4*ncls] (channel (a*2+b)*ncls+c) -> the label channel as [P,28,28] maps (y = 2h+a, x = 2w+b)."""
    p = logits_sub.shape[0]
    ncls = logits_sub.shape[-1] // 4
    v = logits_sub.reshape(p, 14, 14, 2, 2, ncls)[torch.arange(p), ..., labels]          # [P,14,14,2,2]
    return v.permute(0, 1, 3, 2, 4).reshape(p, 28, 28)


def maskrcnn_loss(logits_sub, labels, targets28):
    return F.binary_cross_entropy_with_logits(sub_pixel_to_maps(logits_sub, labels), targets28)


# ------------------------------------------------------------------------------ match branch
def bb_iou_xywh(dt, gt):
    """pycocotools.mask.iou(dt, gt, [0]*len(gt)) (maskApi.c bbIou, public definition): boxes read as xywh, float64."""
    dt, gt = np.asarray(dt, np.float64), np.asarray(gt, np.float64)
    o = np.zeros((len(dt), len(gt)))
    for d in range(len(dt)):
        for g in range(len(gt)):
            D, G = dt[d], gt[g]
            w = min(D[0] + D[2], G[0] + G[2]) - max(D[0], G[0])
            h = min(D[1] + D[3], G[1] + G[3]) - max(D[1], G[1])
            if w > 0 and h > 0:
                i = w * h
                o[d, g] = i / (D[2] * D[3] + G[2] * G[3] - i)
    return o


def filter_proposals(proposals, gt_proposals, matched_idxs):
    """ref match_head.py:441-463 on per-image lists -> (kept proposals, kept matched idxs, kept row index per image)."""
    props, mids, rows = [], [], []
    for p, g, m in zip(proposals, gt_proposals, matched_idxs):
        if len(p) > 1:
            ious = torch.FloatTensor(bb_iou_xywh(p.numpy(), g.numpy())).squeeze()
            top = torch.argsort(ious, descending=True, dim=0)[:min(8 // g.shape[0], len(p))].view(-1)
        else:
            top = torch.arange(len(p))
        props.append(p[top])
        mids.append(m[top])
        rows.append(top)
    return props, mids, rows


def match_loss(logits, gt_pairs, gt_styles, types, matched_idxs):
    """MatchLossPreTrained (ref match_head.py:466-504): logits [n_street, n_shop, 2]."""
    tp = torch.cat([l[i] for l, i in zip(gt_pairs, matched_idxs)])
    ts = torch.cat([l[i] for l, i in zip(gt_styles, matched_idxs)])
    pu, su, ps, ss = tp[types == 0], ts[types == 0], tp[types == 1], ts[types == 1]
    gts = ((pu[:, None] == ps[None]) & (su[:, None] == ss[None]) & (ss[None] != 0) & (su[:, None] != 0)).to(torch.int64)
    loss = F.cross_entropy(logits.reshape(-1, 2), gts.view(-1))
    if loss > 1.0:
        loss = loss / 2.0
    return loss


# ------------------------------------------------------------------------------ golden scenarios (match branch)
def golden_cases():
    """Seeded inputs of the match-branch golden cases: per case a list of images with positive proposals (xyxy), their
    matched GT indices, the GT boxes, pair ids, styles, sources, and a logits tensor sized after filtering is known
    (drawn by the consumer from ``seed``)."""
    rng = np.random.RandomState(1234)
    cases = []

    def image(n_gt, n_pos, shop):
        gt = np.zeros((n_gt, 4), np.float32)
        gt[:, :2] = rng.uniform(0, 200, (n_gt, 2))
        gt[:, 2:] = gt[:, :2] + rng.uniform(20, 200, (n_gt, 2))
        matched = rng.randint(0, n_gt, n_pos).astype(np.int64)
        jit = rng.uniform(-15, 15, (n_pos, 4)).astype(np.float32)
        props = (gt[matched] + jit).astype(np.float32)
        props[:, 2:] = np.maximum(props[:, 2:], props[:, :2] + 1)
        if n_pos > 2:                                       # exact IoU ties: a duplicated proposal
            props[1] = props[0]
            matched[1] = matched[0]
        return dict(props=props, matched=matched, gt=gt, pair_ids=rng.randint(0, 3, n_gt).astype(np.int64),
                    styles=rng.randint(0, 3, n_gt).astype(np.int64), sources=np.array([1 if shop else 0], np.int64))
    cases.append(("one_gt", [image(1, 12, False), image(1, 5, True), image(1, 1, False), image(1, 9, True)]))
    cases.append(("three_gt", [image(3, 20, False), image(3, 2, True), image(3, 7, True), image(1, 1, False)]))
    cases.append(("nine_gt", [image(9, 30, False), image(9, 1, True), image(2, 6, True), image(2, 6, False)]))
    cases.append(("street_only", [image(2, 10, False), image(1, 4, False)]))
    return cases
