"""Float64 restatement of the COCO detection protocol that ``seam_match_rcnn_amd.evaluator_det`` implements, written for
the tests: plain Python loops over scalars, one detection and one ground truth at a time, no code shared with the evaluator
and none of its vectorised shortcuts (no ``searchsorted``, no ``maximum.accumulate``, no IoU matrices).  Mask IoU is taken
from full-resolution boolean masks, never from the 28x28 probabilities.

A scene is a list of images; an image is a dict of NumPy arrays:

    det_boxes [K,4] float32 xyxy, det_labels [K] int, det_scores [K] float, det_masks [K,H,W] bool (segm only)
    gt_boxes  [n,4] float32 xyxy, gt_labels  [n] int, gt_area [n] (optional), gt_crowd [n] (optional), gt_masks [n,H,W] bool

Neither pycocotools nor torchvision is installed where this project is tested, so this file is a second reading of the
published procedure, not a recording of the original.
"""
import numpy as np

THRESHOLDS = np.linspace(0.5, 0.95, 10)
RECALLS = np.linspace(0.0, 1.0, 101)
RANGES = ((0.0, 1e10), (0.0, 32.0 ** 2), (32.0 ** 2, 96.0 ** 2), (96.0 ** 2, 1e10))


def xywh(box):
    """xyxy -> (x, y, w, h) as Python floats, w and h subtracted in fp32."""
    x1, y1, x2, y2 = (np.float32(v) for v in box)
    return float(x1), float(y1), float(x2 - x1), float(y2 - y1)


def box_iou(det, gt, crowd):
    dx, dy, dw, dh = xywh(det)
    gx, gy, gw, gh = xywh(gt)
    iw = min(dx + dw, gx + gw) - max(dx, gx)
    if iw <= 0:
        return 0.0
    ih = min(dy + dh, gy + gh) - max(dy, gy)
    if ih <= 0:
        return 0.0
    inter = iw * ih
    return inter / (dw * dh if crowd else dw * dh + gw * gh - inter)


def mask_iou(det, gt, crowd):
    inter = float(np.count_nonzero(det & gt))
    den = float(np.count_nonzero(det)) if crowd else float(np.count_nonzero(det)) + float(np.count_nonzero(gt)) - inter
    return inter / den if den != 0 else 0.0


def _instances(img, iou_type):
    dets, gts = [], []
    for i in range(len(img["det_labels"])):
        _, _, w, h = xywh(img["det_boxes"][i])
        mask = img["det_masks"][i] if iou_type == "segm" else None
        area = float(np.count_nonzero(mask)) if iou_type == "segm" else w * h
        dets.append(dict(box=img["det_boxes"][i], label=int(img["det_labels"][i]), score=float(img["det_scores"][i]), mask=mask,
                         area=area))
    for i in range(len(img["gt_labels"])):
        _, _, w, h = xywh(img["gt_boxes"][i])
        gts.append(dict(box=img["gt_boxes"][i], label=int(img["gt_labels"][i]),
                        area=float(img["gt_area"][i]) if "gt_area" in img else w * h,
                        crowd=bool(img["gt_crowd"][i]) if "gt_crowd" in img else False,
                        mask=img["gt_masks"][i] if iou_type == "segm" else None))
    return dets, gts


def _match_image(dets, gts, lo, hi, iou_type):
    """-> per detection (score order): score, and per threshold the (matched, ignored) pair; and the non-ignored count."""
    for g in gts:
        g["ignore"] = g["crowd"] or g["area"] < lo or g["area"] > hi
    gts = [g for g in gts if not g["ignore"]] + [g for g in gts if g["ignore"]]
    out = [dict(score=d["score"], matched=[], ignored=[]) for d in dets]
    for t in THRESHOLDS:
        used = [False] * len(gts)
        for d, o in zip(dets, out):
            best, m = min(float(t), 1 - 1e-10), None
            for gi, g in enumerate(gts):
                if used[gi] and not g["crowd"]:
                    continue
                if m is not None and not gts[m]["ignore"] and g["ignore"]:
                    break
                iou = box_iou(d["box"], g["box"], g["crowd"]) if iou_type == "bbox" else mask_iou(d["mask"], g["mask"], g["crowd"])
                if iou < best:
                    continue
                best, m = iou, gi
            if m is None:
                o["matched"].append(False)
                o["ignored"].append(d["area"] < lo or d["area"] > hi)
            else:
                used[m] = True
                o["matched"].append(True)
                o["ignored"].append(gts[m]["ignore"])
    return out, sum(1 for g in gts if not g["ignore"])


def evaluate(scene, iou_type, max_dets=(1, 10, 100)):
    """-> dict(stats=[12 floats], precision [T,R,K,A,M], recall [T,K,A,M], categories)."""
    cats = sorted({int(c) for img in scene for c in img["gt_labels"]})
    T, R = len(THRESHOLDS), len(RECALLS)
    precision = -np.ones((T, R, len(cats), len(RANGES), len(max_dets)))
    recall = -np.ones((T, len(cats), len(RANGES), len(max_dets)))
    for k, cat in enumerate(cats):
        for a, (lo, hi) in enumerate(RANGES):
            per_image, npig = [], 0
            for img in scene:
                dets, gts = _instances(img, iou_type)
                dets = [d for d in dets if d["label"] == cat]
                gts = [g for g in gts if g["label"] == cat]
                if not dets and not gts:
                    continue
                dets = sorted(dets, key=lambda d: -d["score"])[:max_dets[-1]]          # sorted() is stable
                rows, n = _match_image(dets, gts, lo, hi, iou_type)
                per_image.append(rows)
                npig += n
            if npig == 0:
                continue
            for m, top in enumerate(max_dets):
                rows = sorted([r for img_rows in per_image for r in img_rows[:top]], key=lambda r: -r["score"])
                for t in range(T):
                    tp = fp = 0
                    rc, pr = [], []
                    for r in rows:
                        if not r["ignored"][t]:
                            tp += 1 if r["matched"][t] else 0
                            fp += 0 if r["matched"][t] else 1
                        rc.append(np.float64(tp) / npig)
                        pr.append(np.float64(tp) / (np.float64(tp) + np.float64(fp) + np.spacing(1)))
                    recall[t, k, a, m] = rc[-1] if rc else 0.0
                    for i in range(len(pr) - 2, -1, -1):
                        if pr[i + 1] > pr[i]:
                            pr[i] = pr[i + 1]
                    for ri, want in enumerate(RECALLS):
                        q = 0.0
                        for i in range(len(rc)):
                            if rc[i] >= want:
                                q = pr[i]
                                break
                        precision[t, ri, k, a, m] = q
    return dict(stats=summarize(precision, recall), precision=precision, recall=recall, categories=cats)


def summarize(precision, recall):
    """The twelve COCO numbers from the two tables (max_dets in their last axis, the AP rows use the last one)."""
    def mean(cells):
        vals = [float(v) for v in np.asarray(cells).reshape(-1) if v > -1]
        return sum(vals) / len(vals) if vals else -1.0
    last = precision.shape[-1] - 1
    return [mean(precision[:, :, :, 0, last]), mean(precision[0, :, :, 0, last]), mean(precision[5, :, :, 0, last]),
            mean(precision[:, :, :, 1, last]), mean(precision[:, :, :, 2, last]), mean(precision[:, :, :, 3, last]),
            mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
            mean(recall[:, :, 1, last]), mean(recall[:, :, 2, last]), mean(recall[:, :, 3, last])]


def assert_same_stats(got, want, tol=1e-12, what=""):
    """The tests' comparator: twelve numbers, each within ``tol`` (absolute) of the restatement's."""
    got, want = [float(v) for v in got], [float(v) for v in want]
    assert len(got) == 12 and len(want) == 12, f"{what}: twelve numbers expected, got {len(got)} and {len(want)}"
    bad = [(i + 1, g, w) for i, (g, w) in enumerate(zip(got, want)) if not abs(g - w) <= tol]
    assert not bad, f"{what}: entries (index, got, want) differ by more than {tol}: {bad}"


# --------------------------------------------------------------------------------------------- scenes
def xyxy(boxes_xywh):
    b = np.asarray(boxes_xywh, dtype=np.float32).reshape(-1, 4).copy()
    b[:, 2] += b[:, 0]
    b[:, 3] += b[:, 1]
    return b


def image(gt_xywh, gt_labels, det_xywh, det_labels, det_scores, gt_area=None, gt_crowd=None):
    img = dict(gt_boxes=xyxy(gt_xywh), gt_labels=np.asarray(gt_labels, dtype=np.int64), det_boxes=xyxy(det_xywh),
               det_labels=np.asarray(det_labels, dtype=np.int64), det_scores=np.asarray(det_scores, dtype=np.float32))
    if gt_area is not None:
        img["gt_area"] = np.asarray(gt_area, dtype=np.float64)
    if gt_crowd is not None:
        img["gt_crowd"] = np.asarray(gt_crowd, dtype=np.int64)
    return img


def random_scene(seed, n_images=4, n_classes=3, size=200.0, crowd=True):
    """Seeded boxes-only scene: ground truths of mixed sizes; detections that are shifted or shrunk copies of ground truths
    (IoU 0.14 ... 1), strays, duplicate hits, wrong labels and detections of a class without ground truth.  All scores are
    distinct.  The thresholds are 0.05 apart, so an IoU can only be kept out of rounding's reach of them, not far from
    them: a test that uses a scene asserts ``min_threshold_margin(scene) > 1e-6`` first."""
    rng = np.random.RandomState(seed)
    # relative (dx, dw) jitters applied to both axes; IoU of the jittered square box with the original:
    #   shift s (same size):  (1-s)^2 / (2 - (1-s)^2)      shrink f (same corner): f^2
    jit = [(0.0, 1.0), (0.03, 1.0), (0.11, 1.0), (0.0, 0.88), (0.0, 0.76), (0.21, 1.0), (0.5, 1.0)]
    scene, n_scores = [], 0
    for _ in range(n_images):
        ng = int(rng.randint(0, 6))
        side = rng.choice([12.0, 24.0, 40.0, 64.0, 100.0, 120.0], size=ng)
        xy = np.floor(rng.uniform(0, size, size=(ng, 2)))
        gt = np.concatenate([xy, side[:, None], side[:, None]], 1).reshape(-1, 4)
        gl = rng.randint(1, n_classes + 1, size=ng)
        det, dl = [], []
        for g, lab in zip(gt, gl):
            for _ in range(int(rng.randint(0, 3))):
                s, f = jit[int(rng.randint(len(jit)))]
                det.append([g[0] + s * g[2], g[1] + s * g[3], f * g[2], f * g[3]])
                dl.append(int(lab) if rng.rand() < 0.85 else int(rng.randint(1, n_classes + 2)))
        for _ in range(int(rng.randint(0, 3))):
            det.append(list(rng.uniform(0, size, size=2)) + [30.0, 50.0])
            dl.append(int(rng.randint(0, n_classes + 2)))
        img = image(gt, gl, det, dl, np.zeros(len(det)),
                    gt_crowd=(rng.rand(ng) < 0.15).astype(np.int64) if crowd else None)
        n_scores += len(det)
        scene.append(img)
    scores = (rng.permutation(n_scores) + 1.0) / (n_scores + 1.0)            # all distinct
    off = 0
    for img in scene:
        k = len(img["det_labels"])
        img["det_scores"] = scores[off:off + k].astype(np.float32)
        off += k
    return scene


def min_threshold_margin(scene):
    """Smallest distance of any same-image box IoU (in the form its ground truth asks for) to a matching threshold."""
    margin = 1.0
    for img in scene:
        crowd = img["gt_crowd"] if "gt_crowd" in img else np.zeros(len(img["gt_labels"]))
        for d in img["det_boxes"]:
            for g, c in zip(img["gt_boxes"], crowd):
                margin = min(margin, float(np.abs(THRESHOLDS - box_iou(d, g, bool(c))).min()))
    return margin


def to_io(scene, torch, device=None):
    """Scene -> (outputs, targets) as the evaluator takes them (boxes-only; masks are added by the GPU tests)."""
    outs, tgts = [], []
    for img in scene:
        o = dict(boxes=torch.from_numpy(img["det_boxes"].astype(np.float32)).reshape(-1, 4),
                 labels=torch.from_numpy(img["det_labels"].astype(np.int64)),
                 scores=torch.from_numpy(img["det_scores"].astype(np.float32)))
        t = dict(boxes=torch.from_numpy(img["gt_boxes"].astype(np.float32)).reshape(-1, 4),
                 labels=torch.from_numpy(img["gt_labels"].astype(np.int64)))
        if "gt_area" in img:
            t["area"] = torch.from_numpy(img["gt_area"])
        if "gt_crowd" in img:
            t["iscrowd"] = torch.from_numpy(img["gt_crowd"])
        if device is not None:
            o = {k: v.to(device) for k, v in o.items()}
        outs.append(o)
        tgts.append(t)
    return outs, tgts
