"""GPU: box and mask AP on the device (run with -m gpu).

1. ``seam_mask_inter_f32`` equals, as integers, the thresholded paste intersected with the ground truths -- through the C
   ABI, onto poisoned outputs with guard words, twice, bit-identical -- over every image size x D x G x probability-map kind
   of the lists below, with boxes of every awkward kind in each case.
2. ``evaluator_det.evaluate`` on planted detections equals the float64 restatement (tests/det_eval_refs.py) fed with
   full-resolution masks, to 1e-12 (the same decisions on the same integer counts: only summation order differs).
3. On a real seeded model ``paste_masks = False`` changes no box, label or score, its ``mask_probs`` paste to the default
   route's ``masks``, and both routes give the same twelve numbers per IoU type.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import det_eval_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-12

IMAGES = ((1, 1), (33, 47), (64, 40), (96, 96))
DS = (1, 5, 17)
GS = (0, 1, 3, 33)
MAPS = ("uniform", "half", "half_up", "checker", "zeros", "ones")
BOXES = ("random", "partly_outside", "outside", "inverted", "zero_size", "sub_pixel", "whole_image")
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1.0)))
POISON = (0x5A5A5A5A, 0x3C3C3C3C)
GUARD = 16


@pytest.fixture(scope="module")
def ops():
    import seam_match_rcnn_amd.ops as ops
    return ops


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def make_maps(kind, d, rng):
    if kind == "uniform":
        m = rng.uniform(0, 1, size=(d, 28, 28))
    elif kind == "checker":
        yy, xx = np.mgrid[0:28, 0:28]
        m = np.broadcast_to(((yy + xx) % 2).astype(np.float64), (d, 28, 28))
    else:
        m = np.full((d, 28, 28), {"half": 0.5, "half_up": HALF_UP, "zeros": 0.0, "ones": 1.0}[kind])
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.float32))


def make_box(kind, h, w, rng):
    if kind == "random":
        x, y = rng.uniform(0, w), rng.uniform(0, h)
        return [x, y, x + rng.uniform(0.5, w), y + rng.uniform(0.5, h)]
    if kind == "partly_outside":
        return [-rng.uniform(1, w), rng.uniform(0, h / 2), rng.uniform(0.5, w), h + rng.uniform(1, h)]
    if kind == "outside":
        return [[w + 5.0, h + 3.0, 2.0 * w + 9.0, 2.0 * h + 7.0], [-3.0 * w - 4.0, -2.0 * h - 6.0, -w - 4.0, -6.0]][rng.randint(2)]
    if kind == "inverted":
        return [0.8 * w, 0.7 * h, 0.2 * w, 0.1 * h]
    if kind == "zero_size":
        x, y = rng.uniform(0, w), rng.uniform(0, h)
        return [x, y, x, y]
    if kind == "sub_pixel":
        x, y = rng.uniform(0, w), rng.uniform(0, h)
        return [x, y, x + 0.3, y + 0.2]
    return [0.0, 0.0, float(w), float(h)]


def poisoned(n, word):
    """int32 [GUARD + n + GUARD] filled with ``word``; the middle is the output."""
    return torch.full((2 * GUARD + n,), word, dtype=torch.int32, device=DEV)


def ptr(t, offset_words=0):
    return C.c_void_p(t.data_ptr() + 4 * offset_words)


def call_abi(lib, probs, boxes, d, gt, g, h, w, inter_buf, area_buf):
    return lib.seam_mask_inter_f32(ptr(probs), ptr(boxes), d, ptr(gt) if gt is not None else None, g, h, w,
                                   ptr(inter_buf, GUARD) if inter_buf is not None else None,
                                   ptr(area_buf, GUARD) if area_buf is not None else None,
                                   torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("hw", IMAGES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_mask_inter_equals_the_thresholded_paste(ops, lib, hw):
    h, w = hw
    rng = np.random.RandomState(h * 1000 + w)
    ran = 0
    for d in DS:
        for g in GS:
            for mi, kind in enumerate(MAPS):
                kinds = [BOXES[(ran + j) % len(BOXES)] for j in range(d)]
                boxes = torch.tensor([make_box(k, h, w, rng) for k in kinds], dtype=torch.float32).to(DEV)
                probs = make_maps(kind, d, rng).to(DEV)
                gt = torch.from_numpy(rng.choice(np.array([0, 1, 255], dtype=np.uint8), size=(g, h, w))).to(DEV)
                pasted = ops.paste_masks(probs[:, None], boxes, (h, w))
                m = pasted[:, 0] > 0.5
                want_inter = (m[:, None] & (gt != 0)[None]).sum((2, 3)).to(torch.int32)
                want_area = m.sum((1, 2)).to(torch.int32)
                runs = []
                for word in POISON:
                    ib, ab = poisoned(d * g, word), poisoned(d, word)
                    rc = call_abi(lib, probs, boxes, d, gt if g else None, g, h, w, ib if g else None, ab)
                    assert rc == 0, (rc, d, g, kind)
                    for buf, n in ((ib, d * g), (ab, d)):
                        assert bool((buf[:GUARD] == word).all()) and bool((buf[GUARD + n:] == word).all()), ("guard", d, g, kind)
                    runs.append((ib[GUARD:GUARD + d * g].reshape(d, g).clone(), ab[GUARD:GUARD + d].clone()))
                what = f"{h}x{w} D={d} G={g} {kind} {kinds}"
                assert torch.equal(runs[0][0], want_inter) and torch.equal(runs[0][1], want_area), what
                assert torch.equal(runs[1][0], runs[0][0]) and torch.equal(runs[1][1], runs[0][1]), what
                inter, area = ops.mask_inter(probs[:, None] if mi % 2 else probs, boxes, gt)
                assert inter.dtype == torch.int32 and area.dtype == torch.int32 and tuple(inter.shape) == (d, g)
                assert torch.equal(inter, want_inter) and torch.equal(area, want_area), what
                if kind in ("half", "zeros"):                 # a pasted value of exactly 0.5 is not set
                    assert int(want_area.sum()) == 0 and int(area.sum()) == 0, what
                if kind in ("half_up", "ones") and "whole_image" in kinds:      # one ulp above is
                    assert int(area[kinds.index("whole_image")]) > 0, what
                ran += 1
    assert ran == len(DS) * len(GS) * len(MAPS) == 72


def test_mask_inter_sees_every_kind_of_box_and_some_overlap(ops):
    """The sweep above is not vacuous: with solid maps the awkward boxes give the areas their geometry says, and a ground truth
    that is the detection's own mask is met on every pixel."""
    h, w = 64, 40
    rng = np.random.RandomState(7)
    fixed = {"random": [5.3, 7.1, 30.2, 50.9], "partly_outside": [-10.0, 20.0, 15.5, 80.0]}
    boxes = torch.tensor([fixed.get(k) or make_box(k, h, w, rng) for k in BOXES], dtype=torch.float32).to(DEV)
    probs = make_maps("ones", len(BOXES), rng).to(DEV)
    own = (ops.paste_masks(probs[:, None], boxes, (h, w))[:, 0] > 0.5).to(torch.uint8) * 255
    inter, area = ops.mask_inter(probs, boxes, own)
    a = dict(zip(BOXES, area.tolist()))
    assert a["outside"] == 0 and a["inverted"] == 0 and a["random"] > 0 and a["partly_outside"] > 0
    assert 0.9 * h * w < a["whole_image"] <= h * w
    assert torch.equal(inter.diagonal(), area)
    assert torch.equal(inter, inter.t())                   # |A & B| is symmetric when the ground truths are the masks


def test_mask_inter_refusals_leave_the_outputs_untouched(ops, lib):
    d, g, h, w = 3, 2, 20, 30
    rng = np.random.RandomState(3)
    probs, boxes = make_maps("ones", d, rng).to(DEV), torch.tensor([[2.0, 3.0, 25.0, 15.0]] * d).to(DEV)
    gt = torch.ones((g, h, w), dtype=torch.uint8, device=DEV)
    word = POISON[0]
    ib, ab = poisoned(d * g, word), poisoned(d, word)
    s = torch.cuda.current_stream().cuda_stream
    f = lib.seam_mask_inter_f32
    P, B, Gt, I, A = ptr(probs), ptr(boxes), ptr(gt), ptr(ib, GUARD), ptr(ab, GUARD)
    refused = [
        f(None, B, d, Gt, g, h, w, I, A, s), f(P, None, d, Gt, g, h, w, I, A, s), f(P, B, d, None, g, h, w, I, A, s),
        f(P, B, d, Gt, g, h, w, None, A, s), f(P, B, d, Gt, g, h, w, I, None, s), f(P, B, d, None, 0, h, w, None, None, s),
        f(P, B, -1, Gt, g, h, w, I, A, s), f(P, B, d, Gt, -1, h, w, I, A, s), f(P, B, d, Gt, g, -1, w, I, A, s),
        f(P, B, d, Gt, g, h, -1, I, A, s), f(P, B, d, Gt, g, 65536, 32768, I, A, s), f(P, B, d, Gt, g, 46341, 46341, I, A, s),
    ]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert f(P, B, 0, Gt, g, h, w, I, A, s) == 0 and f(None, None, 0, None, 0, 0, 0, None, None, s) == 0        # D == 0: a no-op
    torch.cuda.synchronize()
    assert bool((ib == word).all()) and bool((ab == word).all())
    assert f(P, B, d, None, 0, h, w, None, A, s) == 0                  # G == 0: det_area only, inter and gt may be null
    torch.cuda.synchronize()
    assert bool((ib == word).all()) and bool((ab[:GUARD] == word).all()) and bool((ab[GUARD + d:] == word).all())
    assert ab[GUARD:GUARD + d].tolist() == ops.mask_inter(probs, boxes, gt)[1].tolist() and int(ab[GUARD]) > 0
    # the wrapper's own checks
    with pytest.raises(TypeError):
        ops.mask_inter(probs, boxes, gt.to(torch.float32))
    with pytest.raises(ValueError):
        ops.mask_inter(probs[:, :27], boxes, gt)
    with pytest.raises(ValueError):
        ops.mask_inter(probs, boxes[:2], gt)
    with pytest.raises(ValueError):
        ops.mask_inter(probs, boxes, gt[0])
    empty = ops.mask_inter(probs[:0], boxes[:0], gt)
    assert tuple(empty[0].shape) == (0, g) and tuple(empty[1].shape) == (0,)


# ------------------------------------------------------------------------------------------------ planted protocol
def disk(radius):
    yy, xx = np.mgrid[0:28, 0:28]
    return (((yy - 13.5) ** 2 + (xx - 13.5) ** 2) <= radius ** 2).astype(np.float32)


def planted_images(ops):
    """Two images of different sizes.  Ground-truth masks are thresholded pastes of planted boxes and maps; the detections
    repeat some of them exactly (mask IoU 1), shift or shrink others (a known partial overlap) or miss."""
    solid, ball, ring = np.ones((28, 28), np.float32), disk(12.0), disk(13.0) - disk(6.0)
    soft = np.clip(disk(11.0) * 0.7 + 0.1, 0, 1).astype(np.float32)
    plan = [
        dict(hw=(90, 120),
             gt=[([10, 8, 50, 60], solid, 1), ([60, 20, 110, 80], ball, 2), ([20, 60, 45, 85], ring, 1), ([70, 5, 100, 18], soft, 2)],
             det=[([10, 8, 50, 60], solid, 1, 0.95), ([64, 20, 114, 80], ball, 2, 0.9), ([20, 60, 45, 85], ring, 1, 0.85),
                  ([22, 30, 50, 60], solid, 1, 0.6), ([70, 5, 100, 18], soft, 1, 0.55), ([70, 5, 100, 18], soft, 2, 0.5),
                  ([100, 70, 118, 88], solid, 2, 0.4), ([5, 5, 9, 9], ball, 0, 0.99)]),
        dict(hw=(75, 64),
             gt=[([5, 5, 40, 70], ball, 2), ([30, 10, 60, 40], solid, 3)],
             det=[([5, 5, 40, 70], ball, 2, 0.8), ([30, 10, 60, 46], solid, 3, 0.7), ([30, 10, 60, 40], ring, 3, 0.65),
                  ([0, 50, 20, 74], solid, 1, 0.3)]),
    ]
    scene, outputs, targets = [], [], []
    for p in plan:
        h, w = p["hw"]
        gb = torch.tensor([b for b, _, _ in p["gt"]], dtype=torch.float32)
        gm = (ops.paste_masks(torch.from_numpy(np.stack([m for _, m, _ in p["gt"]]))[:, None].to(DEV), gb.to(DEV), (h, w))[:, 0] > 0.5)
        db = torch.tensor([b for b, _, _, _ in p["det"]], dtype=torch.float32)
        dp = torch.from_numpy(np.stack([m for _, m, _, _ in p["det"]]))[:, None].to(DEV)
        pasted = ops.paste_masks(dp, db.to(DEV), (h, w))
        scene.append(dict(det_boxes=db.numpy(), det_labels=np.int64([c for _, _, c, _ in p["det"]]),
                          det_scores=np.float32([s for _, _, _, s in p["det"]]), det_masks=(pasted[:, 0] > 0.5).cpu().numpy(),
                          gt_boxes=gb.numpy(), gt_labels=np.int64([c for _, _, c in p["gt"]]), gt_masks=gm.cpu().numpy()))
        outputs.append(dict(boxes=db.to(DEV), labels=torch.tensor([c for _, _, c, _ in p["det"]]).to(DEV),
                            scores=torch.tensor([s for _, _, _, s in p["det"]], dtype=torch.float32).to(DEV),
                            mask_probs=dp, masks=pasted))
        targets.append(dict(boxes=gb, labels=torch.tensor([c for _, _, c in p["gt"]]), masks=gm.to(torch.uint8).cpu()))
    return scene, outputs, targets


class Planted:
    """Stands in for the model: planted detections, ``mask_probs`` or pasted ``masks`` as the switch says."""
    paste_masks = True

    def __init__(self, outputs):
        self.outputs, self.seen, self.modes = outputs, 0, []

    def eval(self):
        return self

    def __call__(self, images):
        assert not torch.is_grad_enabled()
        self.modes.append(self.paste_masks)
        drop = "mask_probs" if self.paste_masks else "masks"
        out = [{k: v for k, v in o.items() if k != drop} for o in self.outputs[self.seen:self.seen + len(images)]]
        self.seen += len(images)
        return out


def test_planted_masks_agree_with_the_restatement(ops, monkeypatch):
    from seam_match_rcnn_amd import evaluator_det as E
    scene, outputs, targets = planted_images(ops)
    # the plan holds what it says: exact repeats, partial overlaps, and nothing on a threshold
    ious = [R.mask_iou(scene[0]["det_masks"][i], scene[0]["gt_masks"][j], False) for i, j in ((0, 0), (2, 2), (1, 1), (3, 0))]
    assert ious[0] == 1.0 and ious[1] == 1.0 and 0.5 < ious[2] < 1.0 and 0.1 < ious[3] < 0.9
    margin = min(abs(R.mask_iou(d, g, False) - t) for img in scene for d in img["det_masks"] for g in img["gt_masks"]
                 for t in R.THRESHOLDS)
    assert margin > 1e-6 and R.min_threshold_margin(scene) > 1e-6
    want = {t: R.evaluate(scene, t)["stats"] for t in ("segm", "bbox")}
    assert any(v not in (-1.0, 0.0, 1.0) for v in want["segm"]) and want["segm"] != want["bbox"]

    copies = []
    real_cpu = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (copies.append(self.is_cuda), real_cpu(self, *a, **k))[1])
    images = [torch.zeros(3, *img["gt_masks"].shape[1:]) for img in scene]
    model = Planted(outputs)
    stats, ev = E.evaluate(model, [(images[:1], targets[:1]), (images[1:], targets[1:], [1])], DEV, verbose=False,
                           return_report=True)
    assert copies.count(True) == 2                          # one device-to-host copy per update
    monkeypatch.undo()
    assert model.modes == [False, False] and model.paste_masks is True
    for t in ("segm", "bbox"):
        R.assert_same_stats(stats[t], want[t], TOL, t)
    assert ev.categories == [1, 2, 3]
    # the slow route: pasted masks thresholded with torch ops
    slow = E.DetectionEvaluator()
    slow.update([{k: v for k, v in o.items() if k != "mask_probs"} for o in outputs], targets)
    got = slow.summarize(verbose=False)
    assert got["segm"] == stats["segm"] and got["bbox"] == stats["bbox"]
    # a crowd ground truth and explicit areas go through the mask route too
    crowd_scene = [dict(scene[0], gt_crowd=np.int64([0, 1, 0, 0]), gt_area=np.float64([900.0, 3000.0, 500.0, 12000.0])), scene[1]]
    crowd_targets = [dict(targets[0], iscrowd=torch.tensor([0, 1, 0, 0]), area=torch.tensor([900.0, 3000.0, 500.0, 12000.0])),
                     targets[1]]
    ev = E.DetectionEvaluator()
    ev.update([{k: v for k, v in o.items() if k != "masks"} for o in outputs], crowd_targets)
    got = ev.summarize(verbose=False)
    for t in ("segm", "bbox"):
        R.assert_same_stats(got[t], R.evaluate(crowd_scene, t)["stats"], TOL, "crowd " + t)


# ------------------------------------------------------------------------------------------------ a real model
NCLS = 5


@pytest.fixture(scope="module")
def model_batch():
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS, min_size=256, max_size=320, box_score_thresh=0.0)
    sd = synth.detector_state(5, NCLS)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(0)
    images, targets = [], []
    for i, (h, w) in enumerate(((200, 250), (192, 240))):
        images.append(torch.from_numpy(synth.frames(50 + i, 1, h, w)[0]))
        ng = 2 + i
        xy = torch.rand((ng, 2), generator=g) * torch.tensor([w - 130.0, h - 130.0])
        wh = 30 + torch.rand((ng, 2), generator=g) * 90
        gt = torch.cat([xy, xy + wh], 1).round()
        masks = torch.zeros((ng, h, w), dtype=torch.uint8)
        for j, b in enumerate(gt.to(torch.int64).tolist()):
            masks[j, b[1]:b[3], b[0]:b[2]] = 1
        targets.append(dict(boxes=gt, labels=torch.randint(1, NCLS, (ng,), generator=g), masks=masks))
    return m, images, targets


def test_both_routes_agree_on_a_real_model(ops, model_batch):
    from seam_match_rcnn_amd import evaluator_det as E
    model, images, targets = model_batch
    dev_images = [im.to(DEV) for im in images]
    with torch.no_grad():
        default = model(dev_images)
        model.paste_masks = False
        try:
            lean = model(dev_images)
        finally:
            del model.paste_masks
    assert model.paste_masks is True
    assert sum(len(o["scores"]) for o in default) > 20
    for o, l, im in zip(default, lean, images):
        assert "masks" in o and "mask_probs" not in o and "mask_probs" in l and "masks" not in l
        for k in ("boxes", "labels", "scores"):
            assert torch.equal(o[k], l[k]), k
        assert tuple(l["mask_probs"].shape) == (len(o["scores"]), 1, 28, 28)
        assert torch.equal(ops.paste_masks(l["mask_probs"], l["boxes"], im.shape[-2:]), o["masks"])
    # random targets, plus per image one ground truth that IS a detection's mask (so that the numbers are not all zero)
    tg = []
    for t, o in zip(targets, default):
        k = int(torch.nonzero(o["labels"] > 0)[0])
        own = (o["masks"][k, 0] > 0.5).to(torch.uint8).cpu()
        tg.append(dict(boxes=torch.cat([t["boxes"], o["boxes"][k:k + 1].cpu()]), labels=torch.cat([t["labels"], o["labels"][k:k + 1].cpu()]),
                       masks=torch.cat([t["masks"], own[None]])))
    pasted = E.DetectionEvaluator()
    pasted.update(default, tg)
    want = pasted.summarize(verbose=False)
    got = E.evaluate(model, [(images, tg)], DEV, verbose=False)
    assert model.paste_masks is True and "paste_masks" not in vars(model)
    assert sorted(got) == ["bbox", "segm"] and all(len(v) == 12 for v in got.values())
    assert got["segm"] == want["segm"] and got["bbox"] == want["bbox"]
    assert max(got["segm"]) > 0 and max(got["bbox"]) > 0

    def broken():
        raise RuntimeError("loader broke")
        yield images, tg
    with pytest.raises(RuntimeError, match="loader broke"):
        E.evaluate(model, broken(), DEV, verbose=False)
    assert model.paste_masks is True and "paste_masks" not in vars(model)
