"""GPU: ``input_pipeline.prepare_batch`` in front of ``model(images, targets)`` -- the device-side input path of a training step --
against the eager route, bit for bit.

The model, ``ROI_BATCH`` and the seeding are those of tests/test_gpu_body_train_model.py (``min_size=256, max_size=320``, two
images 200 x 250 and 192 x 240, ``sample_generator`` seeds 1 and 2); here the images are uint8 and the ground truths polygons,
and the first image is flipped.  Route A is the eager one: host ``ToTensor`` and flip, dense masks flipped at original size,
``.to(device)``, ``model(images, targets)``.  Route B is ``prepare_batch``.  The six losses and every parameter gradient must be
equal with ``torch.equal``."""
import copy
import random

import numpy as np
import pytest
import torch

import df2_fixture as FX
import rpn_train_refs as PR
from seam_match_rcnn_amd import mask_utils
from seam_match_rcnn_amd.datasets.DF2Dataset import DeepFashion2Dataset, get_dataloader     # the feature: absent, no import
from seam_match_rcnn_amd.input_pipeline import prepare_batch, prepare_images
from seam_match_rcnn_amd.models import detection as det
from seam_match_rcnn_amd.models.matchrcnn import resize_masks_nearest
from seam_match_rcnn_amd.transform import Compose, RandomHorizontalFlip, ToTensor

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NCLS = 14
ROI_BATCH = 64
SIX = ["loss_classifier", "loss_box_reg", "loss_mask", "loss_match", "loss_objectness", "loss_rpn_box_reg"]
FLIPS = [True, False]


def make_model(layers=3):
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS, min_size=256, max_size=320,
                               trainable_backbone_layers=layers, **params)
    sd = synth.detector_state(5, NCLS)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    m.roi_heads.batch_size_per_image = ROI_BATCH
    return m.to(DEV).train()


def lazy_batch(seed=0):
    """Two uint8 images with polygon ground truths, as a lazy dataset hands them over (nothing flipped yet)."""
    g = torch.Generator().manual_seed(seed)
    rng = np.random.RandomState(7)
    images, targets = [], []
    for i, (h, w) in enumerate(((200, 250), (192, 240))):
        images.append(torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)))
        ng = 2 + i
        gt = PR.random_gt(g, ng, h, w, 30, 120)
        segm = []
        for x1, y1, x2, y2 in gt.tolist():                              # a hexagon inside the box, and for one object a second part
            xm, ym = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
            parts = [[x1, ym, 0.5 * (x1 + xm), y1, 0.5 * (xm + x2), y1, x2, ym, 0.5 * (xm + x2), y2, 0.5 * (x1 + xm), y2]]
            if not segm:
                parts.append([x1, y1, xm, y1, x1, ym])
            segm.append(parts)
        targets.append(dict(boxes=gt.clone(), labels=torch.randint(1, NCLS, (ng,), generator=g), segmentation=segm, size=(h, w),
                            pair_ids=torch.randint(0, 3, (ng,), generator=g), styles=torch.randint(1, 3, (ng,), generator=g),
                            sources=torch.tensor([i])))
    return images, targets


def eager_route(images, targets):
    """The reference's host side: dense masks, ToTensor, the flip of image, boxes and masks, then the two ``.to(device)`` lines."""
    dense = mask_utils.masks_from_annotations([t["segmentation"] for t in targets], [t["size"] for t in targets], DEV)
    out_i, out_t = [], []
    for img, t, m, f in zip(images, targets, dense, FLIPS):
        t = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in t.items() if k not in ("segmentation", "size")}
        t["masks"] = m.cpu()
        x, t = ToTensor()(img, t)
        if f:
            x, t = RandomHorizontalFlip(1.0)(x, t)
        out_i.append(x.to(DEV))
        out_t.append({k: (v.to(DEV) if torch.is_tensor(v) else v) for k, v in t.items()})
    return out_i, out_t


def lazy_route(images, targets):
    out_i, out_t = [], []
    for img, t, f in zip(images, targets, FLIPS):
        t = {k: (v.clone() if torch.is_tensor(v) else copy.deepcopy(v)) for k, v in t.items()}
        x, t = ToTensor(lazy=True)(img, t)
        if f:
            x, t = RandomHorizontalFlip(1.0)(x, t)
        out_i.append(x)
        out_t.append(t)
    return out_i, out_t


def run_model(m, images, targets):
    m.rpn.sample_generator = torch.Generator(device=DEV).manual_seed(1)
    m.roi_heads.sample_generator = torch.Generator(device=DEV).manual_seed(2)
    m.zero_grad(set_to_none=True)
    losses = m(images, targets)
    assert list(losses) == SIX
    sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
    grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
    return {k: v.detach().clone() for k, v in losses.items()}, grads


@pytest.fixture(scope="module")
def runs():
    m = make_model(3)
    images, targets = lazy_batch()
    ea_i, ea_t = eager_route(images, targets)
    la_i, la_t = lazy_route(images, targets)
    prepared, pt = prepare_batch(la_i, la_t, DEV, m)
    a = run_model(m, ea_i, ea_t)
    b = run_model(m, prepared, pt)
    return dict(model=m, eager=(ea_i, ea_t), lazy=(la_i, la_t), prepared=(prepared, pt), a=a, b=b)


def test_prepared_batch_is_the_transform_of_the_eager_images(runs):
    m = runs["model"]
    prepared, pt = runs["prepared"]
    ea_i, ea_t = runs["eager"]
    with torch.no_grad():
        x, sizes, orig, padded = m.transform(ea_i)
    assert len(prepared) == 2 and prepared.sizes == list(sizes) and prepared.orig == list(orig) and prepared.padded == tuple(padded)
    assert (prepared.min_size, prepared.max_size, prepared.size_divisible) == (256, 320, 32)
    assert prepared.tensor.shape == x.shape and torch.equal(prepared.tensor, x)
    for t, e, s in zip(pt, ea_t, sizes):
        assert "segmentation" not in t and "size" not in t and "hflip" not in t
        assert torch.equal(t["boxes"], e["boxes"]) and t["boxes"].device.type == "cuda"      # original-image pixels, flipped
        assert tuple(t["masks"].shape[1:]) == tuple(s)
        assert torch.equal(t["masks"], resize_masks_nearest(e["masks"], s))
        assert bool(t["masks"].any())
        assert resize_masks_nearest(t["masks"], s) is t["masks"]                                # the model passes them through


def test_losses_and_gradients_equal_the_eager_route(runs):
    (la, ga), (lb, gb) = runs["a"], runs["b"]
    for k in SIX:
        print(k, float(la[k]), float(lb[k]))
        assert torch.equal(la[k], lb[k]) or (bool(torch.isnan(la[k])) and bool(torch.isnan(lb[k]))), k
    assert all(bool(torch.isfinite(la[k])) for k in SIX if k != "loss_match")
    assert ga.keys() == gb.keys() and len(ga) > 60
    for k in ga:
        assert torch.equal(ga[k], gb[k]), k
    assert any(k.startswith("backbone.body.layer2") for k in ga)


def test_original_size_masks_are_what_the_evaluator_reads(runs):
    la_i, la_t = runs["lazy"]
    _, ea_t = runs["eager"]
    prepared, pt = prepare_batch(la_i, la_t, DEV, runs["model"], masks="original")
    assert torch.equal(prepared.tensor, runs["prepared"][0].tensor)
    for t, e, (h, w) in zip(pt, ea_t, ((200, 250), (192, 240))):
        assert "segmentation" not in t and "hflip" not in t
        assert tuple(t["masks"].shape[1:]) == (h, w) and torch.equal(t["masks"], e["masks"])
        assert torch.equal(t["boxes"], e["boxes"])
    with pytest.raises(ValueError):
        prepare_batch(la_i, la_t, DEV, runs["model"], masks="half")


def test_prepared_images_for_other_settings_are_refused(runs):
    m = runs["model"]
    prepared, pt = runs["prepared"]
    m.transform.min_size = 224
    try:
        with pytest.raises(ValueError, match="min_size"):
            m(prepared, pt)
        with pytest.raises(ValueError, match="min_size"):
            m.extract_features(prepared)
    finally:
        m.transform.min_size = 256
    other = det.PreparedImages(prepared.tensor, prepared.sizes, prepared.orig, prepared.padded, 256, 320, 32, not prepared.s2d)
    with pytest.raises(ValueError, match="layout"):
        m.transform(other)
    det.set_compute_dtype(m, torch.float16)
    try:
        with pytest.raises(NotImplementedError, match="seam_preprocess_u8"):
            prepare_batch(*runs["lazy"], DEV, m)
    finally:
        det.set_compute_dtype(m, torch.float32)
    with pytest.raises(ValueError):
        prepare_batch([i.float() for i in runs["lazy"][0]], runs["lazy"][1], DEV, m)
    with pytest.raises(ValueError):
        prepare_batch(runs["lazy"][0][:1], runs["lazy"][1], DEV, m)


def test_eval_forward_takes_a_prepared_batch(runs):
    m = runs["model"]
    ea_i, _ = runs["eager"]
    m.eval()
    try:
        with torch.no_grad():
            want = m(ea_i)
            got = m(prepare_images(runs["lazy"][0], DEV, m, FLIPS))
    finally:
        m.train()
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_one_pass_of_the_loop_over_the_dataloader(tmp_path):
    ann_file, root = FX.write(tmp_path)
    ds = DeepFashion2Dataset(ann_file, root, Compose([ToTensor(lazy=True), RandomHorizontalFlip(0.5)]), lazy=True)
    random.seed(2)
    torch.manual_seed(2)
    m = make_model(3)
    m.rpn.sample_generator = torch.Generator(device=DEV).manual_seed(1)
    m.roi_heads.sample_generator = torch.Generator(device=DEV).manual_seed(2)
    opt = torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.01, momentum=0.9)
    watched = {k: p.detach().clone() for k, p in m.named_parameters()
               if k in ("rpn.head.conv.weight", "roi_heads.mask_predictor.mask_fcn_logits.weight", "backbone.body.layer2.0.conv1.weight")}
    assert len(watched) == 3
    images, targets, ids = next(iter(get_dataloader(ds, 2, False)))
    assert ids[0] in ds.street_inds and ids[1] in ds.shop_inds
    prepared, pt = prepare_batch(images, targets, DEV, m)
    losses = m(prepared, pt)
    assert list(losses) == SIX
    for k in SIX:
        print(k, float(losses[k].detach()))
        assert bool(torch.isfinite(losses[k])), k
    opt.zero_grad()
    sum(losses.values()).backward()
    opt.step()
    now = dict(m.named_parameters())
    for k, before in watched.items():
        assert bool(torch.isfinite(now[k]).all()) and not torch.equal(now[k].detach(), before), k
