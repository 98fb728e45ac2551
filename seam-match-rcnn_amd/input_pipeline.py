"""The input stage of a phase-1 training step on the device: what the reference's loop does between the dataloader and the model
(``stuffs/engine.py:38-39``, two ``.to(device)`` lines behind a dataset that has already run ``to_tensor``, the flip and
``annToMask`` on the host), for a batch from a lazy ``datasets.DF2Dataset.DeepFashion2Dataset``::

    for images, targets, ids in get_dataloader(dataset, batch_size, is_parallel):
        images, targets = prepare_batch(images, targets, device, model)
        loss_dict = model(images, targets)

The batch crosses the bus as image bytes (3 per pixel instead of the 12 of a float CHW image) and a few KB of annotation integers.
One launch (``ops.preprocess_u8_batch``) does ToTensor + flip + normalise + resize + pad + layout for all the images, whatever their
sizes; one launch sequence (``mask_utils.masks_from_annotations_resized``) writes the flipped ground-truth masks at the resized
size.  Both are the bits of the eager route (tests/test_gpu_train_input_model.py), which keeps working.

A phase-2 batch from a lazy ``datasets.MultiDF2Dataset.MultiDeepFashion2Dataset`` carries ``"noise_sigma"`` / ``"noise_seed"`` in
its targets: the reference's per-image host noise then runs as one launch (``seam_noise_u8_batch``) on the staged bytes, before
the preprocess launch reads them, in the same copy and on the same stream.  ``apply_noise`` is that launch alone, for callers that
hand the model lists of images.

A phase-3 batch from a lazy ``datasets.MFDataset.MovingFashionDataset`` carries ``"frame_prep"`` / ``"frame_sigma"`` /
``"frame_seed"``: the decoded frames cross the bus at full resolution, and the reference's per-frame host work (BGR -> RGB, noise,
PIL resize to half size) runs as one launch (``seam_frames_prepare_batch_u8``) in front of the preprocess launch, which reads its
output buffer; both tables travel in the batch's one copy.  ``frames.prepare_frames`` is that launch alone.
"""
from __future__ import annotations

import math
from typing import Sequence

import torch

from . import frames as frames_mod
from . import mask_utils, ops
from .models import detection as det
from .models.detection import PreparedImages  # noqa: F401  (the public name lives here)

_LAZY_KEYS = ("segmentation", "size", "hflip")
_NOISE_KEYS = ("noise_sigma", "noise_seed")
_FRAME_KEYS = frames_mod.FRAME_KEYS


def _noise_of(targets):
    """``(sigmas, seeds)`` for ``ops`` when any target carries ``"noise_sigma"`` (a target without it: sigma 0), else None."""
    if not any("noise_sigma" in t for t in targets):
        return None
    return [float(t.get("noise_sigma", 0.0)) for t in targets], [int(t.get("noise_seed", 0)) for t in targets]


def _without(t: dict, keys) -> dict:
    return {k: v for k, v in t.items() if k not in keys}


def apply_noise(images: Sequence[torch.Tensor], targets: Sequence[dict], device):
    """uint8 ``[H,W,3]`` images and the targets of a lazy ``MultiDeepFashion2Dataset`` -> (the noisy uint8 images on ``device``,
    the targets without ``"noise_sigma"`` / ``"noise_seed"``), one copy and one launch (``ops.noise_u8_batch``).  For callers that
    feed the model lists: the fp16 compute dtype, where ``prepare_images`` refuses, and the evaluator's chunks of 6."""
    images, targets = list(images), list(targets)
    if len(images) != len(targets):
        raise ValueError("one target dict per image is needed")
    sigmas, seeds = _noise_of(targets) or ([0.0] * len(targets), [0] * len(targets))
    return ops.noise_u8_batch(images, sigmas, seeds, device=device), [_without(t, _NOISE_KEYS) for t in targets]


def prepare_images(images: Sequence[torch.Tensor], device, model, flips=None, noise=None, frames=None) -> PreparedImages:
    """uint8 ``[H,W,3]`` images (host or device) -> the batch ``model.transform`` would build from ``to_tensor`` of them (flipped
    where ``flips[i]``) for the model's current ``min_size`` / ``max_size`` / ``size_divisible`` and stem form, in one launch.
    ``noise`` = ``(sigmas, seeds)``: the images are first given the noise ``ops.noise_u8_batch`` gives them, one launch more.
    ``frames`` = ``(modes, sigmas, seeds)``: the images are first prepared as ``ops.frames_prepare_batch`` prepares them, one
    launch more, and ``orig`` holds the sizes after that (halved for mode 2)."""
    tr = model.transform
    if det.adt(tr) != torch.float32:
        raise NotImplementedError("prepare_batch writes fp32 batches only (training is fp32 only); with an fp16 compute dtype hand "
                                  "the uint8 [H,W,3] images to the model as a list: the per-image uint8 path (seam_preprocess_u8)")
    images = list(images)
    if not images:
        raise ValueError("prepare_batch: empty image list")
    if not all(isinstance(i, torch.Tensor) and i.dtype == torch.uint8 and i.dim() == 3 and i.shape[2] == 3 for i in images):
        raise ValueError("prepare_batch: the images must be uint8 [H,W,3] tensors (a dataset built with lazy=True / ToTensor(lazy=True))")
    d = tr.size_divisible
    s2d = tr.prepared_s2d()

    def plan(orig):
        sizes = [det.resized_size(h, w, tr.min_size, tr.max_size)[:2] for h, w in orig]
        return sizes, int(math.ceil(max(s[0] for s in sizes) / d) * d), int(math.ceil(max(s[1] for s in sizes) / d) * d)

    if frames is not None:
        if noise is not None:
            raise ValueError("prepare_batch: a batch carries frame keys or noise keys, not both")
        flips = [False] * len(images) if flips is None else [bool(f) for f in flips]
        if len(flips) != len(images):
            raise ValueError("prepare_batch: one flip per image is needed")
        modes = list(frames[0])
        if len(modes) != len(images):
            raise ValueError("prepare_batch: one mode per image is needed")
        orig = [ops.frame_out_size(i.shape[0], i.shape[1], m) for i, m in zip(images, modes)]
        if any(min(z) < 1 for z in orig):
            raise ValueError("prepare_batch: a frame that is halved needs at least 2 x 2 pixels")
        sizes, hp, wp = plan(orig)
        # the preprocess launch's table is staged with the frames launch's: one copy for both
        pre_dims = [(o[0], o[1], z[0], z[1], int(f)) for o, z, f in zip(orig, sizes, flips)]
        st = ops.stage_frames("prepare_batch", images, *frames, device, pre_dims=pre_dims)
        x = ops.preprocess_u8_flat(ops.launch_frames(st), st.out_off, st.pre_dims, hp, wp, s2d)
        return PreparedImages(x, sizes, orig, (hp, wp), tr.min_size, tr.max_size, d, s2d)
    orig = [(int(i.shape[0]), int(i.shape[1])) for i in images]
    sizes, hp, wp = plan(orig)
    x = ops.preprocess_u8_batch(images, sizes, hp, wp, flips, s2d, device=device, noise=noise)
    return PreparedImages(x, sizes, orig, (hp, wp), tr.min_size, tr.max_size, d, s2d)


def prepare_batch(images: Sequence[torch.Tensor], targets: Sequence[dict], device, model, masks: str = "resized"):
    """(images, targets) of a lazy dataset -> (``PreparedImages``, targets on ``device``) for ``model(images, targets)``.

    A target's ``"hflip"`` (set by ``transform.RandomHorizontalFlip`` on a uint8 image, whose bytes it leaves alone) flips the
    image inside the preprocess launch; its boxes are flipped already and stay in original-image pixels (the model rescales
    them).  ``"segmentation"`` + ``"size"`` become ``"masks"``: ``masks="resized"`` -- flipped, at the size the transform
    resizes the image to, which ``resize_masks_nearest`` passes through (training); ``masks="original"`` -- flipped at the
    image's own size, through ``targets_to_device`` and a device flip (what ``evaluator_det`` reads); ``masks="none"`` -- both keys
    are dropped and nothing is rasterised (phase 2's loops and ``evaluator_df2`` read boxes only).  ``"noise_sigma"`` /
    ``"noise_seed"`` (a lazy ``MultiDeepFashion2Dataset``) put the noise launch in front of the preprocess launch and are
    dropped.  ``"frame_prep"`` / ``"frame_sigma"`` / ``"frame_seed"`` (a lazy ``MovingFashionDataset``; ``masks="none"`` is the
    natural setting, its targets have no ``"segmentation"``) put the frames launch there instead and are dropped;
    ``PreparedImages.orig`` then holds the sizes after halving, which the boxes refer to.  A batch that mixes frame keys with
    ``"noise_sigma"`` raises ValueError.  Other tensors move to ``device``; other values pass through."""
    if masks not in ("resized", "original", "none"):
        raise ValueError('prepare_batch: masks must be "resized", "original" or "none"')
    images, targets = list(images), list(targets)
    if len(images) != len(targets):
        raise ValueError("one target dict per image is needed")
    flips = [bool(t.get("hflip", False)) for t in targets]
    with_frames = any("frame_prep" in t for t in targets)
    if with_frames and any("noise_sigma" in t for t in targets):
        raise ValueError("prepare_batch: a batch carries frame keys (MovingFashion) or noise keys (Multi-DeepFashion2), not both")
    prepared = prepare_images(images, device, model, flips, _noise_of(targets), frames_mod.frame_args(targets) if with_frames else None)
    targets = [_without(t, _NOISE_KEYS + _FRAME_KEYS) for t in targets]
    device = prepared.tensor.device
    for i, (t, o) in enumerate(zip(targets, prepared.orig)):
        if "segmentation" in t and "size" not in t:
            raise ValueError(f"prepare_batch: target {i} has 'segmentation' but no 'size' (h, w)")
        if "size" in t and tuple(int(v) for v in t["size"]) != o:
            raise ValueError(f"prepare_batch: target {i}: size {tuple(t['size'])} is not the image's {o}")
    if masks == "original":
        out = mask_utils.targets_to_device([{k: v for k, v in t.items() if k != "hflip"} for t in targets], device)
        for t, f in zip(out, flips):
            if f and "masks" in t:
                t["masks"] = t["masks"].flip(-1)
        return prepared, out
    out = [{k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in t.items() if k not in _LAZY_KEYS} for t in targets]
    with_segm = [i for i, t in enumerate(targets) if "segmentation" in t]
    if with_segm and masks == "resized":
        stacks = mask_utils.masks_from_annotations_resized([targets[i]["segmentation"] for i in with_segm],
                                                           [prepared.orig[i] for i in with_segm],
                                                           [prepared.sizes[i] for i in with_segm], [flips[i] for i in with_segm], device)
        for i, m in zip(with_segm, stacks):
            out[i]["masks"] = m
    return prepared, out
