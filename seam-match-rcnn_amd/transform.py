"""The dataset transforms of the phase-1 loop, the counterpart of the reference's ``stuffs/transform.py`` without torchvision:
``Compose``, ``ToTensor`` and ``RandomHorizontalFlip`` on ``(image, target)`` pairs.

Two forms of an image pass through them.  The eager one is the reference's: ``ToTensor()`` makes the float CHW tensor
(bytes / 255) and the flip turns image, boxes and masks round on the host.  The lazy one (``ToTensor(lazy=True)``, or a dataset
built with ``lazy=True``) keeps the decoded bytes, uint8 ``[H,W,3]``: the flip then moves the boxes only and leaves
``target["hflip"] = True`` for ``input_pipeline.prepare_batch``, which flips image and masks inside its kernels.  Both forms draw
one ``random.random()`` per call, so a seeded run flips the same images either way.  Keypoints are not handled (DeepFashion2
targets carry none here).
"""
from __future__ import annotations

import random

import numpy as np
import torch


def _is_bytes(image) -> bool:
    return isinstance(image, torch.Tensor) and image.dtype == torch.uint8 and image.dim() == 3 and image.shape[2] == 3


def image_bytes(image) -> torch.Tensor:
    """A PIL image (any mode; converted to RGB) or a uint8 ``[H,W,3]`` tensor -> the uint8 ``[H,W,3]`` tensor of its RGB bytes."""
    if _is_bytes(image):
        return image
    if isinstance(image, torch.Tensor):
        raise ValueError(f"expected a PIL image or a uint8 [H,W,3] tensor, got a {image.dtype} tensor of shape {tuple(image.shape)}")
    return torch.from_numpy(np.array(image.convert("RGB"), dtype=np.uint8))


class Compose:
    """The steps applied in order; each takes and returns an ``(image, target)`` pair."""

    def __init__(self, transforms):
        self.transforms = list(transforms)

    def __call__(self, image, target):
        pair = (image, target)
        for step in self.transforms:
            pair = step(*pair)
        return pair


class ToTensor:
    """``ToTensor()``: what torchvision's ``to_tensor`` gives for an RGB image, float32 ``[3,H,W]`` = bytes / 255.
    ``ToTensor(lazy=True)``: the uint8 ``[H,W,3]`` bytes, for ``input_pipeline.prepare_batch``."""

    def __init__(self, lazy: bool = False):
        self.lazy = bool(lazy)

    def __call__(self, image, target):
        b = image_bytes(image)
        if self.lazy:
            return b, target
        return b.permute(2, 0, 1).float().div(255).contiguous(), target


class RandomHorizontalFlip:
    """With probability ``prob`` (one ``random.random()`` per call): mirror the sample left-right.  Boxes become
    ``(width - x2, y1, width - x1, y2)``, in place.  A float ``[3,H,W]`` image and dense ``"masks"`` are flipped here; a uint8
    ``[H,W,3]`` image keeps its bytes and the target's ``"hflip"`` is toggled instead (a MovingFashion frame with
    ``"frame_prep" == 2`` is still at full resolution there: its boxes are mirrored in the half-size image they refer to)."""

    def __init__(self, prob):
        self.prob = prob

    def __call__(self, image, target):
        if random.random() >= self.prob:
            return image, target
        lazy = _is_bytes(image)
        if lazy and "masks" in target:
            raise ValueError("RandomHorizontalFlip: a uint8 [H,W,3] image is flipped on the device, which needs the target's "
                             "'segmentation' instead of dense 'masks' (build the dataset with lazy=True)")
        width = image.shape[1] if lazy else image.shape[-1]
        if lazy and target.get("frame_prep") == 2:      # a MovingFashion frame still at full resolution: its boxes refer to half
            width //= 2
        boxes = target["boxes"]
        left = width - boxes[:, 2]
        boxes[:, 2] = width - boxes[:, 0]
        boxes[:, 0] = left
        if lazy:
            target["hflip"] = not target.get("hflip", False)
            return image, target
        if "masks" in target:
            target["masks"] = target["masks"].flip(-1)
        return image.flip(-1), target
