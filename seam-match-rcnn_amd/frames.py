"""Device-side frame preparation: the per-frame work of ``MovingFashionDataset.__getitem__``
(ref datasets/MFDataset.py:79-93) after ``cv2.VideoCapture.read()``.

The reference does this per frame on a dataloader worker: BGR->RGB, float64 noise over the full-resolution frame
(``np.random.randn`` of 6.2 M values for 1080p), clip, uint8, PIL bicubic resize to half size, ``ToTensor``.  Here the
decoded uint8 frame is uploaded once (1 byte per sample) and everything else runs on the GPU; the result is the uint8
RGB image the model's transform consumes directly (``seam_preprocess_u8`` fuses ToTensor + normalise + resize + pad).
Video decode itself stays with cv2 (out of scope: no decoder in this image).

``prepare_frame`` is the per-frame route (five launches and two intermediate images per frame); ``prepare_clip`` and
``prepare_frames`` (the batch of a lazy ``datasets.MFDataset.MovingFashionDataset``) do the same work for many frames of differing
sizes in one launch (``ops.frames_prepare_batch``, ``seam_frames_prepare_batch_u8``), bit for bit.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import ops


def noise_sigma(u: float) -> float:
    """``tmp_noise = 0.25 if random.random() > 0.75 else 0.05`` (ref MFDataset.py:82), with the draw made explicit."""
    return 0.25 if u > 0.75 else 0.05


@torch.no_grad()
def prepare_frame(bgr: torch.Tensor, noise: bool = True, sigma: float = 0.05, seed: int = 0,
                  noise_values: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Decoded frame uint8 [H,W,3] BGR (device) -> uint8 RGB: noisy and half resolution when ``noise`` (the training /
    default test setting), otherwise the plain channel flip.  ``noise_values``: optional float64 [H,W,3] standard-normal
    draws (bit-exact with the NumPy pipeline given the same draws); default: on-device draws keyed by ``seed``."""
    if not noise:
        return ops.frame_noise(bgr, 0.0)
    rgb = ops.frame_noise(bgr, sigma, noise_values, seed)
    return ops.resize_bicubic_u8(rgb, bgr.shape[0] // 2, bgr.shape[1] // 2)


@torch.no_grad()
def prepare_clip(frames, noise: bool = True, sigmas=None, seed: int = 0):
    """A list of decoded frames -> list of uint8 RGB images ready for ``model(images)`` (which accepts uint8 HWC).  Frame ``i``
    gets ``prepare_frame(f, noise, sigmas[i], seed + 7919 * i)``; frames that all lie on one HIP device take the batched launch
    (``ops.frames_prepare_batch``: the same bytes, one launch for the clip)."""
    frames = list(frames)
    sig = [0.05 if sigmas is None else sigmas[i] for i in range(len(frames))]
    seeds = [seed + 7919 * i for i in range(len(frames))]
    batched = bool(frames) and all(isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.uint8 and f.dim() == 3
                                   and f.shape[2] == 3 and min(f.shape[0], f.shape[1]) >= 2 and f.device == frames[0].device
                                   for f in frames)
    if not batched:
        return [prepare_frame(f, noise, s, sd) for f, s, sd in zip(frames, sig, seeds)]
    mode = ops.FRAME_NOISY_HALF if noise else ops.FRAME_RGB
    return ops.frames_prepare_batch(frames, [mode] * len(frames), sig if noise else [0.0] * len(frames), seeds)


FRAME_KEYS = ("frame_prep", "frame_sigma", "frame_seed")


def frame_args(targets):
    """``(modes, sigmas, seeds)`` of a lazy ``MovingFashionDataset`` batch for ``ops.frames_prepare_batch``; a target without
    ``"frame_prep"`` is an image that stays as it is."""
    modes = [int(t.get("frame_prep", ops.FRAME_AS_IS)) for t in targets]
    return modes, [float(t.get("frame_sigma", 0.0)) for t in targets], [int(t.get("frame_seed", 0)) for t in targets]


@torch.no_grad()
def prepare_frames(images, targets, device):
    """uint8 ``[H,W,3]`` images and the targets of a lazy ``datasets.MFDataset.MovingFashionDataset`` -> (the prepared uint8 RGB
    images on ``device``, the targets without ``"frame_prep"`` / ``"frame_sigma"`` / ``"frame_seed"``): one copy and one launch
    (``ops.frames_prepare_batch``).  For callers that feed the model lists: the evaluator's chunks and the fp16 compute dtype,
    where ``input_pipeline.prepare_images`` refuses."""
    images, targets = list(images), list(targets)
    if len(images) != len(targets):
        raise ValueError("one target dict per image is needed")
    modes, sigmas, seeds = frame_args(targets)
    out = ops.frames_prepare_batch(images, modes, sigmas, seeds, device=device)
    return out, [{k: v for k, v in t.items() if k not in FRAME_KEYS} for t in targets]
