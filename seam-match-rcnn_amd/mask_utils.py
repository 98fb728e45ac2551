"""Ground-truth masks from COCO-style annotations, on the device: the counterpart of the reference's ``stuffs/mask_utils.py``
(a wrapper over ``pycocotools._mask``), for what ``datasets/DF2Dataset.py:152-155`` does with it.

The reference rasterises every object on a dataloader worker and ships the uint8 ``[n,H,W]`` stack to the device each step
(7.8 MB for 8 objects at 800 x 1216).  Here the annotations themselves go up -- a few KB of integers for a batch -- and
``csrc/seam_masks.hip`` builds the stacks where ``model(images, targets)`` and ``evaluator_det`` read them.  The arithmetic
restates ``maskApi.c`` (rleFrPoly, rleFrString, rleMerge, rleDecode) from the published procedure; it is not pinned against
pycocotools itself, which is not installed where this project is tested.

A ``segmentation`` entry is one of: a polygon list ``[[x0, y0, x1, y1, ...], ...]`` (several parts are merged), an uncompressed
RLE ``{"counts": [..], "size": [h, w]}``, or a compressed RLE ``{"counts": "<string>", "size": [h, w]}``.
Not here: ``encode``, ``area``, ``toBbox``, ``iou``.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import ops


def rle_from_string(s) -> list:
    """Compressed RLE string (or bytes) -> counts (``rleFrString``): per count, 5 bits per character from ``ord(ch) - 48``,
    bit 0x20 = another character follows, bit 0x10 of the last = sign; counts from the fourth on are deltas against the count
    two places before."""
    if isinstance(s, (bytes, bytearray)):
        s = bytes(s).decode("ascii")
    if not isinstance(s, str):
        raise ValueError(f"rle_from_string: expected str or bytes, got {type(s).__name__}")
    counts, x, k = [], 0, 0
    for ch in s:
        c = ord(ch) - 48
        if not 0 <= c < 64:
            raise ValueError(f"rle_from_string: character {ch!r} is outside the code's alphabet")
        x |= (c & 0x1F) << (5 * k)
        k += 1
        if c & 0x20:
            continue
        if c & 0x10:
            x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
        x, k = 0, 0
    if k:
        raise ValueError("rle_from_string: the string ends inside a count")
    return counts


def rle_to_string(counts: Sequence[int]) -> str:
    """counts -> compressed RLE string (``rleToString``); here so that the codec's round trip can be tested."""
    out = []
    for i, x in enumerate(counts):
        x = int(x) - (int(counts[i - 2]) if i > 2 else 0)
        while True:
            c = x & 0x1F
            x >>= 5
            more = x != (-1 if c & 0x10 else 0)
            out.append(chr((c | 0x20 if more else c) + 48))
            if not more:
                break
    return "".join(out)


def _split(segm, size, what: str):
    """One ``segmentation`` entry -> (polygon parts or None, RLE counts or None), both validated against ``size``."""
    h, w = int(size[0]), int(size[1])
    if isinstance(segm, dict):
        if "counts" not in segm:
            raise ValueError(f"{what}: an RLE segmentation needs 'counts'")
        if "size" in segm and [int(v) for v in segm["size"]] != [h, w]:
            raise ValueError(f"{what}: the RLE's size {list(segm['size'])} disagrees with the image size {[h, w]}")
        counts = segm["counts"]
        if isinstance(counts, (str, bytes, bytearray)):
            try:
                counts = rle_from_string(counts)
            except ValueError as e:
                raise ValueError(f"{what}: {e}") from e
        return None, counts
    if isinstance(segm, (list, tuple)):
        for q, part in enumerate(segm):
            if not isinstance(part, (list, tuple, np.ndarray)):
                raise ValueError(f"{what} part {q}: a polygon segmentation is a list of [x0, y0, x1, y1, ...] parts")
            if len(part) == 0 or len(part) % 2:
                raise ValueError(f"{what} part {q}: a polygon part needs a non-empty, even number of coordinates, got {len(part)}")
        return list(segm), None
    raise ValueError(f"{what}: segmentation must be a polygon list or an RLE dict, got {type(segm).__name__}")


def _segm(a):
    return a["segmentation"] if isinstance(a, dict) and "segmentation" in a else a


def masks_from_annotations(annos_per_image: Sequence[Sequence], sizes: Sequence[Sequence[int]], device) -> list:
    """``annos_per_image[i]``: image i's objects, each an annotation dict with ``"segmentation"`` or the segmentation entry
    itself; ``sizes[i] = (h, w)``.  Returns a list of uint8 0/1 ``[n_i,H_i,W_i]`` device tensors (views of one flat buffer):
    what ``torch.stack([annToMask(obj, size) for obj in anno])`` gives per image.  The whole batch is one table upload and one
    launch sequence per annotation form present.  ValueError (naming image and object) for an RLE whose counts do not sum to
    h*w, a dict size that disagrees with ``sizes[i]``, an odd-length or empty polygon part, non-finite coordinates."""
    if len(annos_per_image) != len(sizes):
        raise ValueError(f"masks_from_annotations: {len(annos_per_image)} images but {len(sizes)} sizes")
    polys, rles = [], []
    for i, (annos, size) in enumerate(zip(annos_per_image, sizes)):
        if len(size) != 2:
            raise ValueError(f"masks_from_annotations: image {i}: size must be (h, w)")
        pairs = [_split(_segm(a), size, f"masks_from_annotations: image {i} object {j}") for j, a in enumerate(annos)]
        polys.append([p for p, _ in pairs])
        rles.append([r for _, r in pairs])
    lay, rle_tables = ops.pack_rle_masks(rles, sizes)       # every ValueError is raised before the device is touched
    _, poly_tables = ops.pack_poly_masks(polys, sizes)
    flat = ops.mask_flat(lay, device)
    ops.launch_rle_masks(lay, rle_tables, device, flat)
    return ops.launch_poly_masks(lay, poly_tables, device, flat)


def annToMask(ann, size) -> np.ndarray:
    """The reference's ``annToMask(ann, size)``: ``ann["segmentation"]`` (polygons, uncompressed or compressed RLE) on an image of
    ``size = [h, w]`` -> NumPy uint8 ``[h,w]``, rasterised on the current HIP device."""
    return masks_from_annotations([[ann]], [size], torch.device("cuda"))[0][0].cpu().numpy()


def targets_to_device(targets: Sequence[dict], device) -> list:
    """What a training or evaluation loop writes instead of ``[{k: v.to(device) for k, v in t.items()} for t in targets]``
    (ref stuffs/engine.py:39) when the dataset hands over annotations instead of masks: tensors move to ``device``; a target's
    ``"segmentation"`` (one entry per object) and ``"size"`` (h, w) are replaced by ``"masks"``, uint8 ``[n,H,W]`` built on the
    device for the whole batch at once.  Other values pass through unchanged."""
    out = [{k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in t.items() if k not in ("segmentation", "size")}
           for t in targets]
    with_segm = [i for i, t in enumerate(targets) if "segmentation" in t]
    for i in with_segm:
        if "size" not in targets[i]:
            raise ValueError(f"targets_to_device: target {i} has 'segmentation' but no 'size' (h, w)")
    if with_segm:
        sizes = [[int(v) for v in targets[i]["size"]] for i in with_segm]
        masks = masks_from_annotations([targets[i]["segmentation"] for i in with_segm], sizes, device)
        for i, m in zip(with_segm, masks):
            out[i]["masks"] = m
    return out
