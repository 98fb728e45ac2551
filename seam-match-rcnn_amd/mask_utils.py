"""COCO masks on the device, both directions: the counterpart of the reference's ``stuffs/mask_utils.py`` (a wrapper over
``pycocotools._mask``).  Annotations -> masks is what ``datasets/DF2Dataset.py:152-155`` does with it; masks -> RLE is what a
COCO results file needs (``evaluator_det.coco_results``).

The reference rasterises every object on a dataloader worker and ships the uint8 ``[n,H,W]`` stack to the device each step
(7.8 MB for 8 objects at 800 x 1216).  Here the annotations themselves go up -- a few KB of integers for a batch -- and
``csrc/seam_masks.hip`` builds the stacks where ``model(images, targets)`` and ``evaluator_det`` read them.  The arithmetic
restates ``maskApi.c`` (rleFrPoly, rleFrString, rleMerge, rleDecode) from the published procedure; it is not pinned against
pycocotools itself, which is not installed where this project is tested.

A ``segmentation`` entry is one of: a polygon list ``[[x0, y0, x1, y1, ...], ...]`` (several parts are merged), an uncompressed
RLE ``{"counts": [..], "size": [h, w]}``, or a compressed RLE ``{"counts": "<string>", "size": [h, w]}``.

The other direction: ``encode`` (dense masks, NumPy or device) and ``encode_detections`` (28x28 probabilities and boxes, no pasted
mask) run ``csrc/seam_rle.hip`` and bring a few hundred integers per object to the host, where ``counts_to_bytes`` writes the
compressed strings with vectorised NumPy; ``decode``, ``area``, ``toBbox``, ``annToRLE`` and ``iou`` complete the reference's
module.  A pixel is set iff its byte is non-zero (pycocotools' ``encode`` agrees for bytes 0/1 only).

``merge``, ``frPyObjects`` and ``iou`` on RLEs work on bitmaps of one bit per pixel (``ops.rle_bits`` straight from the run lists,
``ops.bits_combine``, ``ops.bits_to_rle``, ``ops.bits_inter``): no dense mask is written for an RLE operation.  Like the rest of
the module they are held by restatements of the published procedure (tests/rle_algebra_refs.py), not pinned against pycocotools.
"""
from __future__ import annotations

from typing import Sequence

import numpy as np
import torch

from . import ops, ops_masks


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
    lay, rle_tables, poly_tables = _pack_annotations(annos_per_image, sizes)
    flat = ops.mask_flat(lay, device)
    ops.launch_rle_masks(lay, rle_tables, device, flat)
    return ops.launch_poly_masks(lay, poly_tables, device, flat)


def _pack_annotations(annos_per_image, sizes, who: str = "masks_from_annotations"):
    """(layout, RLE tables, polygon tables) of a batch of annotations; every ValueError is raised before the device is touched and
    names ``who``, the public function that was called."""
    if len(annos_per_image) != len(sizes):
        raise ValueError(f"{who}: {len(annos_per_image)} images but {len(sizes)} sizes")
    polys, rles = [], []
    for i, (annos, size) in enumerate(zip(annos_per_image, sizes)):
        if len(size) != 2:
            raise ValueError(f"{who}: image {i}: size must be (h, w)")
        pairs = [_split(_segm(a), size, f"{who}: image {i} object {j}") for j, a in enumerate(annos)]
        polys.append([p for p, _ in pairs])
        rles.append([r for _, r in pairs])
    lay, rle_tables = ops.pack_rle_masks(rles, sizes)
    _, poly_tables = ops.pack_poly_masks(polys, sizes)
    return lay, rle_tables, poly_tables


def masks_from_annotations_resized(annos_per_image: Sequence[Sequence], sizes: Sequence[Sequence[int]],
                                   out_sizes: Sequence[Sequence[int]], flips, device) -> list:
    """``masks_from_annotations`` for a training step: image i's stack comes out at ``out_sizes[i]`` (the size the model's
    transform resizes the image to), flipped left-right where ``flips[i]`` -- uint8 ``[n_i, *out_sizes[i]]``, bit for bit
    ``resize_masks_nearest(stack.flip(-1) if flip else stack, out_size)`` of what ``masks_from_annotations`` returns, without
    writing the original-size stack (``seam_poly_masks_resized_u8`` / ``seam_rle_masks_resized_u8``)."""
    lay, rle_tables, poly_tables = _pack_annotations(annos_per_image, sizes, "masks_from_annotations_resized")
    out_lay, _ = ops.resized_mask_layout(lay, out_sizes, flips)
    flat = ops.mask_flat(out_lay, device)
    ops.launch_rle_masks_resized(lay, rle_tables, out_sizes, flips, device, flat)
    return ops.launch_poly_masks_resized(lay, poly_tables, out_sizes, flips, device, flat)


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


# ------------------------------------------------------------------------------------------------ masks -> RLE
def counts_to_bytes(counts_per_object: Sequence) -> list:
    """``rle_to_string`` for a batch of counts arrays at once, as ASCII bytes, without a Python loop per character.  A value
    (a count; from the fourth of an object on, its difference to the count two places before) takes the fewest 5-bit groups
    that hold it as a signed number; group g of all values that have one is computed and stored in one pass, with 0x20 added
    unless it is the value's last, so the loop runs seven times at the most for 32-bit counts."""
    arrs = [np.asarray(c, dtype=np.int64).reshape(-1) for c in counts_per_object]
    if not arrs:
        return []
    lens = np.asarray([a.size for a in arrs], np.int64)
    x = np.concatenate(arrs)
    starts = np.cumsum(lens) - lens
    idx = np.arange(x.size, dtype=np.int64) - np.repeat(starts, lens)
    prev2 = np.concatenate([np.zeros(2, np.int64), x])[:x.size]
    x = x - np.where(idx > 2, prev2, 0)
    mag = np.where(x < 0, ~x, x)                                     # fits n groups iff mag < 2^(5n-1)
    if x.size and int(mag.max()) < 2 ** 31:
        x, mag = x.astype(np.int32), mag.astype(np.int32)            # the usual case, half the bytes to move
    n = np.ones(x.size, np.int64)
    for g in range(1, 13):
        over = mag >= (1 << (5 * g - 1))
        if not over.any():
            break
        n += over
    first = np.cumsum(n) - n                                         # each value's first character
    out = np.empty(int(n.sum()), np.uint8)
    sel, xs, ns, g = first, x, n, 0
    while sel.size:                                                  # group g of every value that has one
        out[sel + g] = ((xs >> (5 * g)) & 0x1F) + np.where(ns - 1 > g, 0x20 + 48, 48)
        g += 1
        more = ns > g
        sel, xs, ns = sel[more], xs[more], ns[more]
    blob = out.tobytes()
    char_end = np.concatenate([[0], np.cumsum(n)])[starts + lens]    # characters up to each object's last count
    return [blob[lo:hi] for lo, hi in zip(np.concatenate([[0], char_end[:-1]]).tolist(), char_end.tolist())]


def _rle_dicts(counts_per_object, sizes) -> list:
    return [{"size": [int(h), int(w)], "counts": c} for c, (h, w) in zip(counts_to_bytes(counts_per_object), sizes)]


def encode(bimask):
    """The reference's ``encode``: NumPy uint8 ``[h,w]`` -> one RLE dict ``{"size": [h, w], "counts": <compressed bytes>}``,
    ``[h,w,n]`` (any memory order) -> a list of n.  A uint8 device tensor ``[n,H,W]`` (or ``[H,W]``) is encoded where it lies,
    without a copy to the host.  A pixel is set iff its byte is non-zero."""
    if isinstance(bimask, torch.Tensor):
        if bimask.dtype != torch.uint8 or bimask.dim() not in (2, 3):
            raise ValueError("encode: a device mask must be uint8 [n,H,W] or [H,W]")
        single = bimask.dim() == 2
        stack = (bimask[None] if single else bimask).contiguous()
    else:
        m = np.asarray(bimask)
        if m.dtype != np.uint8 or m.ndim not in (2, 3):
            raise ValueError("encode: a mask must be uint8 [h,w] or [h,w,n]")
        single = m.ndim == 2
        m = m[:, :, None] if single else m
        stack = torch.from_numpy(np.ascontiguousarray(m.transpose(2, 0, 1))).to(torch.device("cuda"))
    n, h, w = (int(v) for v in stack.shape)
    lay = ops.mask_layout([n], [(h, w)])
    out = _rle_dicts(ops.rle_encode(stack.reshape(-1), lay), [(h, w)] * n)
    return out[0] if single else out


def encode_detections(mask_probs: torch.Tensor, boxes: torch.Tensor, size) -> list:
    """The detections of one image as RLE dicts, straight from what the model returns with ``paste_masks = False``:
    ``mask_probs`` [K,1,28,28], ``boxes`` [K,4] in pixels of the ``size = (h, w)`` image.  Equal to
    ``encode(paste_masks(mask_probs, boxes, size) > 0.5)`` bit for bit; no pasted mask is written (``ops.rle_encode_paste``)."""
    h, w = int(size[0]), int(size[1])
    counts = ops.rle_encode_paste(mask_probs, boxes.to(torch.float32), (h, w))
    return _rle_dicts(counts, [(h, w)] * len(counts))


# ------------------------------------------------------------------------------------------------ RLE -> everything else
def _as_list(rles):
    return (rles, False) if isinstance(rles, list) else ([rles], True)


def _counts(rle, what: str) -> np.ndarray:
    h, w = (int(v) for v in rle["size"])
    _, counts = _split(rle, (h, w), what)
    return np.asarray(counts, dtype=np.int64).reshape(-1)


def decode(rleObjs, keep_on_device: bool = False):
    """The reference's ``decode``: one RLE dict -> NumPy uint8 ``[h,w]``; a list of n (of one size) -> ``[h,w,n]`` in Fortran
    order.  Rasterised on the device by ``rle_masks``; ``keep_on_device`` returns the uint8 ``[n,H,W]`` tensor instead."""
    rles, single = _as_list(rleObjs)
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"decode: the RLEs of one call must share a size, got {sorted(sizes)}")
    if not rles:
        raise ValueError("decode: needs at least one RLE")
    size = sizes.pop()
    stack = ops.rle_masks([[_counts(r, f"decode: object {j}") for j, r in enumerate(rles)]], [size], torch.device("cuda"))[0]
    if keep_on_device:
        return stack
    m = np.asfortranarray(stack.cpu().numpy().transpose(1, 2, 0))
    return m[:, :, 0] if single else m


def area(rleObjs):
    """Set pixels of each RLE (``rleArea``: the odd-indexed counts), uint32."""
    rles, single = _as_list(rleObjs)
    a = np.asarray([_counts(r, f"area: object {j}")[1::2].sum() for j, r in enumerate(rles)], dtype=np.uint32)
    return a[0] if single else a


def toBbox(rleObjs):
    """Tight ``[x, y, w, h]`` of each RLE's set pixels, float64 (``rleToBbox``): from the counts, on the host.  ``[0,0,0,0]`` for
    an empty mask; a run of ones that reaches into the next column makes the box full height."""
    rles, single = _as_list(rleObjs)
    out = np.zeros((len(rles), 4), dtype=np.float64)
    for j, r in enumerate(rles):
        h = int(r["size"][0])
        c = _counts(r, f"toBbox: object {j}")
        m = (c.size // 2) * 2
        if m == 0:
            continue
        t = np.cumsum(c[:m]) - (np.arange(m) & 1)                     # first pixel of a run of ones, last pixel of it
        y, x = t % h, t // h
        ys, ye = int(y.min()), int(y.max())
        if (x[0::2] < x[1::2]).any():
            ys, ye = 0, h - 1
        xs, xe = int(x.min()), int(x.max())
        out[j] = (xs, ys, xe - xs + 1, ye - ys + 1)
    return out[0] if single else out


def annToRLE(ann, size) -> dict:
    """The reference's ``annToRLE(ann, size)``: polygons or uncompressed RLE -> compressed RLE dict (rasterised and encoded on
    the device); an already compressed RLE is returned as it is."""
    segm = _segm(ann)
    h, w = int(size[0]), int(size[1])
    if isinstance(segm, dict) and isinstance(segm.get("counts"), (str, bytes, bytearray)):
        return segm
    if isinstance(segm, dict):
        _, counts = _split(segm, (h, w), "annToRLE")
        ops.pack_rle_masks([[counts]], [(h, w)])                       # validates: integers, non-negative, sum h*w
        return _rle_dicts([np.asarray(counts, dtype=np.int64)], [(h, w)])[0]
    return encode(masks_from_annotations([[ann]], [size], torch.device("cuda"))[0])[0]


def merge(rleObjs, intersect: bool = False) -> dict:
    """The reference's ``merge``: the union (``intersect``: the intersection) of a list of RLE dicts of one size -> one compressed
    RLE dict.  The run lists become bitmaps, are combined word by word and encoded again, all on the device.  One input comes back
    re-encoded.  The result is the canonical run list of the combined mask -- the first count a run of zeros that may be 0, no
    interior zero-length run -- which is what ``maskApi.c``'s ``rleMerge`` gives for canonical inputs; for inputs that carry
    interior zero-length runs ``rleMerge`` can keep such a run, and this function still returns the canonical form of the same
    mask.  An empty list gives ``{"size": [0, 0], "counts": b""}``.  Inputs of different sizes raise ValueError (pycocotools
    silently returns an empty RLE there)."""
    rles = list(rleObjs) if isinstance(rleObjs, (list, tuple)) else [rleObjs]
    if not rles:
        return {"size": [0, 0], "counts": b""}
    sizes = {tuple(int(v) for v in r["size"]) for r in rles}
    if len(sizes) > 1:
        raise ValueError(f"merge: the RLEs must share a size, got {sorted(sizes)}")
    size = sizes.pop()
    counts = ops.rle_merge([[_counts(r, f"merge: object {j}") for j, r in enumerate(rles)]], [size], bool(intersect))
    return _rle_dicts(counts, [size])[0]


def _is_number(v) -> bool:
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def _box_polygon(bb) -> list:
    """``rleFrBbox``: the box [x, y, w, h] as the polygon [x, y, x, y+h, x+w, y+h, x+w, y], in float64."""
    x, y, bw, bh = (float(v) for v in bb)
    xe, ye = x + bw, y + bh
    return [x, y, x, ye, xe, ye, xe, y]


def frPyObjects(pyobj, h, w):
    """The reference's ``frPyObjects(pyobj, h, w)``, by pycocotools' dispatch rules: an ``ndarray [n,4]`` or a list of 4-lists are
    boxes ``[x, y, w, h]``, a list of longer lists are polygons ``[x0, y0, x1, y1, ...]``, a list of dicts with ``counts`` and
    ``size`` are uncompressed RLEs -> a list with one compressed RLE dict each (polygons are NOT merged); a single 4-list, longer
    list or dict -> one RLE dict.  A box is rasterised as its four-corner polygon (``rleFrBbox``).  Boxes and polygons go through
    the polygon rasteriser and the encoder on the device; an RLE's ``size`` must be ``[h, w]``."""
    h, w = int(h), int(w)

    def polys(parts_per_object):
        if not parts_per_object:
            return []
        return encode(masks_from_annotations([[[p] for p in parts_per_object]], [(h, w)], torch.device("cuda"))[0])

    def boxes(rows):
        rows = np.asarray(rows, dtype=np.float64)
        if rows.ndim != 2 or rows.shape[1] != 4:
            raise ValueError(f"frPyObjects: boxes must be [n,4], got shape {rows.shape}")
        return polys([_box_polygon(r) for r in rows])

    def unc(dicts):
        counts = [_split(d, (h, w), f"frPyObjects: object {j}")[1] for j, d in enumerate(dicts)]
        ops.pack_rle_masks([counts], [(h, w)])                         # validates: integers, non-negative, sum h*w
        return _rle_dicts([np.asarray(c, dtype=np.int64) for c in counts], [(h, w)] * len(counts))

    def is_rle(v):
        return isinstance(v, dict) and "counts" in v and "size" in v

    if isinstance(pyobj, np.ndarray):
        return boxes(pyobj)
    if isinstance(pyobj, (list, tuple)) and len(pyobj) and is_rle(pyobj[0]):
        return unc(pyobj)
    if isinstance(pyobj, (list, tuple)) and len(pyobj) and isinstance(pyobj[0], (list, tuple, np.ndarray)):
        if len(pyobj[0]) == 4:
            return boxes(pyobj)
        if len(pyobj[0]) > 4:
            return polys([list(p) for p in pyobj])
    elif isinstance(pyobj, (list, tuple)) and len(pyobj) == 4 and all(_is_number(v) for v in pyobj):
        return boxes([pyobj])[0]
    elif isinstance(pyobj, (list, tuple)) and len(pyobj) > 4 and all(_is_number(v) for v in pyobj):
        return polys([list(pyobj)])[0]
    elif is_rle(pyobj):
        return unc([pyobj])[0]
    raise ValueError("frPyObjects: input type is not supported")


def rle_inter_tables(dt_counts: Sequence, gt_counts: Sequence, size):
    """Detections and ground truths of one ``size`` as counts arrays -> (inter int64 [D,G], det_area int64 [D], gt_area int64 [G]):
    bitmaps from the run lists and pair-wise popcounts, the detections in chunks of ``ops_masks.RLE_BITS_BUDGET_BYTES`` (every chunk
    carries the ground truths), one host copy per chunk."""
    nd, ng = len(dt_counts), len(gt_counts)
    per = 4 * ops.rle_bits_cells([size])[0]
    inter, d_area, g_area = np.zeros((nd, ng), np.int64), np.zeros(nd, np.int64), np.zeros(ng, np.int64)
    budget = max(ops_masks.RLE_BITS_BUDGET_BYTES - per * ng, per)
    for lo, hi in ops.budget_chunks([per] * nd, budget) or [(0, 0)]:
        k = hi - lo
        ws, lay = ops.rle_bits(list(dt_counts[lo:hi]) + list(gt_counts), [size] * (k + ng))
        pairs = np.stack(np.meshgrid(np.arange(k), k + np.arange(ng), indexing="ij"), -1).reshape(-1, 2)
        table = ops.bits_inter(ws, lay, pairs).cpu().numpy()          # the chunk's one device-to-host copy
        inter[lo:hi] = table[:k * ng].reshape(k, ng)
        d_area[lo:hi] = table[k * ng:k * ng + k]
        g_area[:] = table[k * ng + k:]
    return inter, d_area, g_area


def iou(dt, gt, iscrowd) -> np.ndarray:
    """The reference's ``iou(dt, gt, iscrowd)`` -> float64 ``[len(dt), len(gt)]``.  Boxes (``[n,4]`` xywh arrays or lists of
    4-lists) go through ``evaluator_det``'s restatement of ``bbIou``; lists of RLE dicts become bitmaps on the device, straight
    from their run lists, and the intersections and areas are popcounts of words (``rle_inter_tables``): no dense mask is
    written.  A crowd ground truth divides by the detection's area."""
    from . import evaluator_det as E
    crowd = np.asarray(iscrowd, dtype=np.int64).reshape(-1) != 0

    def is_rle(v):
        return isinstance(v, list) and len(v) > 0 and isinstance(v[0], dict)

    if is_rle(dt) != is_rle(gt) and len(dt) and len(gt):
        raise ValueError("iou: dt and gt must both be boxes or both be RLEs")
    if len(crowd) != len(gt):
        raise ValueError("iou: one iscrowd flag per ground truth is needed")
    if len(dt) == 0 or len(gt) == 0:
        return np.zeros((len(dt), len(gt)), dtype=np.float64)
    if not is_rle(dt):
        d, g = (np.asarray(v, dtype=np.float64).reshape(-1, 4) for v in (dt, gt))
        return E._box_iou_xywh(*(d[:, i] for i in range(4)), *(g[:, i] for i in range(4)), crowd)
    sizes = {tuple(int(v) for v in r["size"]) for r in dt + gt}
    if len(sizes) > 1:
        raise ValueError("iou: dt and gt RLEs differ in size")
    inter, d_area, g_area = rle_inter_tables([_counts(r, f"iou: dt {j}") for j, r in enumerate(dt)],
                                             [_counts(r, f"iou: gt {j}") for j, r in enumerate(gt)], sizes.pop())
    return E._mask_iou(inter, d_area.astype(np.float64), g_area.astype(np.float64), crowd)


def results_inter_tables(anns_per_image: Sequence[Sequence[dict]], dets_per_image: Sequence[Sequence[dict]], sizes) -> list:
    """The mask tables of a batch of images for ``evaluator_det.update_results``: per image (inter int64 [D,G], det_area int64
    [D], gt_pixels int64 [G]) from the results' ``segmentation`` RLEs against the annotations' ``segmentation`` (polygons,
    uncompressed or compressed RLE).  All RLEs of the batch become bitmaps in one launch; the polygon ground truths are rasterised
    in one ``masks_from_annotations`` call and bit-packed behind them; one pair launch and one host copy serve the batch."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    counts, obj_size, dense_at, det_idx, gt_idx = [], [], [], [], []
    polys, poly_sizes = [], []
    for i, (anns, dets, size) in enumerate(zip(anns_per_image, dets_per_image, sizes)):
        det_idx.append(list(range(len(counts), len(counts) + len(dets))))
        for j, r in enumerate(dets):
            c = _split(r["segmentation"], size, f"results: image {i} detection {j}")[1]
            if c is None:
                raise ValueError(f"results: image {i} detection {j}: a result's segmentation must be an RLE")
            counts.append(np.asarray(c, dtype=np.int64).reshape(-1))
            obj_size.append(size)
        idx, mine = [], []
        for j, a in enumerate(anns):
            parts, c = _split(_segm(a), size, f"annotations: image {i} object {j}")
            if c is None:
                idx.append(("dense", len(dense_at) + len(mine)))
                mine.append(parts)
            else:
                idx.append(("runs", len(counts)))
                counts.append(np.asarray(c, dtype=np.int64).reshape(-1))
                obj_size.append(size)
        gt_idx.append(idx)
        if mine:
            dense_at += [size] * len(mine)
            polys.append(mine)
            poly_sizes.append(size)
    dense = None
    if polys:
        stacks = masks_from_annotations(polys, poly_sizes, torch.device("cuda"))
        base = stacks[0].untyped_storage()
        if all(s.untyped_storage().data_ptr() == base.data_ptr() for s in stacks):      # views of the rasteriser's one flat buffer
            flat = torch.empty(0, dtype=torch.uint8, device=stacks[0].device).set_(base)
            starts = [s.storage_offset() for s in stacks]
        else:
            flat = torch.cat([s.reshape(-1) for s in stacks])
            starts = np.cumsum([0] + [s.numel() for s in stacks[:-1]]).tolist()
        offs = [st + k * h * w for st, s, (h, w) in zip(starts, stacks, poly_sizes) for k in range(s.shape[0])]
        dense = (flat, offs, dense_at)
    n_runs = len(counts)
    ws, lay = ops.rle_bits(counts, obj_size, dense=dense)
    pairs, spans = [], []
    for d_i, g_i in zip(det_idx, gt_idx):
        g_obj = [k if kind == "runs" else n_runs + k for kind, k in g_i]
        spans.append((len(pairs), d_i, g_obj))
        pairs += [(d, g) for d in d_i for g in g_obj]
    table = ops.bits_inter(ws, lay, pairs).cpu().numpy()              # the batch's one device-to-host copy
    area = table[len(pairs):]
    out = []
    for at, d_i, g_obj in spans:
        nd, ng = len(d_i), len(g_obj)
        out.append((table[at:at + nd * ng].reshape(nd, ng), area[np.asarray(d_i, np.int64)], area[np.asarray(g_obj, np.int64)]))
    return out
