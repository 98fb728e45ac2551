"""Polygon and RLE ground-truth masks on the device: the packed tables, the rasterising launches, RLE encoding and the bitmap
algebra (merge, intersection, area) behind the COCO scoring."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _native
from ._ops_common import _mask_device, _ptr, _req, _stream

__all__ = ["MASK_MAX_SIDE", "MASK_MAX_POINTS", "MaskLayout", "mask_layout", "mask_views", "pack_poly_masks", "pack_rle_masks",
           "mask_flat", "launch_poly_masks", "launch_rle_masks", "resized_mask_layout", "launch_poly_masks_resized",
           "launch_rle_masks_resized", "poly_masks", "rle_masks", "rle_counts_from_positions", "rle_encode", "rle_encode_paste",
           "BitsLayout", "rle_bits_cells", "rle_bits", "bits_combine", "bits_to_rle", "bits_inter", "budget_chunks", "rle_merge"]


# ---------------------------------------------------------------------------------------------------- ground-truth masks (csrc/seam_masks.hip)
MASK_MAX_SIDE = 16384              # h, w of an image whose annotations are rasterised
MASK_MAX_POINTS = 2 ** 31          # boundary points of one poly_masks call (32-bit thread index), exclusive


@dataclass
class MaskLayout:
    """Where every object's [h,w] bytes lie in the flat uint8 buffer of a batch: image after image, an image's objects adjacent,
    so that image i's stack is the view ``flat[img_off[i]:img_off[i+1]].view(n_i, H_i, W_i)``."""
    counts: list                   # objects per image
    sizes: list                    # (h, w) per image
    obj_hw: object                 # int32 [n,2]
    obj_off: object                # int64 [n] byte offsets
    img_off: list                  # len(images) + 1 byte offsets

    @property
    def total(self) -> int:
        return self.img_off[-1]


def mask_layout(counts: Sequence[int], sizes: Sequence[Sequence[int]]) -> MaskLayout:
    import numpy as np
    if len(counts) != len(sizes):
        raise ValueError(f"masks: {len(counts)} images but {len(sizes)} sizes")
    hw, off, img_off, pos = [], [], [0], 0
    for i, (n, size) in enumerate(zip(counts, sizes)):
        h, w = (int(size[0]), int(size[1])) if len(size) == 2 else (0, 0)
        if len(size) != 2 or h != size[0] or w != size[1] or not (1 <= h <= MASK_MAX_SIDE and 1 <= w <= MASK_MAX_SIDE):
            raise ValueError(f"masks: image {i}: size {tuple(size)} must be (h, w) with 1 <= h, w <= {MASK_MAX_SIDE}")
        for _ in range(n):
            hw.append((h, w))
            off.append(pos)
            pos += h * w
        img_off.append(pos)
    return MaskLayout(list(counts), [(int(s[0]), int(s[1])) for s in sizes], np.asarray(hw, np.int32).reshape(-1, 2),
                      np.asarray(off, np.int64), img_off)


def mask_views(flat: torch.Tensor, lay: MaskLayout) -> list:
    return [flat[lay.img_off[i]:lay.img_off[i + 1]].view(n, h, w) for i, (n, (h, w)) in enumerate(zip(lay.counts, lay.sizes))]


def _selected(objs_per_image):
    """(image, object, flat object index, entry) of every entry that is not None."""
    out, k = [], 0
    for i, objs in enumerate(objs_per_image):
        for j, o in enumerate(objs):
            if o is not None:
                out.append((i, j, k, o))
            k += 1
    return out


def pack_poly_masks(polys: Sequence[Sequence], sizes: Sequence[Sequence[int]]):
    """Host packing of ``seam_poly_masks_u8``: ``polys[i][j]`` is object j of image i as a list of parts, each a flat
    ``[x0, y0, x1, y1, ...]`` sequence (an empty list: an object of zero parts, all zeros; None: not a polygon object, skipped).
    Returns (layout, tables): the int32 / int64 NumPy tables of include/seam_hip.h, the vertices upsampled in float64 as
    ``trunc(5*x + 0.5)``.  Raises ValueError, naming the object, for an odd-length or empty part, a coordinate that is not
    finite or with ``|5x + 0.5| >= 2^31``, and for ``MASK_MAX_POINTS`` boundary points or more."""
    import numpy as np
    lay = mask_layout([len(o) for o in polys], sizes)
    flat_xy, names, part_len, part_obj, part_words, sel_obj = [], [], [], [], [], []
    words_of = {}
    for i, j, k, parts in _selected(polys):
        h, w = lay.sizes[i]
        if (h, w) not in words_of:
            words_of[(h, w)] = int(_native.lib().seam_poly_masks_ws_bytes(h, w)) // 4
        for q, part in enumerate(parts):
            what = f"poly_masks: image {i} object {j} part {q}"
            try:
                xy = np.asarray(part, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"{what}: not a sequence of numbers") from e
            if xy.ndim != 1 or xy.size == 0 or xy.size % 2:
                raise ValueError(f"{what}: expected a flat, non-empty [x0, y0, x1, y1, ...] of even length, got shape {xy.shape}")
            flat_xy.append(xy)
            names.append(what)
            part_len.append(xy.size // 2)
            part_obj.append(len(sel_obj))
            part_words.append(words_of[(h, w)])
        sel_obj.append(k)
    P = len(part_len)
    part_len = np.asarray(part_len, np.int64)
    part_off = np.zeros(P + 1, np.int64)
    np.cumsum(part_len, out=part_off[1:])
    V = int(part_off[-1])
    up = 5.0 * (np.concatenate(flat_xy) if P else np.zeros(0))
    up = up + 0.5                                               # the multiply and the add stay apart, as (int)(5*x + 0.5) has them
    bad = ~(np.abs(up) < 2.0 ** 31)                             # also true for NaN
    if bad.any():
        at = int(np.flatnonzero(bad)[0])
        who = names[int(np.searchsorted(part_off, at // 2, side="right")) - 1]
        raise ValueError(f"{who}: a coordinate is not finite" if not np.isfinite(up[at]) else f"{who}: |5x + 0.5| must stay below 2^31")
    allp = np.trunc(up).astype(np.int64).reshape(-1, 2)
    nxt = np.arange(V, dtype=np.int64) + 1                      # ring successor of every vertex
    nxt[part_off[1:] - 1] = part_off[:-1]
    step = np.abs(allp[nxt] - allp)
    edge_pts = np.maximum(step[:, 0], step[:, 1]) + 1
    edge_pt_off = np.zeros(V + 1, np.int64)
    np.cumsum(edge_pts, out=edge_pt_off[1:])
    T = int(edge_pt_off[-1])
    if T >= MASK_MAX_POINTS:
        raise ValueError(f"poly_masks: {T} boundary points in one call, the limit is {MASK_MAX_POINTS} (split the batch)")
    part_ws_off = np.zeros(P + 1, np.int64)
    np.cumsum(part_words, out=part_ws_off[1:])
    sel = np.asarray(sel_obj, np.int64)
    tables = dict(pts=allp.astype(np.int32), part_off=part_off.astype(np.int32), part_obj=np.asarray(part_obj, np.int32),
                  edge_pt_off=edge_pt_off.astype(np.int32), part_ws_off=part_ws_off, obj_hw=np.ascontiguousarray(lay.obj_hw[sel]),
                  obj_out_off=np.ascontiguousarray(lay.obj_off[sel]), P=P, V=V, T=T, n=len(sel_obj), sel=sel)
    return lay, tables


def pack_rle_masks(rles: Sequence[Sequence], sizes: Sequence[Sequence[int]]):
    """Host packing of ``seam_rle_masks_u8``: ``rles[i][j]`` is object j of image i as its uncompressed counts (runs of 0 and 1
    alternating in column-major order, the first a run of zeros; None: not an RLE object, skipped).  Raises ValueError, naming
    the object, for counts that are negative, not integers, or do not sum to h*w."""
    import numpy as np
    lay = mask_layout([len(o) for o in rles], sizes)
    starts, run_off, sel_obj = [], [0], []
    for i, j, k, counts in _selected(rles):
        what = f"image {i} object {j}"
        h, w = lay.sizes[i]
        try:
            raw = np.asarray(counts)
            c = raw.astype(np.int64)
        except (TypeError, ValueError, OverflowError) as e:
            raise ValueError(f"rle_masks: {what}: counts are not a sequence of integers") from e
        if c.ndim != 1 or c.size == 0 or not (raw == c).all():
            raise ValueError(f"rle_masks: {what}: counts must be a flat, non-empty sequence of integers")
        if (c < 0).any() or int(c.sum()) != h * w:
            raise ValueError(f"rle_masks: {what}: counts must be non-negative and sum to h*w = {h * w}, got sum {int(c.sum())}")
        starts.append(np.cumsum(c) - c)
        run_off.append(run_off[-1] + c.size)
        sel_obj.append(k)
    if run_off[-1] >= 2 ** 31:
        raise ValueError("rle_masks: 2^31 runs or more in one call (split the batch)")
    sel = np.asarray(sel_obj, np.int64)
    tables = dict(run_start=(np.concatenate(starts) if starts else np.zeros(0, np.int64)).astype(np.int32),
                  obj_run_off=np.asarray(run_off, np.int32), obj_hw=np.ascontiguousarray(lay.obj_hw[sel]),
                  obj_out_off=np.ascontiguousarray(lay.obj_off[sel]), n=len(sel_obj), sel=sel)
    return lay, tables


def _upload_tables(tables: dict, names, device) -> dict:
    """One host-to-device copy for all tables of a call: the int64 ones first (8-byte alignment), everything as int32 words."""
    import numpy as np
    names = sorted(names, key=lambda k: -tables[k].dtype.itemsize)
    words = [np.ascontiguousarray(tables[k]).reshape(-1).view(np.int32) for k in names]
    dev = torch.from_numpy(np.concatenate(words)).to(device)
    out, pos = {}, 0
    for k, wd in zip(names, words):
        t = dev[pos:pos + wd.size]
        out[k] = t.view(torch.int64) if tables[k].dtype.itemsize == 8 else t
        pos += wd.size
    return out


def mask_flat(lay: MaskLayout, device, flat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The flat uint8 buffer of a batch's masks on ``device``: allocated (uninitialised), or ``flat`` checked against the layout."""
    device = _mask_device(device)
    if flat is None:
        return torch.empty((lay.total,), dtype=torch.uint8, device=device)
    flat = _req(flat, torch.uint8, "flat")
    if flat.dim() != 1 or flat.numel() != lay.total or flat.device != device:
        raise ValueError(f"masks: flat must be a uint8 [{lay.total}] tensor on {device}")
    return flat


def launch_poly_masks(lay: MaskLayout, t: dict, device, flat: Optional[torch.Tensor] = None) -> list:
    """``seam_poly_masks_u8`` over the tables of ``pack_poly_masks``: one upload, one launch sequence.  ``flat``: the batch's
    flat buffer when another producer fills the objects that were None in the packing; allocated here otherwise."""
    device = _mask_device(device)
    flat = mask_flat(lay, device, flat)
    if t["n"]:
        names = ("pts", "part_off", "part_obj", "edge_pt_off", "part_ws_off", "obj_hw", "obj_out_off")
        d = _upload_tables(t, names, device)
        ws_bytes = 4 * int(t["part_ws_off"][-1])
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        p = [_ptr(d[k]) if d[k].numel() else None for k in names]
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_poly_masks_u8(*p, _ptr(flat), _ptr(ws) if ws_bytes else None, ws_bytes, t["P"], t["V"],
                                                           t["T"], t["n"], _stream()), "seam_poly_masks_u8")
    return mask_views(flat, lay)


def launch_rle_masks(lay: MaskLayout, t: dict, device, flat: Optional[torch.Tensor] = None) -> list:
    """``seam_rle_masks_u8`` over the tables of ``pack_rle_masks`` (``flat`` as in ``launch_poly_masks``)."""
    device = _mask_device(device)
    flat = mask_flat(lay, device, flat)
    if t["n"]:
        names = ("run_start", "obj_run_off", "obj_hw", "obj_out_off")
        d = _upload_tables(t, names, device)
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_rle_masks_u8(*[_ptr(d[k]) for k in names], _ptr(flat), t["n"], _stream()),
                          "seam_rle_masks_u8")
    return mask_views(flat, lay)


def resized_mask_layout(lay: MaskLayout, out_sizes: Sequence[Sequence[int]], flips: Optional[Sequence] = None):
    """The output side of the resized expands (csrc/seam_input.hip) for a batch laid out as ``lay``: image i's objects are written
    at ``out_sizes[i]``, flipped where ``flips[i]``.  Returns (layout of the resized stacks, obj_out int32 [n,3] = (out_h, out_w,
    flip) per object of the batch)."""
    import numpy as np
    out_lay = mask_layout(lay.counts, out_sizes)
    flips = [False] * len(lay.counts) if flips is None else [bool(f) for f in flips]
    if len(flips) != len(lay.counts):
        raise ValueError(f"masks: {len(lay.counts)} images but {len(flips)} flips")
    flip = np.repeat(np.asarray(flips, np.int32), np.asarray(lay.counts, np.int64)).reshape(-1, 1)
    return out_lay, np.concatenate([out_lay.obj_hw, flip], axis=1).astype(np.int32)


def _resized_tables(t: dict, out_lay: MaskLayout, obj_out) -> dict:
    import numpy as np
    return dict(t, obj_out=np.ascontiguousarray(obj_out[t["sel"]]), obj_out_off=np.ascontiguousarray(out_lay.obj_off[t["sel"]]))


def launch_poly_masks_resized(lay: MaskLayout, t: dict, out_sizes, flips, device, flat: Optional[torch.Tensor] = None) -> list:
    """``launch_poly_masks`` with the expand of ``seam_poly_masks_resized_u8``: image i's stack comes out as uint8
    ``[n_i, *out_sizes[i]]`` = ``resize_masks_nearest(stack.flip(-1) if flips[i] else stack, out_sizes[i])`` bit for bit, and the
    original-size stack is never written.  ``flat``: the flat buffer of the RESIZED layout (``resized_mask_layout``)."""
    device = _mask_device(device)
    out_lay, obj_out = resized_mask_layout(lay, out_sizes, flips)
    flat = mask_flat(out_lay, device, flat)
    if t["n"]:
        t = _resized_tables(t, out_lay, obj_out)
        names = ("pts", "part_off", "part_obj", "edge_pt_off", "part_ws_off", "obj_hw", "obj_out", "obj_out_off")
        d = _upload_tables(t, names, device)
        ws_bytes = 4 * int(t["part_ws_off"][-1])
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        p = [_ptr(d[k]) if d[k].numel() else None for k in names]
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_poly_masks_resized_u8(*p, _ptr(flat), flat.numel(), _ptr(ws) if ws_bytes else None,
                                                                   ws_bytes, t["P"], t["V"], t["T"], t["n"], _stream()),
                          "seam_poly_masks_resized_u8")
    return mask_views(flat, out_lay)


def launch_rle_masks_resized(lay: MaskLayout, t: dict, out_sizes, flips, device, flat: Optional[torch.Tensor] = None) -> list:
    """``launch_rle_masks`` with the expand of ``seam_rle_masks_resized_u8`` (arguments as ``launch_poly_masks_resized``)."""
    device = _mask_device(device)
    out_lay, obj_out = resized_mask_layout(lay, out_sizes, flips)
    flat = mask_flat(out_lay, device, flat)
    if t["n"]:
        t = _resized_tables(t, out_lay, obj_out)
        names = ("run_start", "obj_run_off", "obj_hw", "obj_out", "obj_out_off")
        d = _upload_tables(t, names, device)
        with torch.cuda.device(device):
            _native.check(_native.lib().seam_rle_masks_resized_u8(*[_ptr(d[k]) for k in names], _ptr(flat), flat.numel(), t["n"],
                                                                  _stream()), "seam_rle_masks_resized_u8")
    return mask_views(flat, out_lay)


def poly_masks(polys: Sequence[Sequence], sizes: Sequence[Sequence[int]], device) -> list:
    """Polygon annotations of a batch of images -> list of uint8 0/1 [n_i,H_i,W_i] device stacks (views of one flat buffer), one
    table upload and one launch sequence for the batch; arguments and errors as ``pack_poly_masks``, no object may be None."""
    if any(o is None for img in polys for o in img):
        raise ValueError("poly_masks: every object needs a list of parts")
    return launch_poly_masks(*pack_poly_masks(polys, sizes), device)


def rle_masks(rles: Sequence[Sequence], sizes: Sequence[Sequence[int]], device) -> list:
    """Uncompressed RLE annotations of a batch of images -> list of uint8 0/1 [n_i,H_i,W_i] device stacks; arguments and errors
    as ``pack_rle_masks``, no object may be None."""
    if any(o is None for img in rles for o in img):
        raise ValueError("rle_masks: every object needs its counts")
    return launch_rle_masks(*pack_rle_masks(rles, sizes), device)


# ---------------------------------------------------------------------------------------------------- masks to RLE (csrc/seam_rle.hip)
def _rle_cells(h: int, w: int) -> int:
    b = int(_native.lib().seam_rle_encode_ws_bytes(int(h), int(w)))
    if b == 0:
        raise ValueError(f"rle_encode: size ({h}, {w}) must be (h, w) with 1 <= h, w <= {MASK_MAX_SIDE} and h*w < 2^31")
    return b // 4


def _rle_finish(counts: torch.Tensor, last_cell: torch.Tensor, hws, positions_launch) -> list:
    """The second half of both encoders: prefix sum, the per-object ends to the host (copy 1), the positions kernel into a
    buffer of exactly that size, the positions to the host (copy 2), then ``diff([0, *positions, h*w])`` per object."""
    import numpy as np
    scan = torch.cumsum(counts, 0)                                   # int64, inclusive
    ends = scan[last_cell].cpu().numpy()                             # device-to-host copy 1 of 2: the totals
    total = int(ends[-1])
    pos = torch.empty((total,), dtype=torch.int32, device=counts.device)
    positions_launch(scan, pos, total)
    pos = pos.cpu().numpy().astype(np.int64) if total else np.zeros(0, np.int64)      # copy 2 of 2: the positions
    return rle_counts_from_positions(pos, ends, hws)


def rle_counts_from_positions(pos, ends, hws) -> list:
    """Host: the batch's run boundaries (object o's are ``pos[ends[o-1]:ends[o]]``, ascending) -> per object
    ``diff([0, *positions, h*w])``, all objects in one pass."""
    import numpy as np
    n = len(hws)
    ends = np.asarray(ends, dtype=np.int64)
    lens = np.diff(ends, prepend=0)
    first = np.cumsum(lens + 2) - (lens + 2)                         # each object's slot for its leading 0
    edges = np.zeros(int(ends[-1]) + 2 * n, np.int64)
    edges[np.arange(pos.size, dtype=np.int64) + 2 * np.repeat(np.arange(n, dtype=np.int64), lens) + 1] = pos
    edges[first + lens + 1] = [h * w for h, w in hws]
    runs = np.diff(edges)
    keep = np.ones(runs.size, dtype=bool)
    keep[first[1:] - 1] = False                                      # the step from one object's h*w to the next one's 0
    return np.split(runs[keep], np.cumsum(lens + 1)[:-1])


def rle_encode(flat: torch.Tensor, lay: MaskLayout) -> list:
    """The objects of a flat uint8 mask buffer (``mask_flat`` / ``mask_views``; a pixel is set iff its byte != 0) -> one NumPy
    int64 ``counts`` array per object, maskApi's ``rleEncode``: column-major runs of 0 and 1 alternating, the first a run of
    zeros (``[h*w]`` for an empty mask, ``[0, h*w]`` for a full one).  Two device-to-host copies whatever the number of objects:
    the per-object totals, then the run boundaries."""
    import numpy as np
    flat = _req(flat, torch.uint8, "flat")
    if flat.dim() != 1 or flat.numel() != lay.total or not flat.is_cuda:
        raise ValueError(f"rle_encode: flat must be a uint8 [{lay.total}] tensor on the HIP device")
    n = int(len(lay.obj_off))
    if n == 0:
        return []
    hw_host = np.ascontiguousarray(lay.obj_hw, dtype=np.int32).reshape(n, 2)
    cells_of = {}
    for h, w in {(int(h), int(w)) for h, w in hw_host}:
        cells_of[(h, w)] = _rle_cells(h, w)
    cell_off = np.zeros(n + 1, np.int64)
    np.cumsum([cells_of[(int(h), int(w))] for h, w in hw_host], out=cell_off[1:])
    cells = int(cell_off[-1])
    tables = dict(obj_hw=hw_host, obj_off=np.ascontiguousarray(lay.obj_off, dtype=np.int64), cell_off=cell_off)
    d = _upload_tables(tables, ("obj_hw", "obj_off", "cell_off"), flat.device)
    ws = torch.empty((cells,), dtype=torch.int32, device=flat.device)
    counts = torch.empty((cells,), dtype=torch.int32, device=flat.device)
    lib = _native.lib()
    hw_ptr = hw_host.ctypes.data_as(C.c_void_p)
    with torch.cuda.device(flat.device):
        _native.check(lib.seam_rle_encode_masks_u8(_ptr(flat), flat.numel(), hw_ptr, _ptr(d["obj_hw"]), _ptr(d["obj_off"]),
                                                   _ptr(d["cell_off"]), _ptr(ws), 4 * cells, _ptr(counts), n, _stream()),
                      "seam_rle_encode_masks_u8")

        def positions(scan, pos, total):
            _native.check(lib.seam_rle_positions_masks(hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * cells,
                                                       _ptr(scan), _ptr(pos) if total else None, total, n, _stream()),
                          "seam_rle_positions_masks")

        return _rle_finish(counts, d["cell_off"][1:] - 1, [(int(h), int(w)) for h, w in hw_host], positions)


def rle_encode_paste(probs: torch.Tensor, boxes: torch.Tensor, hw) -> list:
    """The detections of one image, probs [D,1,28,28] or [D,28,28] and boxes [D,4] in pixels of the ``hw = (H, W)`` image ->
    one NumPy int64 ``counts`` array per detection: the RLE of ``paste_masks(probs, boxes, hw) > 0.5`` bit for bit (the set
    ``mask_inter`` counts), without the [D,1,H,W] paste -- only each clipped integer box is evaluated, each pixel once.  Two
    device-to-host copies, as ``rle_encode``."""
    probs, boxes = _req(probs, name="probs"), _req(boxes, name="boxes")
    d = probs.shape[0]
    if tuple(probs.shape[1:]) not in ((1, 28, 28), (28, 28)) or tuple(boxes.shape) != (d, 4):
        raise ValueError("rle_encode_paste: probs must be [D,1,28,28] or [D,28,28] and boxes [D,4]")
    if not probs.is_cuda or boxes.device != probs.device:
        raise ValueError("rle_encode_paste: probs and boxes must be on one HIP device")
    if boxes.data_ptr() & 15:                                       # the kernel reads a box as one float4
        boxes = boxes.clone()
    h, w = int(hw[0]), int(hw[1])
    per = _rle_cells(h, w)
    if d == 0:
        return []
    cells = per * d
    ws = torch.empty((cells,), dtype=torch.int32, device=probs.device)
    counts = torch.empty((cells,), dtype=torch.int32, device=probs.device)
    lib = _native.lib()
    with torch.cuda.device(probs.device):
        _native.check(lib.seam_rle_encode_paste_f32(_ptr(probs), _ptr(boxes), d, h, w, _ptr(ws), 4 * cells, _ptr(counts),
                                                    _stream()), "seam_rle_encode_paste_f32")

        def positions(scan, pos, total):
            _native.check(lib.seam_rle_positions_paste(d, h, w, _ptr(ws), 4 * cells, _ptr(scan), _ptr(pos) if total else None,
                                                       total, _stream()), "seam_rle_positions_paste")

        last = torch.arange(1, d + 1, device=probs.device, dtype=torch.int64) * per - 1
        return _rle_finish(counts, last, [(h, w)] * d, positions)


# ---------------------------------------------------------------------------------------------------- RLE algebra on bitmaps (csrc/seam_rle.hip)
RLE_BITS_BUDGET_BYTES = 64 << 20   # bitmap words (and dense bytes packed into them) of one chunk of a merge / iou / scoring job


@dataclass
class BitsLayout:
    """The objects of one bitmap workspace (int32 words, ``[ceil(h/32)][w]`` per object): object o's words start at
    ``cell_off[o]``; the objects lie one after the other in index order."""
    hw: object                     # NumPy int32 [n,2], the launchers' host table
    cell_off: object               # NumPy int64 [n+1], running sum of the objects' cells
    dev: dict                      # device tables: obj_hw int32 [n,2], cell_off int64 [n+1]

    @property
    def n(self) -> int:
        return int(self.hw.shape[0])

    @property
    def cells(self) -> int:
        return int(self.cell_off[-1])

    @property
    def hw_ptr(self):
        return self.hw.ctypes.data_as(C.c_void_p)


def rle_bits_cells(sizes: Sequence[Sequence[int]]) -> list:
    """Words of each object's bitmap, ``w * ceil(h/32)``; ValueError for a size the kernels refuse."""
    memo = {}
    return [memo[s] if s in memo else memo.setdefault(s, _rle_cells(*s)) for s in ((int(h), int(w)) for h, w in sizes)]


def _bits_layout(sizes, device, extra: Optional[dict] = None):
    """-> (layout, device copies of ``extra``'s tables): one upload for everything a chunk needs."""
    import numpy as np
    hw = np.ascontiguousarray(np.asarray([(int(h), int(w)) for h, w in sizes], np.int32).reshape(-1, 2))
    cell_off = np.zeros(len(hw) + 1, np.int64)
    np.cumsum(rle_bits_cells(hw.tolist()), out=cell_off[1:])
    tables = dict(extra or {}, obj_hw=hw, cell_off=cell_off)
    d = _upload_tables(tables, tuple(tables), device)
    return BitsLayout(hw, cell_off, dict(obj_hw=d["obj_hw"], cell_off=d["cell_off"])), d


def rle_bits(counts_per_object: Sequence, sizes: Sequence[Sequence[int]], device=None, dense=None):
    """Uncompressed RLE counts -> bitmaps, one bit per pixel, without a dense mask (``seam_rle_bits_from_runs``).
    ``counts_per_object[o]``: object o's counts, ``sizes[o] = (h, w)`` (any mix of sizes).  ``dense``: optional
    ``(flat uint8 tensor, byte offsets, sizes)`` of further objects that lie as row-major masks on the device (the rasteriser's
    output); they follow the run-list objects in the workspace, packed by the encoder's values stage.
    -> (ws int32 [cells] device tensor, BitsLayout).  One table upload; errors as ``pack_rle_masks``."""
    import numpy as np
    device = _mask_device(device if device is not None else (dense[0].device if dense is not None else "cuda"))
    n_runs_obj = len(counts_per_object)
    if len(sizes) != n_runs_obj:
        raise ValueError(f"rle_bits: {n_runs_obj} objects but {len(sizes)} sizes")
    _, t = pack_rle_masks([[c] for c in counts_per_object], sizes)   # validates: integers, non-negative, sum h*w
    d_sizes = [(int(h), int(w)) for h, w in dense[2]] if dense is not None else []
    extra = dict(run_start=t["run_start"], obj_run_off=t["obj_run_off"])
    all_sizes = [(int(h), int(w)) for h, w in sizes] + d_sizes
    cells = rle_bits_cells(all_sizes)
    first_dense = int(sum(cells[:n_runs_obj]))
    if d_sizes:
        extra["dense_off"] = np.asarray(dense[1], np.int64).reshape(-1)
        if extra["dense_off"].size != len(d_sizes):
            raise ValueError("rle_bits: one byte offset per dense object is needed")
        extra["dense_cell_off"] = np.cumsum([0] + cells[n_runs_obj:-1], dtype=np.int64)      # from the dense objects' first word
    lay, d = _bits_layout(all_sizes, device, extra)
    ws = torch.empty((lay.cells,), dtype=torch.int32, device=device)
    lib = _native.lib()
    with torch.cuda.device(device):
        if n_runs_obj:
            _native.check(lib.seam_rle_bits_from_runs(_ptr(d["run_start"]) if d["run_start"].numel() else None, _ptr(d["obj_run_off"]),
                                                      int(t["obj_run_off"][-1]), lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]),
                                                      _ptr(ws), 4 * lay.cells, n_runs_obj, _stream()), "seam_rle_bits_from_runs")
        if d_sizes:
            flat = _req(dense[0], torch.uint8, "dense")
            if flat.dim() != 1 or flat.device != device:
                raise ValueError(f"rle_bits: the dense buffer must be a flat uint8 tensor on {device}")
            tail = ws[first_dense:]
            scratch = torch.empty_like(tail)                          # the encoder's count stage comes with its values stage
            hw_tail = np.ascontiguousarray(lay.hw[n_runs_obj:])
            _native.check(lib.seam_rle_encode_masks_u8(_ptr(flat), flat.numel(), hw_tail.ctypes.data_as(C.c_void_p),
                                                       _ptr(d["obj_hw"][2 * n_runs_obj:]), _ptr(d["dense_off"]),
                                                       _ptr(d["dense_cell_off"]), _ptr(tail), 4 * tail.numel(), _ptr(scratch),
                                                       len(d_sizes), _stream()), "seam_rle_encode_masks_u8")
    return ws, lay


def bits_combine(ws: torch.Tensor, lay: BitsLayout, groups: Sequence[Sequence[int]], intersect: bool = False):
    """``groups[g]``: indices of objects of ``(ws, lay)``, all of one size -> (ws2, lay2) with object g the union (``intersect``:
    the intersection) of its group (``seam_rle_bits_combine``).  ValueError for an empty group, an index out of range or a group
    of mixed sizes."""
    import numpy as np
    sizes = []
    for g, grp in enumerate(groups):
        idx = [int(i) for i in grp]
        if not idx or min(idx) < 0 or max(idx) >= lay.n:
            raise ValueError(f"bits_combine: group {g} must name at least one object of 0..{lay.n - 1}")
        shapes = {(int(lay.hw[i, 0]), int(lay.hw[i, 1])) for i in idx}
        if len(shapes) > 1:
            raise ValueError(f"bits_combine: group {g} mixes the sizes {sorted(shapes)}")
        sizes.append(shapes.pop())
    group_off = np.zeros(len(groups) + 1, np.int32)
    np.cumsum([len(g) for g in groups], out=group_off[1:])
    group_obj = np.asarray([int(i) for g in groups for i in g], np.int32)
    lay2, d = _bits_layout(sizes, ws.device, dict(group_off=group_off, group_obj=group_obj))
    ws2 = torch.empty((lay2.cells,), dtype=torch.int32, device=ws.device)
    if groups:
        with torch.cuda.device(ws.device):
            _native.check(_native.lib().seam_rle_bits_combine(
                _ptr(d["group_off"]), _ptr(d["group_obj"]), int(group_obj.size), _ptr(lay.dev["obj_hw"]), _ptr(lay.dev["cell_off"]),
                _ptr(ws), 4 * ws.numel(), lay.n, lay2.hw_ptr, _ptr(lay2.dev["obj_hw"]), _ptr(lay2.dev["cell_off"]), _ptr(ws2),
                4 * lay2.cells, lay2.n, int(bool(intersect)), _stream()), "seam_rle_bits_combine")
    return ws2, lay2


def bits_to_rle(ws: torch.Tensor, lay: BitsLayout) -> list:
    """Bitmaps -> one NumPy int64 canonical ``counts`` array per object (``seam_rle_count_bits``, the prefix sum,
    ``seam_rle_positions_masks``): what ``rle_encode`` gives for the same masks.  Two device-to-host copies, as ``rle_encode``."""
    if lay.n == 0:
        return []
    counts = torch.empty((lay.cells,), dtype=torch.int32, device=ws.device)
    lib = _native.lib()
    d = lay.dev
    with torch.cuda.device(ws.device):
        _native.check(lib.seam_rle_count_bits(lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * lay.cells,
                                              _ptr(counts), lay.n, _stream()), "seam_rle_count_bits")

        def positions(scan, pos, total):
            _native.check(lib.seam_rle_positions_masks(lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * lay.cells,
                                                       _ptr(scan), _ptr(pos) if total else None, total, lay.n, _stream()),
                          "seam_rle_positions_masks")

        return _rle_finish(counts, d["cell_off"][1:] - 1, [(int(h), int(w)) for h, w in lay.hw], positions)


def bits_inter(ws: torch.Tensor, lay: BitsLayout, pairs, areas: bool = True) -> torch.Tensor:
    """``pairs`` int [P,2] (object indices of one size each) -> device int64 ``[P (+ n)]``: the pairs' ``popcount(a & b)``
    (``seam_rle_bits_inter``) followed, with ``areas``, by every object's own popcount (``seam_rle_bits_area``), so that one
    host copy brings both.  ValueError for an index out of range or a pair of two sizes."""
    import numpy as np
    pairs = np.ascontiguousarray(np.asarray(pairs, np.int64).reshape(-1, 2))
    if pairs.size and (pairs.min() < 0 or pairs.max() >= lay.n):
        raise ValueError(f"bits_inter: pairs must name objects of 0..{lay.n - 1}")
    if pairs.size and (lay.hw[pairs[:, 0]] != lay.hw[pairs[:, 1]]).any():
        raise ValueError("bits_inter: the two objects of a pair must share a size")
    P = int(pairs.shape[0])
    out = torch.empty((P + (lay.n if areas else 0),), dtype=torch.int64, device=ws.device)
    lib = _native.lib()
    d = lay.dev
    with torch.cuda.device(ws.device):
        if P:
            dp = torch.from_numpy(pairs.astype(np.int32)).to(ws.device)
            _native.check(lib.seam_rle_bits_inter(_ptr(dp), P, lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws),
                                                  4 * lay.cells, lay.n, _ptr(out), _stream()), "seam_rle_bits_inter")
        if areas and lay.n:
            _native.check(lib.seam_rle_bits_area(lay.hw_ptr, _ptr(d["obj_hw"]), _ptr(d["cell_off"]), _ptr(ws), 4 * lay.cells, lay.n,
                                                 _ptr(out[P:]), _stream()), "seam_rle_bits_area")
    return out


def budget_chunks(costs: Sequence[int], budget: int = None) -> list:
    """Consecutive index ranges ``(lo, hi)`` whose costs sum to at most ``budget`` (``RLE_BITS_BUDGET_BYTES``); an item that
    alone exceeds it gets a chunk of its own."""
    budget = RLE_BITS_BUDGET_BYTES if budget is None else int(budget)
    out, lo, acc = [], 0, 0
    for i, c in enumerate(costs):
        if i > lo and acc + c > budget:
            out.append((lo, i))
            lo, acc = i, 0
        acc += int(c)
    if len(costs) > lo:
        out.append((lo, len(costs)))
    return out


def rle_merge(groups: Sequence[Sequence], sizes: Sequence[Sequence[int]], intersect: bool = False) -> list:
    """``groups[g]``: the counts arrays of the RLEs to merge, all of ``sizes[g]`` -> one canonical counts array per group.  The
    groups are processed in chunks of ``RLE_BITS_BUDGET_BYTES`` of source and destination bitmaps."""
    cells = rle_bits_cells(sizes)
    out = []
    for lo, hi in budget_chunks([4 * c * (len(g) + 1) for c, g in zip(cells, groups)]):
        flat = [c for g in groups[lo:hi] for c in g]
        flat_sizes = [sizes[i] for i in range(lo, hi) for _ in groups[i]]
        ws, lay = rle_bits(flat, flat_sizes)
        idx, k = [], 0
        for g in groups[lo:hi]:
            idx.append(list(range(k, k + len(g))))
            k += len(g)
        out += bits_to_rle(*bits_combine(ws, lay, idx, intersect))
    return out
