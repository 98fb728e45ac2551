"""Host restatement of the RLE algebra of the COCO mask procedure (``maskApi.c``: rleMerge, rleFrBbox, rleIou's mask branch) and
of ``frPyObjects``' dispatch, in plain Python loops over integers.  It shares no code with the product
(``seam_match_rcnn_amd.mask_utils`` / ``ops.rle_bits`` / ``csrc/seam_rle.hip``) and defines what the device results must be, bit
for bit.  Unpinned against pycocotools itself (not installed where this project is tested);
tests/test_rle_algebra_refs_host.py cross-checks it against ``rle_encode`` of the combined decoded masks."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mask_refs import poly_mask, random_counts, random_polygon, rle_decode, rle_to_string      # noqa: E402,F401
from rle_refs import rle_encode                                                            # noqa: E402


def rle_merge_pair(A, B, intersect):
    """rleMerge's inner loop: two run lists of one size walked together, a count emitted where the combined value changes (and
    at the end)."""
    out = []
    ca, cb = A[0], B[0]
    v = va = vb = 0
    a = b = 1
    cc, ct = 0, 1
    while ct > 0:
        c = min(ca, cb)
        cc += c
        ct = 0
        ca -= c
        if ca == 0 and a < len(A):
            ca = A[a]
            a += 1
            va = 1 - va
        ct += ca
        cb -= c
        if cb == 0 and b < len(B):
            cb = B[b]
            b += 1
            vb = 1 - vb
        ct += cb
        vp = v
        v = int(va and vb) if intersect else int(va or vb)
        if v != vp or ct == 0:
            out.append(cc)
            cc = 0
    return out


def rle_merge(rles, intersect=False):
    """rleMerge: [(counts, h, w), ...] -> (counts, h, w), the pair-wise merge folded over the list.  No input: ([], 0, 0); one
    input: itself; a size mismatch: ([], 0, 0), as the C code leaves it."""
    if not rles:
        return [], 0, 0
    cnts, h, w = list(rles[0][0]), rles[0][1], rles[0][2]
    for counts, bh, bw in rles[1:]:
        if (bh, bw) != (h, w):
            return [], 0, 0
        cnts = rle_merge_pair(cnts, list(counts), intersect)
    return cnts, h, w


def bbox_polygon(bb):
    """rleFrBbox's polygon: xs, ys, xs, ye, xe, ye, xe, ys with xe = xs + w, ye = ys + h in float64."""
    xs, ys = float(bb[0]), float(bb[1])
    xe, ye = xs + float(bb[2]), ys + float(bb[3])
    return [xs, ys, xs, ye, xe, ye, xe, ys]


def rle_fr_bbox(bb, h, w):
    return rle_encode(poly_mask([bbox_polygon(bb)], h, w))


def rle_fr_poly(xy, h, w):
    return rle_encode(poly_mask([list(xy)], h, w))


def rle_fr_uncompressed(d):
    return [int(c) for c in d["counts"]]


def fr_py_objects(pyobj, h, w):
    """pycocotools' frPyObjects dispatch -> a list of counts lists, or one counts list for a single object."""
    if isinstance(pyobj, np.ndarray):
        return [rle_fr_bbox(bb, h, w) for bb in pyobj]
    if isinstance(pyobj, list) and isinstance(pyobj[0], dict) and "counts" in pyobj[0] and "size" in pyobj[0]:
        return [rle_fr_uncompressed(d) for d in pyobj]
    if isinstance(pyobj, list) and isinstance(pyobj[0], (list, tuple, np.ndarray)) and len(pyobj[0]) == 4:
        return [rle_fr_bbox(bb, h, w) for bb in pyobj]
    if isinstance(pyobj, list) and isinstance(pyobj[0], (list, tuple, np.ndarray)) and len(pyobj[0]) > 4:
        return [rle_fr_poly(xy, h, w) for xy in pyobj]
    if isinstance(pyobj, list) and len(pyobj) == 4:
        return rle_fr_bbox(pyobj, h, w)
    if isinstance(pyobj, list) and len(pyobj) > 4:
        return rle_fr_poly(pyobj, h, w)
    if isinstance(pyobj, dict) and "counts" in pyobj and "size" in pyobj:
        return rle_fr_uncompressed(pyobj)
    raise Exception("input type is not supported.")


def mask_iou(dt_counts, gt_counts, h, w, iscrowd):
    """Mask IoU with the crowd rule, pixel by pixel: inter / (|d| + |g| - inter), a crowd ground truth divides by |d|; 0 for a
    zero denominator (the project's rule, evaluator_det).  -> float64 [D,G]"""
    out = np.zeros((len(dt_counts), len(gt_counts)), np.float64)
    dms = [rle_decode([int(c) for c in d], h, w) for d in dt_counts]
    gms = [rle_decode([int(c) for c in g], h, w) for g in gt_counts]
    for i, dm in enumerate(dms):
        for j, gm in enumerate(gms):
            inter = da = ga = 0
            for y in range(h):
                for x in range(w):
                    p, q = int(dm[y, x] != 0), int(gm[y, x] != 0)
                    inter += p & q
                    da += p
                    ga += q
            den = da if iscrowd[j] else da + ga - inter
            out[i, j] = inter / den if den else 0.0
    return out
