"""Host restatement of maskApi.c's rleEncode / rleArea / rleToBbox in plain Python loops over integers.  It shares no code with
the product (``seam_match_rcnn_amd.mask_utils`` / ``ops.rle_encode`` / ``csrc/seam_rle.hip``) and defines what the device's run
lengths must be, bit for bit.  One deliberate difference to pycocotools, this project's rule everywhere: a pixel is set iff its
byte is non-zero (rleEncode compares each byte with its predecessor, which agrees for bytes 0/1 only).  Unpinned against
pycocotools itself (not installed where this project is tested); tests/test_rle_refs_host.py cross-checks it against
``mask_refs.rle_decode``, ``np.nonzero`` and ``mask.sum()``."""


def rle_encode(mask):
    """uint8 [h,w] -> counts: the column-major walk, runs of 0 and 1 alternating, the first a run of zeros."""
    h, w = mask.shape
    counts, prev, run = [], 0, 0
    for x in range(w):
        for y in range(h):
            v = 1 if mask[y, x] != 0 else 0
            if v != prev:
                counts.append(run)
                run, prev = 0, v
            run += 1
    counts.append(run)
    return counts


def rle_area(counts):
    """Set pixels: the odd-indexed counts."""
    a = 0
    for j in range(1, len(counts), 2):
        a += counts[j]
    return a


def rle_to_bbox(counts, h, w):
    """[x, y, w, h] of the set pixels by the run walk; [0,0,0,0] for no run of ones.  A run of ones that ends in a later column
    than it starts in makes the box full height."""
    m = (len(counts) // 2) * 2
    if m == 0:
        return [0.0, 0.0, 0.0, 0.0]
    xs, ys, xe, ye, cc, xp = w, h, 0, 0, 0, 0
    for j in range(m):
        cc += counts[j]
        t = cc - j % 2
        y = t % h
        x = (t - y) // h
        if j % 2 == 0:
            xp = x
        elif xp < x:
            ys, ye = 0, h - 1
        xs, xe, ys, ye = min(xs, x), max(xe, x), min(ys, y), max(ye, y)
    return [float(xs), float(ys), float(xe - xs + 1), float(ye - ys + 1)]


def tight_box(mask):
    """The same box from the pixels themselves; agrees with rle_to_bbox unless a run of ones spans two columns (full height
    then: the caller decides which applies)."""
    import numpy as np
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return [0.0, 0.0, 0.0, 0.0]
    return [float(xs.min()), float(ys.min()), float(xs.max() - xs.min() + 1), float(ys.max() - ys.min() + 1)]


def spans_columns(mask):
    """True when some run of ones goes on from the bottom of a column into the top of the next."""
    h, w = mask.shape
    return any(mask[h - 1, x] != 0 and mask[0, x + 1] != 0 for x in range(w - 1))
