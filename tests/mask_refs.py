"""Host restatement of the COCO mask procedure (``maskApi.c``: rleFrPoly, rleFrString, rleToString, rleMerge, rleDecode), written
from the published procedure in plain Python / NumPy with integers and float64, the multiply and the add kept apart.  It shares no
code with the product (``seam_match_rcnn_amd.mask_utils`` / ``ops.poly_masks`` / ``csrc/seam_masks.hip``) and defines what the
device masks must be, bit for bit.  Unpinned against pycocotools itself (not installed where this project is tested)."""
import math

import numpy as np

SCALE = 5.0


def c_int(x):
    """C's (int) of a double: truncation toward zero."""
    return int(math.trunc(x))


def upsample(xy):
    """Step 1: the closed ring of upsampled integer vertices."""
    k = len(xy) // 2
    X = [c_int(SCALE * float(xy[2 * j]) + 0.5) for j in range(k)]
    Y = [c_int(SCALE * float(xy[2 * j + 1]) + 0.5) for j in range(k)]
    return X + X[:1], Y + Y[:1]


def boundary_points(X, Y):
    """Step 2: every integer point of every edge of the closed ring, in order."""
    u, v = [], []
    for j in range(len(X) - 1):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ye - ys)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe = xe, xs
            ys, ye = ye, ys
        if dx >= dy:
            if dx == 0:                      # zero-length edge: 0/0 in C, its v is never read
                u.append(xs)
                v.append(ys)
                continue
            s = float(ye - ys) / float(dx)
            for d in range(dx + 1):
                t = dx - d if flip else d
                u.append(t + xs)
                prod = s * float(t)
                v.append(c_int(float(ys) + prod + 0.5))
        else:
            s = float(xe - xs) / float(dy)
            for d in range(dy + 1):
                t = dy - d if flip else d
                v.append(t + ys)
                prod = s * float(t)
                u.append(c_int(float(xs) + prod + 0.5))
    return u, v


def crossings(xy, h, w):
    """Steps 1-3 of one polygon part: the list of (x, y) crossings, y in [0, h]."""
    X, Y = upsample(xy)
    if len(X) < 2:
        return []
    u, v = boundary_points(X, Y)
    out = []
    for j in range(1, len(u)):
        if u[j] == u[j - 1]:
            continue
        xd = float(u[j] if u[j] < u[j - 1] else u[j] - 1)
        xd = (xd + 0.5) / SCALE - 0.5
        if math.floor(xd) != xd or xd < 0 or xd > w - 1:
            continue
        yd = float(v[j] if v[j] < v[j - 1] else v[j - 1])
        yd = (yd + 0.5) / SCALE - 0.5
        if yd < 0:
            yd = 0.0
        elif yd > h:
            yd = float(h)
        yd = math.ceil(yd)
        out.append((int(xd), int(yd)))
    return out


def part_mask(xy, h, w):
    """Step 4, the sorted linear form: uint8 [h,w]."""
    a = sorted(x * h + y for x, y in crossings(xy, h, w))
    a.append(h * w)
    flat = np.zeros(h * w, np.uint8)                 # column-major
    val, pos = 0, 0
    for p in a:
        if val:
            flat[pos:p] = 1
        pos, val = p, val ^ 1
    return np.ascontiguousarray(flat.reshape(w, h).T)


def part_mask_by_columns(xy, h, w):
    """mask[r,c] = parity(#crossings in column c with y <= r): what a per-column fill computes."""
    tog = np.zeros((h + 1, w), np.int64)
    for x, y in crossings(xy, h, w):
        tog[y, x] += 1
    return (np.cumsum(tog, axis=0)[:h] & 1).astype(np.uint8)


def column_counts(xy, h, w):
    n = np.zeros(w, np.int64)
    for x, _ in crossings(xy, h, w):
        n[x] += 1
    return n


def poly_mask(parts, h, w):
    """An object: the union of its parts' masks."""
    m = np.zeros((h, w), np.uint8)
    for xy in parts:
        m |= part_mask(xy, h, w)
    return m


def rle_decode(counts, h, w):
    """Runs of 0 and 1 alternating in column-major order, the first a run of zeros."""
    flat = np.zeros(h * w, np.uint8)
    pos, val = 0, 0
    for c in counts:
        if val:
            flat[pos:pos + c] = 1
        pos += c
        val ^= 1
    assert pos == h * w, (pos, h, w)
    return np.ascontiguousarray(flat.reshape(w, h).T)


def rle_from_string(s):
    if isinstance(s, bytes):
        s = s.decode("ascii")
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = ord(s[p]) - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_to_string(counts):
    out = []
    for i, x in enumerate(counts):
        x = int(x)
        if i > 2:
            x -= int(counts[i - 2])
        more = True
        while more:
            c = x & 0x1f
            x >>= 5                                   # arithmetic shift
            more = (x != -1) if (c & 0x10) else (x != 0)
            if more:
                c |= 0x20
            out.append(chr(c + 48))
    return "".join(out)


def ann_mask(segm, h, w):
    """What annToMask returns for one annotation's ``segmentation``."""
    if isinstance(segm, list):
        return poly_mask(segm, h, w)
    counts = segm["counts"]
    if not isinstance(counts, (list, tuple, np.ndarray)):
        counts = rle_from_string(counts)
    return rle_decode([int(c) for c in counts], h, w)


# ------------------------------------------------------------------------------------------------ seeded generators
def random_polygon(rng, h, w, integer_only=False, max_pts=9, small_steps=False):
    """1..max_pts vertices up to 3 px outside every edge; integer, half-integer or free coordinates."""
    k = int(rng.integers(1, max_pts + 1))
    mode = 0 if integer_only else int(rng.integers(0, 3))
    if small_steps:                                   # integer vertices at most 12 px apart: slopes like 5/6, whose s*t half cases
        x = float(rng.integers(-3, w + 4))           # round differently under a fused multiply-add
        y = float(rng.integers(-3, h + 4))
        xy = []
        for _ in range(k):
            xy += [x, y]
            x = float(min(max(x + int(rng.integers(-12, 13)), -3), w + 3))
            y = float(min(max(y + int(rng.integers(-12, 13)), -3), h + 3))
        return xy
    xy = []
    for _ in range(k):
        for lim in (w, h):
            if mode == 0:
                c = float(rng.integers(-3, lim + 4))
            elif mode == 1:
                c = float(rng.integers(-6, 2 * lim + 7)) / 2.0
            else:
                c = float(rng.uniform(-3.0, lim + 3.0))
            xy.append(c)
    return xy


def random_counts(rng, h, w, max_runs=12, zero_runs=True):
    """Counts of alternating runs that sum to h*w; zero-length runs (also the first) appear when ``zero_runs``."""
    n = h * w
    k = int(rng.integers(1, max_runs + 1))
    cuts = np.sort(rng.integers(0, n + 1, size=k - 1))
    if not zero_runs:
        cuts = np.unique(cuts[(cuts > 0) & (cuts < n)])
    edges = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    return [int(c) for c in np.diff(edges)]
