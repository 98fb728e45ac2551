"""Plain numpy references of the detection post-process kernels (``csrc/seam_detect.hip``, ``csrc/seam_paste.h``) and the
input generators their tests share.  No torch op takes part in the arithmetic: everything is float64 or exact integers.
``test_detect_refs_host.py`` ties each reference to ``oracle/detection.py`` on the CPU; ``test_gpu_stress_detect.py`` holds the
kernels to them.

Lattice boxes.  Coordinates are multiples of 1/4 in [0, 64], sides multiples of 1/4 in [1/4, 16] (some forced to 0).  In
quarter units every coordinate is an integer <= 256, every side an integer <= 64, every area, intersection and union an integer
<= 8192 (in 1/16 units): all of them are exact in fp32 in ANY evaluation order, fused or not, so the only rounding of an IoU is
the one correctly rounded division (hipcc's default fp32 division is correctly rounded; the kernels are built without any
fast-math flag).  ``np.float32(I) / np.float32(U)`` from the integers is therefore bit for bit what a correct kernel computes,
and ``iou > np.float32(thr)`` its decision.  The lattice survives ``batched_nms``' class offset ``idx * (max + 1)`` for
idx <= 12: coordinates stay below 2^12 quarter units and sides do not change.  ``lattice_boxes`` plants pairs whose IoU is
EXACTLY 1/2, 1/4, 3/10 and 7/10 (3/10 and 7/10 round to the same fp32 as the thresholds 0.3 and 0.7 do), so ``>`` against
``>=`` decides survivors; ``nms_mask_ref`` refuses an input without at least ``MIN_TIES`` pairs exactly at a threshold of 0.5 or
0.25 unless the caller says that the case is not about ties (N = 1, 2 or a hand-built composition cannot hold 5 such pairs).

Bounds (u = 2^-24, the unit roundoff of fp32; every bound is a count of roundings times u times the sum of the absolute terms):

decode    x1 = bx + 0.5 w + dx w - 0.5 pw, pw = exp(dw) w.  Roundings on the longest chain: w, cx, dx, dx*w, + cx, dw, exp(dw)*w,
          the final subtraction: DECODE_ROUNDINGS = 8 on S = |bx| + 0.5 |w| + |dx w| + 0.5 |pw| (no single term passes more
          than 5 of them, which leaves room for the products of roundings).  The rounding of dw (u |dw|
          absolute) moves exp(dw) by u |dw| relative, and expf itself is off by EXPF_ULP = 1 ulp = 2 u relative (HIP's math-API
          documentation lists expf at 1 ulp; the toolchain ships no table, ``heads_refs.py`` takes the same figure): the bound adds
          (|dw| + 2 EXPF_ULP) u 0.5 |pw|.  Clipping is 1-Lipschitz and its limits are fp32 numbers: it adds nothing.  The clamp
          constant is the kernel's fp32 ``log(1000/16)`` (torch.clamp of an fp32 tensor uses the same fp32 number).
sigmoid   1 / (1 + e), e = expf(-x): e 2 u relative (weight e / (1 + e) <= 1), the sum u, the division u:
          SIGMOID_ROUNDINGS = 4, plus FLT_MIN absolute for results in the subnormal range (flushed or not).
paste     top = (1 - lx) a + lx b, bot likewise, v = (1 - ly) top + ly bot.  Longest chain: 1 - lx, the product lx*b, the fused
          add; then 1 - ly, ly*bot, the fused add: PASTE_ROUNDINGS = 6 on S = the same expression over |map|.  The integer box and
          the sample positions are formed in fp32 exactly as ``paste_box`` / ``paste_value`` form them (contraction off, the fused
          steps evaluated as exact rationals and rounded once); only the three interpolations are float64.
box_iou   float boxes: each area three roundings (two sides, the product), the intersection three; the union adds two sums.  The
          union is >= both areas and >= the intersection for non-inverted boxes, so its absolute error is below
          (3 + 3 + 3 + 2) u union; with the numerator's 3 u and the division's u: IOU_ROUNDINGS = 15 relative roundings
          (+ 1 for their products).
"""
from fractions import Fraction

import numpy as np

U = 2.0 ** -24
FLT_MIN = 2.0 ** -126
XFORM_CLIP = float(np.float32(4.135166556742356))        # the kernels' fp32 log(1000/16)
EXPF_ULP = 1.0
DECODE_ROUNDINGS = 8
SIGMOID_ROUNDINGS = 4
PASTE_ROUNDINGS = 6
IOU_ROUNDINGS = 15
MIN_TIES = 5
TIE_THRESHOLDS = (0.5, 0.25)


# ------------------------------------------------------------------------------------------------ lattice boxes
def quarter_units(boxes):
    """fp32 boxes [N,4] on the lattice -> int64 quarter units (asserts that they are on it)."""
    b = np.asarray(boxes, dtype=np.float64)
    q = np.rint(b * 4.0)
    assert np.array_equal(q, b * 4.0), "boxes are not multiples of 1/4"
    assert float(np.abs(q).max(initial=0.0)) < 2 ** 12, "lattice coordinates must stay below 2^12 quarter units"
    return q.astype(np.int64)


def on_lattice(boxes):
    b = np.asarray(boxes, dtype=np.float64) * 4.0
    return bool(np.array_equal(np.rint(b), b)) and float(np.abs(b).max(initial=0.0)) < 2 ** 12


def lattice_boxes(rng, n, zero_frac=0.04, plant=True):
    """n lattice boxes [n,4] fp32 in a random order.  ``plant``: a third of them (more in a small set) come in pairs built to
    have an IoU of exactly 1/2, 1/4, 3/10 or 7/10 (the second box lies inside the first and shares its corner), the members of
    a pair at unrelated positions of the list; the rest is random with coarse sides, which makes further exact ties."""
    q = np.zeros((n, 4), np.int64)
    side = rng.randint(1, 65, (n, 2))
    coarse = rng.rand(n) < 0.5
    side[coarse] = 4 * rng.randint(1, 17, (int(coarse.sum()), 2))
    zero = rng.rand(n, 2) < zero_frac / 2
    side[zero] = 0
    org = (rng.rand(n, 2) * (257 - side)).astype(np.int64)
    q[:, :2], q[:, 2:] = org, org + side
    if plant and n >= 2:
        # (num, den) of the planted IoU: the inner box covers num/den of the outer one
        kinds = [(1, 2), (1, 4), (1, 2), (1, 4), (3, 10), (7, 10)]
        pairs = max(n // 6, min(n // 2, 18))                 # 18 pairs hold 6 each at 1/2 and 1/4: small sets meet MIN_TIES
        slots = rng.permutation(n)[:2 * min(pairs, n // 2)].reshape(-1, 2)
        for j, (a, b) in enumerate(slots):
            num, den = kinds[j % 6]
            if j % 6 == 3:                                   # half the width and half the height
                w, h = 2 * rng.randint(1, 33), 2 * rng.randint(1, 33)
                iw, ih = w // 2, h // 2
            else:                                            # the same height, num/den of the width
                w, h = den * rng.randint(1, 64 // den + 1), rng.randint(1, 65)
                iw, ih = w // den * num, h
            x, y = rng.randint(0, 257 - w), rng.randint(0, 257 - h)
            q[a] = (x, y, x + w, y + h)
            q[b] = (x, y, x + iw, y + ih)
    return (q.astype(np.float64) / 4.0).astype(np.float32)


# A suppresses B (IoU 1/3), B overlaps C (1/3), A only touches C (0): B is gone before it can suppress C, so C survives at any
# threshold in [0, 1/3)
CHAIN = np.array([[0, 0, 8, 8], [4, 0, 12, 8], [8, 0, 16, 8]], np.float32)


def lattice_inter_union(a, b):
    """Integer intersection and union (1/16 units) of every pair of lattice boxes a [Na,4], b [Nb,4] -> (I, U) int64 [Na,Nb].
    The intersection's sides are clamped at 0 and the areas are not (torchvision's form): inverted boxes have negative areas."""
    qa, qb = quarter_units(a), quarter_units(b)
    iw = np.maximum(np.minimum(qa[:, None, 2], qb[None, :, 2]) - np.maximum(qa[:, None, 0], qb[None, :, 0]), 0)
    ih = np.maximum(np.minimum(qa[:, None, 3], qb[None, :, 3]) - np.maximum(qa[:, None, 1], qb[None, :, 1]), 0)
    inter = iw * ih
    area_a = (qa[:, 2] - qa[:, 0]) * (qa[:, 3] - qa[:, 1])
    area_b = (qb[:, 2] - qb[:, 0]) * (qb[:, 3] - qb[:, 1])
    union = area_a[:, None] + area_b[None, :] - inter
    assert int(np.abs(union).max(initial=0)) < 2 ** 24 and int(inter.max(initial=0)) < 2 ** 24
    return inter, union


def _f32_ratio(inter, union):
    with np.errstate(divide="ignore", invalid="ignore"):
        return inter.astype(np.float32) / union.astype(np.float32)


def exact_tie_count(boxes, thr):
    """Pairs i < j of lattice boxes whose IoU equals the threshold as a rational number."""
    return _tie_count(*lattice_inter_union(boxes, boxes), thr)


def _tie_count(inter, union, thr):
    fr = Fraction(thr).limit_denominator(64)
    tie = (inter * fr.denominator == union * fr.numerator) & (union > 0)
    return int(np.triu(tie, 1).sum())


def nms_mask_ref(boxes, thr, require_ties=True):
    """The full N x N bit table: out[i, j] = IoU(i, j) > thr in fp32, on lattice boxes.  A threshold of 0.5 or 0.25 must find at
    least MIN_TIES pairs exactly on it (``require_ties=False`` for inputs that are about something else)."""
    inter, union = lattice_inter_union(boxes, boxes)
    if require_ties and any(abs(thr - t) < 1e-12 for t in TIE_THRESHOLDS):
        ties = _tie_count(inter, union, thr)
        assert ties >= MIN_TIES, f"only {ties} pair(s) exactly at IoU {thr}: the comparison's strictness would go untested"
    return _f32_ratio(inter, union) > np.float32(thr)


def greedy_nms_ref(boxes, thr, max_keep=0, require_ties=False):
    """Sequential greedy scan over lattice boxes sorted by descending score -> keep bool [N].  A kept box suppresses every later
    box whose fp32 IoU with it is > fp32(thr) (NaN, from 0/0, compares false both ways).  max_keep > 0: stop after that many
    survivors, everything behind is not kept."""
    q = quarter_units(boxes)
    n = q.shape[0]
    if require_ties:
        nms_mask_ref(boxes, thr, True)
    area = (q[:, 2] - q[:, 0]) * (q[:, 3] - q[:, 1])
    t32 = np.float32(thr)
    supp = np.zeros(n, bool)
    keep = np.zeros(n, bool)
    kept = 0
    for i in range(n):
        if supp[i]:
            continue
        keep[i] = True
        kept += 1
        if max_keep > 0 and kept >= max_keep:
            break
        r = q[i + 1:]
        iw = np.maximum(np.minimum(q[i, 2], r[:, 2]) - np.maximum(q[i, 0], r[:, 0]), 0)
        ih = np.maximum(np.minimum(q[i, 3], r[:, 3]) - np.maximum(q[i, 1], r[:, 1]), 0)
        inter = iw * ih
        supp[i + 1:] |= _f32_ratio(inter, area[i] + area[i + 1:] - inter) > t32
    return keep


def batched_nms_ref(boxes, scores, idxs, valid, thr, top_n):
    """NMS run separately inside every class over the valid entries, the survivors of all classes merged by descending score
    (stable: equal scores keep the lower index first) and cut to ``top_n`` -> kept indices int64.  No coordinate offset."""
    boxes, scores, idxs, valid = np.asarray(boxes), np.asarray(scores), np.asarray(idxs), np.asarray(valid, bool)
    survivors = []
    for c in np.unique(idxs[valid]):
        members = np.nonzero(valid & (idxs == c))[0]
        members = members[np.argsort(-scores[members].astype(np.float64), kind="stable")]
        survivors.append(members[greedy_nms_ref(boxes[members], thr)])
    if not survivors:
        return np.zeros((0,), np.int64)
    s = np.sort(np.concatenate(survivors))
    s = s[np.argsort(-scores[s].astype(np.float64), kind="stable")]
    return s[:top_n].astype(np.int64)


# ------------------------------------------------------------------------------------------------ RPN top-k
def rpn_topk_ref(logits, k):
    """The kernel's documented order (``rpn_key``): NaN ranks as -inf, -0 equals +0, descending, ties lowest anchor index
    first; the first k indices.  Unlike torch.sort, which puts NaN first."""
    x = np.asarray(logits, dtype=np.float32).astype(np.float64).copy()
    x[np.isnan(x)] = -np.inf
    x[x == 0.0] = 0.0
    return np.argsort(-x, kind="stable")[:k].astype(np.int64)


# ------------------------------------------------------------------------------------------------ decode / sigmoid
def decode_ref(deltas, boxes, weights, clip_hw=None):
    """BoxCoder.decode (+ clip) in float64 from the fp32 inputs: deltas [N,ncls*4], boxes [N,4] -> (out [N,ncls*4] float64, bound
    [N,ncls*4] float64, the error allowed to an fp32 evaluation, module docstring).  A NaN dw / dh counts as the clamp value
    (``fminf`` returns its other operand)."""
    d = np.asarray(deltas, dtype=np.float32).astype(np.float64)
    b = np.asarray(boxes, dtype=np.float32).astype(np.float64)
    n = b.shape[0]
    d = d.reshape(n, -1, 4)
    wx, wy, ww, wh = [float(np.float32(v)) for v in weights]
    out = np.zeros_like(d)
    bound = np.zeros_like(d)
    with np.errstate(over="ignore", invalid="ignore"):
        for ax, (wc, ws) in enumerate(((wx, ww), (wy, wh))):
            lo, hi = b[:, ax][:, None], b[:, ax + 2][:, None]
            size = hi - lo
            ctr = lo + 0.5 * size
            dc = d[:, :, ax] / wc
            ds = d[:, :, ax + 2] / ws
            ds = np.where(np.isnan(ds), XFORM_CLIP, np.minimum(ds, XFORM_CLIP))
            pc = dc * size + ctr
            ps = np.exp(ds) * size
            out[:, :, ax] = pc - 0.5 * ps
            out[:, :, ax + 2] = pc + 0.5 * ps
            s = np.abs(lo) + 0.5 * np.abs(size) + np.abs(dc * size) + 0.5 * np.abs(ps)
            e = (np.abs(ds) + 2.0 * EXPF_ULP) * 0.5 * np.abs(ps)
            e = np.where(ps == 0.0, 0.0, e)                    # exp underflowed: |dw| may be inf, the term is 0
            bound[:, :, ax] = bound[:, :, ax + 2] = U * (DECODE_ROUNDINGS * s + e) + FLT_MIN
    if clip_hw is not None:
        ch, cw = float(np.float32(clip_hw[0])), float(np.float32(clip_hw[1]))
        out[:, :, 0::2] = np.clip(out[:, :, 0::2], 0.0, cw)
        out[:, :, 1::2] = np.clip(out[:, :, 1::2], 0.0, ch)
    return out.reshape(n, -1), bound.reshape(n, -1)


def sigmoid_ref(x):
    """float64 sigmoid of fp32 (or fp16) logits and the error allowed to ``1 / (1 + expf(-x))`` in fp32."""
    x = np.asarray(x).astype(np.float64)
    with np.errstate(over="ignore"):
        ref = 1.0 / (1.0 + np.exp(-x))
    return ref, SIGMOID_ROUNDINGS * U * ref + FLT_MIN


def mask_select_ref(logits, labels):
    """logits [K,14,14,4*ncls] in sub-pixel groups (group a*2+b holds pixel (2h+a, 2w+b)) -> the chosen channel's logits
    [K,1,28,28] float64 (no arithmetic: a gather)."""
    lg = np.asarray(logits)
    k = lg.shape[0]
    ncls = lg.shape[3] // 4
    g = lg.reshape(k, 14, 14, 2, 2, ncls)[np.arange(k), :, :, :, :, np.asarray(labels)]      # [K,14,14,2,2]
    return g.transpose(0, 1, 3, 2, 4).reshape(k, 1, 28, 28).astype(np.float64)


# ------------------------------------------------------------------------------------------------ paste
def _round_f32(q):
    """Fraction -> the nearest fp32 (ties to even), as a Python float.  Normal and subnormal range."""
    if q == 0:
        return 0.0
    sign = -1.0 if q < 0 else 1.0
    q = abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    e = max(e, -126)
    scaled = q / Fraction(2) ** (e - 23)
    m = scaled.numerator // scaled.denominator
    rem = scaled - m
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and (m & 1)):
        m += 1
    return sign * float(m) * 2.0 ** (e - 23)


def _fma32(a, b, c):
    """fp32 fused multiply-add of fp32 numbers given as Python floats: exact product and sum, one rounding."""
    return _round_f32(Fraction(a) * Fraction(b) + Fraction(c))


def paste_box_ref(box):
    """``paste_box`` step for step in fp32 -> (x0, y0, x1, y1, bw, bh, sx, sy); contraction off, the two fused steps fused."""
    f = np.float32
    bx = [f(v) for v in box]
    scale = f(30.0) / f(28.0)
    wh = f(f(f(bx[2] - bx[0]) * f(0.5)) * scale)
    hh = f(f(f(bx[3] - bx[1]) * f(0.5)) * scale)
    xs, ys = f(bx[2] + bx[0]), f(bx[3] + bx[1])
    x0, y0 = int(_fma32(float(xs), 0.5, -float(wh))), int(_fma32(float(ys), 0.5, -float(hh)))      # int() truncates toward 0
    x1, y1 = int(_fma32(float(xs), 0.5, float(wh))), int(_fma32(float(ys), 0.5, float(hh)))
    assert max(abs(x0), abs(y0), abs(x1), abs(y1)) < 2 ** 23, "the integer box must stay where (float)r + 0.5 is exact"
    bw, bh = max(x1 - x0 + 1, 1), max(y1 - y0 + 1, 1)
    return x0, y0, x1, y1, bw, bh, float(f(30.0) / f(bw)), float(f(30.0) / f(bh))


def _paste_axis(o0, o1, size, step, extent):
    """Canvas positions p in [0, extent) inside the integer box along one axis -> (p, lo index, hi index, hi weight fp32) on the
    30-cell padded map, as ``paste_value`` forms them."""
    lo_p, hi_p = max(o0, 0), min(o1, o0 + size - 1, extent - 1)
    p = np.arange(lo_p, hi_p + 1, dtype=np.int64)
    i0 = np.zeros(p.size, np.int64)
    lam = np.zeros(p.size, np.float64)
    for j, pos in enumerate(p):
        fpos = _fma32(step, float(pos - o0) + 0.5, -0.5)
        if fpos < 0.0:
            fpos = 0.0
        i = min(int(fpos), 29)
        i0[j] = i
        lam[j] = min(max(float(np.float32(fpos) - np.float32(i)), 0.0), 1.0)
    i1 = np.where(i0 < 29, i0 + 1, i0)
    return p, i0, i1, lam


def paste_ref(masks, boxes, hw):
    """masks [K,1,28,28] (or [K,28,28]), boxes [K,4] fp32, canvas (H, W) -> (value [K,1,H,W] float64, bound [K,1,H,W] float64).
    Zero (and a zero bound) outside the integer box."""
    m = np.asarray(masks, dtype=np.float32).astype(np.float64).reshape(-1, 28, 28)
    k = m.shape[0]
    h, w = int(hw[0]), int(hw[1])
    val = np.zeros((k, 1, h, w))
    bound = np.zeros((k, 1, h, w))
    growth = (1.0 + U) ** PASTE_ROUNDINGS - 1.0
    for i in range(k):
        x0, y0, x1, y1, bw, bh, sx, sy = paste_box_ref(np.asarray(boxes)[i])
        ys, iy0, iy1, ly = _paste_axis(y0, y1, bh, sy, h)
        xs, ix0, ix1, lx = _paste_axis(x0, x1, bw, sx, w)
        if ys.size == 0 or xs.size == 0:
            continue
        pad = np.zeros((30, 30))
        pad[1:29, 1:29] = m[i]
        for src, dst in ((pad, val), (np.abs(pad), bound)):
            top = (1.0 - lx)[None, :] * src[iy0][:, ix0] + lx[None, :] * src[iy0][:, ix1]
            bot = (1.0 - lx)[None, :] * src[iy1][:, ix0] + lx[None, :] * src[iy1][:, ix1]
            dst[i, 0, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1] = (1.0 - ly)[:, None] * top + ly[:, None] * bot
        inside = bound[i, 0, ys[0]:ys[-1] + 1, xs[0]:xs[-1] + 1]
        inside[...] = growth * inside + FLT_MIN
    return val, bound


def paste_inside(box, hw):
    """Boolean [H,W]: the canvas pixels inside the integer box (where a pasted value may be non-zero)."""
    x0, y0, x1, y1, bw, bh, _, _ = paste_box_ref(box)
    h, w = int(hw[0]), int(hw[1])
    yy, xx = np.arange(h)[:, None], np.arange(w)[None, :]
    return (yy >= y0) & (yy <= min(y1, y0 + bh - 1)) & (xx >= x0) & (xx <= min(x1, x0 + bw - 1))


# ------------------------------------------------------------------------------------------------ box IoU
def box_iou_ref(a, b):
    """IoU of every pair, torchvision's ``box_iou`` form (no clamping of the areas).  Lattice boxes: the bit-exact fp32 result
    ``float32(I) / float32(U)`` as float32, bound None.  Other boxes: float64 from the fp32 inputs and the relative-rounding
    bound of the module docstring."""
    if on_lattice(a) and on_lattice(b):
        return _f32_ratio(*lattice_inter_union(a, b)), None
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    iw = np.maximum(np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0]), 0.0)
    ih = np.maximum(np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1]), 0.0)
    inter = iw * ih
    aa = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    ab = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    with np.errstate(divide="ignore", invalid="ignore"):
        iou = inter / (aa[:, None] + ab[None, :] - inter)
    return iou, (IOU_ROUNDINGS + 1) * U * np.abs(iou) + FLT_MIN
