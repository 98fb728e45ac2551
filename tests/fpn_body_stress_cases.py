"""Seeded case generators of the FPN / body / stem adjoint stress (``test_gpu_stress_fpn_body_train.py``), host code only.

One generator per kernel of ``csrc/seam_fpn_train.hip`` and ``csrc/seam_body_train.hip``.  Each yields dicts of small operands
(torch tensors on the CPU) with a ``tags`` set; ``REQUIRED[kernel][category]`` is the number of cases that must carry the
category.  Every tag is computed from the operands a case really holds, never from the intent of its row in the tables below,
so ``test_fpn_body_stress_cases_host.py`` proves on the CPU that the sweep enters the paths it is meant to enter:

  roi_align_bwd    more than 256 ROIs in one (image, level) bucket (the second step of the ordered compaction and its running
                   base), C > 256 (blockIdx.y >= 1) and C = 260 (a last channel chunk with idle lanes), P = 32 (RB_PMAX), maps
                   of 1 x 1 and of 5 x 6 tiles and more, boxes whose first / last sample sits at a tile border and one fp32 step
                   to either side of it (the bounding-box rejection decides there), levels given and mapped, empty buckets,
                   image indices and boxes that are not numbers
  rpn_scatter      8 levels (SC_MAX_LEVELS), a ragged last 64-channel block (C = 72), hundreds of rows on one 3 x 3
                   neighbourhood (the per-row barrier chain), rows outside their map, 1 x 1 maps
  upsample_add_bwd ratios 1, 2, 3, 5 and fractions, a coarse map larger than the fine one (coarse pixels that receive
                   nothing), a coarse map of 1 x 1, with and without ``base``
  subsample_add_bwd   both parities of H and W down to 1
  conv3x3s2_dgrad  gridDim.y > 1 of every BN variant (C = 96, 192, 256 / 512), K > C and K < C, the real 512 / 512 layer, extents
                   of both parities down to 1, a parity class wider than one 128-pixel tile
  maxpool3s2_relu_bwd every value of nblocks % 8 (the XCD remap), 1 - 3 chunks per pooled row
  relu_mask_add    1 ... just over 1024 float4 lanes, C that is only a multiple of 4

The float64 reference of one case takes well under a second: ``roi_reference_cost`` is what ``fpn_train_refs.roi_align_bwd_scatter``
spends (its einsum visits H * W * P * P * C products per ROI), and the host test bounds it.
"""
import numpy as np
import torch

import fpn_train_refs as FR
from oracle import detection as OD

NAN, INF = float("nan"), float("inf")


def _step(v, j):
    """``j`` fp32 steps away from ``v``."""
    v = np.float32(v)
    for _ in range(abs(j)):
        v = np.nextafter(v, np.float32(np.inf if j > 0 else -np.inf))
    return float(v)


# ------------------------------------------------------------------------------------------------ RoIAlign adjoint
# N, P, sr, C, K, explicit levels, pyramid (None: drawn), flags
ROI_SPECS = [
    (2, 7, 2, 8, 40, False, [(33, 41), (17, 21), (9, 11), (5, 6)], {"border"}),
    (3, 7, 2, 8, 48, True, [(41, 35), (1, 1), (12, 9), (7, 30)], {"border", "bad"}),
    (1, 14, 2, 8, 30, False, [(35, 41), (20, 18), (8, 8), (3, 4)], {"border"}),
    (2, 5, 3, 64, 20, True, [(34, 41), (9, 9), (16, 24), (1, 7)], {"border"}),
    (2, 32, 2, 4, 10, True, [(20, 24), (10, 12), (5, 6), (3, 3)], set()),
    (1, 32, 4, 8, 8, False, [(17, 9), (24, 16), (6, 5), (2, 2)], {"bad"}),
    (2, 32, 1, 4, 12, True, [(9, 33), (1, 1), (4, 4), (16, 8)], {"border"}),
    (5, 1, 1, 4, 340, True,[(12, 15), (9, 9), (5, 5), (3, 2)], {"k256"}),
    (2, 2, 2, 8, 520, True, [(20, 24), (10, 12), (5, 6), (3, 3)], {"k256"}),
    (3, 1, 4, 4, 700, False, [(16, 16), (8, 8), (4, 4), (2, 2)], {"k256"}),
    (1, 5, 1, 8, 330, True, [(33, 41), (3, 3), (8, 9), (1, 1)], {"k256", "border"}),
    (4, 2, 3, 4, 400, True, [(7, 7), (25, 9), (2, 13), (6, 6)], {"k256", "bad"}),
    (2, 7, 2, 260, 20, True, [(16, 16), (8, 8), (4, 4), (2, 2)], set()),
    (1, 5, 2, 260, 30, False, [(16, 13), (9, 16), (5, 5), (1, 1)], {"border"}),
    (3, 2, 1, 512, 64, True, [(16, 16), (11, 7), (3, 16), (1, 1)], {"bad"}),
    (2, 7, 2, 512, 16, False, [(12, 16), (6, 8), (3, 4), (2, 2)], set()),
    (1, 14, 2, 256, 8, True, [(14, 14), (7, 7), (4, 4), (2, 2)], set()),
    (2, 1, 1, 64, 40, False, [(41, 41), (21, 21), (11, 11), (6, 6)], {"border"}),
    (4, 7, 4, 4, 36, True, [(3, 40), (38, 2), (1, 1), (13, 13)], {"border", "bad"}),
    (2, 2, 2, 64, 50, False, None, {"bad"}),
    (5, 5, 2, 8, 60, True, None, set()),
    (1, 14, 3, 4, 20, False, [(30, 40), (15, 20), (8, 10), (4, 5)], {"border"}),
    (3, 7, 1, 8, 45, True, [(8, 8), (16, 16), (24, 24), (32, 32)], {"border"}),
    (2, 5, 4, 4, 33, False, [(1, 1), (2, 3), (41, 41), (9, 9)], set()),
    (2, 7, 2, 8, 64, True, [(33, 41), (41, 33), (5, 5), (2, 2)], {"border", "image0"}),
    (1, 2, 2, 4, 1, True, [(5, 5), (4, 4), (3, 3), (2, 2)], set()),
    (2, 7, 2, 64, 0, False, "fixture", set()),
    (2, 14, 2, 8, 0, True, "fixture", set()),
    (3, 5, 3, 260, 24, True, None, {"bad"}),
    (4, 7, 2, 8, 70, True, None, {"border"}),
]
MAPPED_SIZE = [(8.0, 105.0), (120.0, 215.0), (235.0, 430.0), (470.0, 1000.0)]     # sqrt(area) of a box LevelMapper sends to level l


def _box_on_level(rng, l, hws, scales, mapped):
    """A random box that lands on level ``l``: any box of that level's grid when the level is given, a box whose size the
    LevelMapper sends there (well inside the level's range) when it is mapped."""
    h, w = hws[l]
    s = scales[l]
    if mapped:
        size = rng.uniform(*MAPPED_SIZE[l])
        ar = rng.uniform(0.75, 1.35)
        bw, bh = size * ar, size / ar
        cx, cy = rng.uniform(0, w) / s, rng.uniform(0, h) / s
    else:
        bw, bh = rng.uniform(0.5, max(1.5, 0.9 * w)) / s, rng.uniform(0.5, max(1.5, 0.9 * h)) / s
        cx, cy = rng.uniform(0, w) / s, rng.uniform(0, h) / s
    return [cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]


def _degenerate(rng, l, hws, scales):
    """The degenerate kinds of ``fpn_train_refs.roi_set`` on the grid of level ``l`` (image coordinates)."""
    h, w = hws[l]
    s = scales[l]
    cx, cy = rng.uniform(0, max(w - 1, 0.5)), rng.uniform(0, max(h - 1, 0.5))
    g = [
        [w + 50, h + 50, w + 60, h + 60],                       # far outside: every sample skipped
        [-3, 0.2 * h, 0.3 * w, 0.7 * h],                        # over the left edge
        [0.3 * w, -3.5, 0.8 * w, 0.4 * h],                      # over the top edge
        [0.7 * w, 0.1 * h, w + 4, 0.6 * h],                     # over the right edge
        [0.2 * w, 0.6 * h, 0.5 * w, h + 5],                     # over the bottom edge
        [-6, -6, 0.5, 0.7],                                     # a corner: samples in (-1, 0) are clamped, those below skipped
        [cx + 0.2, cy + 0.3, cx + 0.9, cy + 1.1],               # smaller than a pixel: the extent clamp
        [0, 0, w, h],                                           # the whole map
        [w - 0.5, h - 0.5, w, h],                               # the last pixel: row / column collapse
    ]
    return [[v / s for v in b] for b in g]


def _border_boxes(rng, l, hws, scales, p, sr, mapped):
    """Boxes whose scaled edge is a multiple of 8 of the level's grid, and one fp32 step to either side.  With the far edge
    at 8m and a bin narrower than 2 sr, the last sample lies in [8m - 1, 8m): pixel 8m -- the first of the next tile -- gets
    a term only as that sample's upper neighbour, which a bounding box one pixel too tight drops.  With the near edge at 8m the
    first sample sits just past the border and pixel 8m - 1 gets nothing."""
    h, w = hws[l]
    s = scales[l]
    out = []
    lim = 24.0 if mapped else 1e9                               # a mapped box must stay on level 0 (its size below 105)
    for size, axis in ((w, 0), (h, 1)):
        ms = list(range(1, (size - 1) // 8 + 1))
        if not ms:
            continue
        for j in (-1, 0, 1):
            m = ms[rng.randint(len(ms))]
            ext = rng.uniform(1.0, min(1.8 * sr * p, 8 * m + 1, lim))
            other = (h, w)[axis]
            o1 = rng.uniform(-1, max(other - 2, 0))
            o2 = o1 + rng.uniform(1.0, min(max(other, 2), lim))
            far = _step(8 * m / s, j)
            near = _step(8 * m / s, j)
            for a1, a2 in ((far - ext / s, far), (near, near + ext / s)):
                out.append([a1, o1 / s, a2, o2 / s] if axis == 0 else [o1 / s, a1, o2 / s, a2])
    return out


def _draw_pyramid(rng, c):
    top = 16 if c > 256 else 41
    return [(int(rng.randint(1, top + 1)), int(rng.randint(1, top + 1))) for _ in range(4)]


def _inside(roi, lvl, n, hws, scales):
    """The ROI belongs to a bucket and its box meets the level's map."""
    b = roi[0]
    if not (np.isfinite(roi).all() and 0 <= b < n and 0 <= lvl < 4):
        return False
    h, w = hws[lvl]
    s = scales[lvl]
    return roi[3] * s > 0 and roi[1] * s < w and roi[4] * s > 0 and roi[2] * s < h


def roi_align_bwd_cases():
    scales = list(FR.ROI_SCALES)
    for idx, (n, p, sr, c, k, explicit, hws, flags) in enumerate(ROI_SPECS):
        rng = np.random.RandomState(1000 + idx)
        tags = set()
        keep = None
        if hws == "fixture":                                     # the ROI set of test_gpu_fpn_train.py on its own pyramid
            hws = list(FR.ROI_HWS)
            rois = FR.roi_set("some").numpy().astype(np.float64)
            k = rois.shape[0]
            levels = FR.explicit_levels(k, torch.from_numpy(rois[:, 0] == 1)).numpy() if explicit else None
            keep = np.ones(k, bool)
        else:
            if hws is None:
                hws = _draw_pyramid(rng, c)
            mapped = not explicit
            boxes, lv, img = [], [], []

            def add(b, l, i=None):
                boxes.append(b)
                lv.append(l)
                img.append(int(rng.randint(n)) if i is None else i)

            if "k256" in flags:                                  # one bucket of about 270 ROIs, half of the rest in a second one
                heavy_l = 0 if mapped else int(np.argmax([h * w if h * w <= 100 else 0 for h, w in hws]))
                heavy_i = int(rng.randint(n))
                second = ((heavy_i + 1) % n, heavy_l) if n > 1 else (heavy_i, (heavy_l + 1) % 4)
                nh = int(rng.randint(268, 281))
                for _ in range(nh):
                    add(_box_on_level(rng, heavy_l, hws, scales, mapped), heavy_l, heavy_i)
                for _ in range((k - nh) // 2):
                    add(_box_on_level(rng, second[1], hws, scales, mapped), second[1], second[0])
            if "border" in flags:
                for l in ((0,) if mapped else range(4)):
                    for b in _border_boxes(rng, l, hws, scales, p, sr, mapped):
                        if len(boxes) < k - 4:
                            add(b, l)
                            tags.add("tile_border_edges")
            if len(boxes) < k - 12:
                l = 0 if mapped else int(rng.randint(4))
                for b in _degenerate(rng, l, hws, scales):
                    add(b, l)
            one_image = "image0" in flags
            while len(boxes) < k:
                l = int(rng.randint(4))
                add(_box_on_level(rng, l, hws, scales, mapped), l)
                if len(boxes) + 1 < k and rng.rand() < 0.08:      # an exact duplicate, sometimes in another image
                    add(list(boxes[-1]), l, img[-1] if rng.rand() < 0.5 else None)
            order = rng.permutation(k)
            rois = np.concatenate([np.asarray(img, np.float64)[:, None], np.asarray(boxes, np.float64)], 1)[order]
            if one_image:
                rois[:, 0] = 0
            levels = np.asarray(lv, np.int64)[order] if explicit else None
            keep = np.ones(k, bool)
            if explicit and k > 8:                               # given levels outside 0..3: the ROI contributes nothing
                for j, bad_l in zip(rng.choice(k, 3, replace=False), (-1, 4, 9)):
                    levels[j] = bad_l
            if "bad" in flags:
                rows = rng.choice(k, 7, replace=False)
                for j, b in zip(rows[:5], (float(n), -1.0, NAN, INF, float(n + 5))):
                    rois[j, 0] = b
                rois[rows[5], 1:] = NAN                          # a box of NaNs
                rois[rows[6], 1:3] = NAN                         # ... and one whose origin alone is no number
                keep[rows[5:]] = False                           # the references cannot take a NaN position: left out there
                tags.add("bad_rois")
        rois = torch.from_numpy(rois.astype(np.float32))
        ref_levels = torch.zeros(k, dtype=torch.int64)
        kp = torch.from_numpy(keep)
        if explicit:
            levels = torch.from_numpy(levels.astype(np.int32))
            ref_levels = levels.to(torch.int64)
            tags.add("explicit_levels")
            if bool(((levels < 0) | (levels > 3)).any()):
                tags.add("levels_out_of_range")
        else:
            ref_levels[kp] = OD.map_levels(rois[kp][:, 1:], 2, 5)
            tags.add("mapped_levels")
        dout = torch.from_numpy(rng.standard_normal((k, p, p, c)).astype(np.float32))
        # tags from the operands
        r64 = rois.numpy().astype(np.float64)
        bucket = np.array([(int(r64[i, 0]) * 4 + int(ref_levels[i])) if keep[i] and _inside(r64[i], int(ref_levels[i]), n, hws, scales)
                           else -1 for i in range(k)])
        counts = np.bincount(bucket[bucket >= 0], minlength=n * 4)
        if k > 256 and counts.max() > 256:
            ok = True
            for b0 in range(256, k, 256):                        # two buckets have members on both sides of every boundary
                lo, hi = set(bucket[max(b0 - 256, 0):b0].tolist()) - {-1}, set(bucket[b0:b0 + 256].tolist()) - {-1}
                ok = ok and len(lo & hi) >= 2
            if ok:
                tags.add("k_gt_256")
        if (counts == 0).any():
            tags.add("empty_bucket")
        if c > 256:
            tags.add("c_second_chunk")
        if c == 260:
            tags.add("c_ragged_chunk")
        if p == 32:
            tags.add("p32")
        if any(hw == (1, 1) for hw in hws):
            tags.add("one_by_one_level")
        tl = [sorted(((h + 7) // 8, (w + 7) // 8)) for h, w in hws]
        if any(a >= 5 and b >= 6 for a, b in tl):
            tags.add("many_tiles")
        cost = sum(hws[int(ref_levels[i])][0] * hws[int(ref_levels[i])][1] for i in range(k)
                   if keep[i] and 0 <= int(ref_levels[i]) < 4 and np.isfinite(r64[i, 0]) and 0 <= r64[i, 0] < n) * p * p * c
        yield dict(name=f"roi{idx}_N{n}_P{p}_sr{sr}_C{c}_K{k}", N=n, P=p, sr=sr, C=c, K=k, hws=[tuple(x) for x in hws], scales=scales,
                   rois=rois, levels=levels, ref_levels=ref_levels, keep=kp, dout=dout, tags=tags, roi_reference_cost=cost)


def roi_reference(case):
    """``fpn_train_refs.roi_align_bwd_scatter`` of a case: per level (sum, A, T).  ROIs whose origin is NaN are left out (every
    sample position is then NaN and the kernel gives them nothing); bad image indices and levels stay in, the reference skips
    them itself.  A box with a NaN far corner alone is not drawn: the extent clamp fmaxf(x2 - x1, 1) turns it into a box one
    pixel wide, in the forward kernel and in the adjoint alike, and the float64 oracle has no such rule to compare with."""
    kp = case["keep"]
    return FR.roi_align_bwd_scatter(case["dout"][kp], case["rois"][kp], case["ref_levels"][kp], case["hws"], case["scales"],
                                    case["sr"], case["N"])


# ------------------------------------------------------------------------------------------------ RPN window scatter
# L, N, C, M, maps (None: drawn from 1 x 1 ... 12 x 15), flags
SCATTER_SPECS = [
    (1, 1, 4, 1, [(1, 1)], set()),
    (3, 2, 8, 37, "fixture", set()),
    (8, 2, 8, 300, None, set()),
    (8, 4, 72, 300, None, {"bad"}),
    (8, 1, 64, 2000, None, set()),
    (2, 1, 4, 300, [(6, 7), (3, 4)], {"pile"}),
    (3, 2, 72, 300, [(12, 15), (5, 5), (2, 3)], {"pile"}),
    (5, 3, 256, 37, None, set()),
    (4, 2, 256, 300, None, {"bad"}),
    (1, 4, 64, 2000, [(12, 15)], set()),
    (6, 2, 4, 2000, [(1, 1), (12, 15), (1, 1), (7, 2), (3, 9), (1, 6)], {"bad"}),
    (8, 3, 4, 37, None, {"bad"}),
    (2, 1, 72, 1, [(4, 4), (2, 2)], set()),
    (3, 2, 8, 300, [(1, 1), (1, 15), (12, 1)], set()),
    (7, 4, 64, 300, None, {"bad"}),
    (8, 2, 256, 300, None, set()),
    (3, 1, 8, 2000, [(9, 11), (4, 4), (1, 1)], {"pile"}),
    (4, 3, 72, 2000, None, set()),
    (5, 2, 64, 37, [(1, 1), (2, 2), (3, 3), (1, 1), (5, 4)], set()),
    (8, 4, 8, 2000, None, {"bad", "pile"}),
]


def rpn_scatter_cases():
    for idx, (l, n, c, m, hws, flags) in enumerate(SCATTER_SPECS):
        rng = np.random.RandomState(2000 + idx)
        tags = set()
        if hws == "fixture":
            hws, rows = list(FR.SCATTER_HWS), FR.scatter_rows().numpy().astype(np.int64)
        else:
            if hws is None:
                hws = [(int(rng.randint(1, 13)), int(rng.randint(1, 16))) for _ in range(l)]
            rows = np.zeros((m, 4), np.int64)
            for r in range(m):
                lv = int(rng.randint(l))
                rows[r] = (rng.randint(n), lv, rng.randint(hws[lv][0]), rng.randint(hws[lv][1]))
            if "pile" in flags:                                  # 250 rows inside one 3 x 3 neighbourhood of the largest map
                lv = int(np.argmax([h * w for h, w in hws]))
                h, w = hws[lv]
                y0, x0, im = int(rng.randint(h)), int(rng.randint(w)), int(rng.randint(n))
                for r in rng.choice(m, min(250, m), replace=False):
                    rows[r] = (im, lv, min(max(y0 + rng.randint(-1, 2), 0), h - 1), min(max(x0 + rng.randint(-1, 2), 0), w - 1))
            if "bad" in flags:
                h0, w0 = hws[0]
                bad = [(-1, 0, 0, 0), (n, 0, 0, 0), (0, -1, 0, 0), (0, l, 0, 0), (0, 0, -1, 0), (0, 0, h0, 0), (0, 0, 0, -1), (0, 0, 0, w0),
                       (0, 0, 1 << 30, 0), (0, 0, 0, -(1 << 31)), (1 << 20, 0, 0, 0), (0, 8, 0, 0)]
                for r, b in zip(rng.choice(m, len(bad), replace=False), bad):
                    rows[r] = b
        hws = [tuple(x) for x in hws]
        ok = np.array([0 <= i < n and 0 <= lv < l and 0 <= y < hws[lv][0] and 0 <= x < hws[lv][1] for i, lv, y, x in rows.tolist()])
        if not ok.all():
            tags.add("bad_rows")
        if l == 8:
            tags.add("l8")
        if (c // 4) % 16:
            tags.add("c_ragged")
        if any(hw == (1, 1) for hw in hws):
            tags.add("one_by_one_map")
        # rows per 3 x 3 neighbourhood: every row within one pixel of (y, x) reaches (y, x)
        reach = {}
        for i, lv, y, x in rows[ok].tolist():
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if 0 <= y + dy < hws[lv][0] and 0 <= x + dx < hws[lv][1]:
                        reach[(i, lv, y + dy, x + dx)] = reach.get((i, lv, y + dy, x + dx), 0) + 1
        if reach and max(reach.values()) >= 200:
            tags.add("pile_up")
        dp = torch.from_numpy(rng.standard_normal((rows.shape[0], 3, 3, c)).astype(np.float32))
        yield dict(name=f"scatter{idx}_L{l}_N{n}_C{c}_M{rows.shape[0]}", L=l, N=n, C=c, M=rows.shape[0], hws=hws,
                   rows=torch.from_numpy(rows.astype(np.int32)), dpatch=dp, tags=tags)


# ------------------------------------------------------------------------------------------------ top-down merge
# fine, coarse, C, N
UPSAMPLE_SPECS = [
    ((8, 10), (8, 10), 12, 2), ((1, 1), (1, 1), 4, 1), ((7, 5), (7, 5), 256, 1),
    ((8, 10), (4, 5), 12, 3), ((6, 4), (3, 2), 256, 2),
    ((25, 21), (13, 11), 12, 2), ((13, 11), (7, 6), 4, 1),
    ((9, 12), (3, 4), 12, 2), ((15, 6), (5, 2), 256, 1), ((10, 15), (2, 3), 4, 3), ((20, 5), (4, 1), 12, 1),
    ((25, 18), (9, 7), 12, 2), ((23, 31), (5, 9), 4, 1), ((17, 3), (6, 2), 256, 1),
    ((4, 5), (8, 10), 12, 2), ((3, 9), (7, 4), 4, 3), ((1, 1), (5, 6), 12, 1), ((5, 7), (6, 7), 256, 1), ((2, 30), (9, 11), 4, 2),
    ((12, 15), (1, 1), 12, 2), ((41, 1), (1, 1), 4, 1), ((3, 3), (1, 1), 256, 3), ((6, 8), (1, 4), 12, 1),
    ((40, 41), (8, 14), 4, 1), ((9, 9), (4, 4), 12, 2),
]


def _ratio_tags(fine, coarse):
    tags = set()
    for f, c in zip(fine, coarse):
        if c > f:
            tags.add("coarse_gt_fine")
        elif c == f:
            tags.add("ratio1")
        elif f == 2 * c:
            tags.add("ratio2")
        elif f % c:
            tags.add("ratio2_odd" if f == 2 * c - 1 else "ratio_fraction")
        if f >= 3 * c:
            tags.add("ratio_ge3")
    if tuple(coarse) == (1, 1):
        tags.add("coarse_1x1")
    return tags


def upsample_add_bwd_cases():
    for idx, (fine, coarse, c, n) in enumerate(UPSAMPLE_SPECS):
        rng = np.random.RandomState(3000 + idx)
        tags = _ratio_tags(fine, coarse)
        dl = torch.from_numpy(rng.standard_normal((n, fine[0], fine[1], c)).astype(np.float32))
        base = None
        if idx % 2 == 0:
            base = torch.from_numpy(rng.standard_normal((n, coarse[0], coarse[1], c)).astype(np.float32))
            tags.add("with_base")
        yield dict(name=f"up{idx}_{fine[0]}x{fine[1]}_to_{coarse[0]}x{coarse[1]}_C{c}_N{n}", fine=fine, coarse=coarse, C=c, N=n,
                   dlat=dl, base=base, tags=tags)


# N, H, W, C
SUBSAMPLE_SPECS = [(1, 1, 1, 4), (2, 1, 9, 12), (1, 8, 1, 4), (2, 7, 6, 12), (1, 19, 19, 4), (3, 18, 2, 12), (1, 2, 2, 256),
                   (2, 5, 16, 256), (1, 13, 4, 4), (2, 6, 19, 12)]


def subsample_add_bwd_cases():
    for idx, (n, h, w, c) in enumerate(SUBSAMPLE_SPECS):
        rng = np.random.RandomState(4000 + idx)
        tags = {f"h_{'odd' if h % 2 else 'even'}", f"w_{'odd' if w % 2 else 'even'}"}
        if h == 1 or w == 1:
            tags.add("one_wide")
        d = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32))
        dp = torch.from_numpy(rng.standard_normal((n, (h - 1) // 2 + 1, (w - 1) // 2 + 1, c)).astype(np.float32))
        yield dict(name=f"sub{idx}_{n}x{h}x{w}x{c}", N=n, H=h, W=w, C=c, d=d, dpool=dp, tags=tags)


# ------------------------------------------------------------------------------------------------ stride-2 input gradient
# N, H, W, C, K
DGRAD_SPECS = [
    (2, 7, 9, 96, 32), (1, 8, 10, 96, 256), (1, 1, 11, 192, 64), (2, 9, 1, 192, 256), (1, 9, 11, 256, 256), (1, 6, 8, 512, 512),
    (1, 5, 7, 512, 96), (1, 4, 4, 256, 512), (2, 17, 18, 96, 32), (2, 17, 19, 256, 64), (1, 2, 2, 64, 96), (3, 5, 5, 128, 32),
    (1, 7, 6, 32, 512), (1, 9, 11, 512, 256), (2, 3, 4, 192, 96), (1, 1, 1, 64, 64),
]


def conv3x3s2_dgrad_cases():
    for idx, (n, h, w, c, k) in enumerate(DGRAD_SPECS):
        rng = np.random.RandomState(5000 + idx)
        bn = 128 if c % 128 == 0 else 64 if c % 64 == 0 else 32
        tags = {f"h_{'odd' if h % 2 else 'even'}", f"w_{'odd' if w % 2 else 'even'}"}
        if c // bn > 1:
            tags.add(f"bn{bn}_grid_y_gt1")
        if k > c:
            tags.add("k_gt_c")
        if k < c:
            tags.add("k_lt_c")
        if (c, k) == (512, 512):
            tags.add("real_512")
        if h == 1 or w == 1:
            tags.add("one_wide")
        if max(n * ((h + 1 - a) // 2) * ((w + 1 - b) // 2) for a in (0, 1) for b in (0, 1)) > 128:
            tags.add("class_wider_than_a_tile")
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        dy = torch.from_numpy(rng.standard_normal((n, ho, wo, k)).astype(np.float32))
        wt = torch.from_numpy((rng.standard_normal((k, c, 3, 3)) * 0.1).astype(np.float32))
        scale = torch.from_numpy((rng.rand(k) + 0.5).astype(np.float32))
        mask = rng.standard_normal((n, h, w, c)).astype(np.float32)
        mask.reshape(-1)[::7] = 0.0                               # y == 0 and the negative zero count as "not positive"
        mask.reshape(-1)[3::11] = -0.0
        yield dict(name=f"dgrad{idx}_{n}x{h}x{w}_C{c}_K{k}", N=n, H=h, W=w, C=c, K=k, dy=dy, w=wt, scale=scale,
                   mask=torch.from_numpy(mask), tags=tags)


def dgrad_reference(case, with_scale):
    """(dx, A, T): the float64 input gradient of ``test_gpu_body_train.py::case``, the same transposed convolution of |dy| with
    |w * scale|, and the number of terms of each element -- taps(class) * K with 1, 2, 2, 4 taps by row and column parity."""
    import torch.nn.functional as F
    n, h, w, c, k = (case[x] for x in "NHWCK")
    wt = case["w"].double()
    if with_scale:
        wt = wt * case["scale"].double().view(-1, 1, 1, 1)
    out = []
    for dy, ww in ((case["dy"].double(), wt), (case["dy"].double().abs(), wt.abs())):
        x = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, ww, None, 2, 1)
        y.backward(dy.permute(0, 3, 1, 2))
        out.append(x.grad.permute(0, 2, 3, 1).contiguous())
    taps = (1 + (torch.arange(h) % 2))[:, None] * (1 + (torch.arange(w) % 2))[None, :]
    t = (taps * k).double()[None, :, :, None].expand(n, h, w, c)
    return out[0], out[1], t


# ------------------------------------------------------------------------------------------------ stem pool adjoint
# N, H, W, C
POOL_SPECS = [(1, 1, 1, 4), (1, 3, 5, 8), (1, 5, 2, 4), (2, 4, 7, 8), (1, 9, 9, 64), (3, 4, 6, 4), (1, 13, 1, 8), (2, 8, 8, 64),
              (1, 6, 40, 64), (1, 9, 35, 64), (1, 5, 70, 64), (2, 4, 67, 64), (3, 2, 33, 64), (1, 1, 70, 8), (1, 22, 10, 8),
              (1, 2, 2, 4)]


def maxpool3s2_relu_bwd_cases():
    """y on the grid k/4 and dpool on k/64 as ``test_gpu_stem_train.py::pool_case``: positive ties are the rule, every sum of up
    to four terms is exact in fp32."""
    for idx, (n, h, w, c) in enumerate(POOL_SPECS):
        rng = np.random.RandomState(6000 + idx)
        ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        nchunks = (wo * (c // 4) + 255) // 256
        tags = {f"xcd_rem_{(n * ho * nchunks) % 8}", f"nchunks_{nchunks}", f"h_{'odd' if h % 2 else 'even'}",
                f"w_{'odd' if w % 2 else 'even'}"}
        if h == 1 or w == 1:
            tags.add("one_wide")
        y = (rng.randint(-4, 9, (n, h, w, c)).astype(np.float32)) / 4
        y.reshape(-1)[1::7] = -0.0
        dpool = rng.randint(-256, 257, (n, ho, wo, c)).astype(np.float32) / 64
        yield dict(name=f"pool{idx}_{n}x{h}x{w}x{c}", N=n, H=h, W=w, C=c, y=torch.from_numpy(y), dpool=torch.from_numpy(dpool), tags=tags)


# M, C
RELU_SPECS = [(1, 4), (3, 12), (7, 36), (16, 64), (86, 12), (29, 36), (64, 64), (1025, 4), (65, 64), (114, 36)]


def relu_mask_add_cases():
    for idx, (m, c) in enumerate(RELU_SPECS):
        rng = np.random.RandomState(7000 + idx)
        y, a, b = (rng.standard_normal((m, c)).astype(np.float32) for _ in range(3))
        y.reshape(-1)[::3] = 0.0
        y.reshape(-1)[1::5] = -0.0
        a.reshape(-1)[::4] = -0.0                                  # (-0) + (-0) stays a negative zero where y > 0
        b.reshape(-1)[::2] = -0.0
        lanes = m * c // 4
        tags = {"with_b" if idx % 2 == 0 else "without_b"}
        if lanes > 1024:
            tags.add("over_1024_lanes")
        if lanes % 256:
            tags.add("ragged_block")
        if c % 16:
            tags.add("c_only_multiple_of_4")
        yield dict(name=f"relu{idx}_M{m}_C{c}", M=m, C=c, y=torch.from_numpy(y), a=torch.from_numpy(a),
                   b=torch.from_numpy(b) if idx % 2 == 0 else None, tags=tags)


GENERATORS = {
    "roi_align_bwd": roi_align_bwd_cases,
    "rpn_scatter": rpn_scatter_cases,
    "upsample_add_bwd": upsample_add_bwd_cases,
    "subsample_add_bwd": subsample_add_bwd_cases,
    "conv3x3s2_dgrad": conv3x3s2_dgrad_cases,
    "maxpool3s2_relu_bwd": maxpool3s2_relu_bwd_cases,
    "relu_mask_add": relu_mask_add_cases,
}

REQUIRED = {
    "roi_align_bwd": dict(k_gt_256=4, c_second_chunk=3, c_ragged_chunk=2, p32=2, one_by_one_level=2, many_tiles=4, tile_border_edges=4,
                          explicit_levels=4, levels_out_of_range=4, mapped_levels=4, empty_bucket=4, bad_rois=3),
    "rpn_scatter": dict(l8=3, c_ragged=3, pile_up=3, bad_rows=3, one_by_one_map=3),
    "upsample_add_bwd": dict(ratio1=2, ratio2=2, ratio2_odd=2, ratio_ge3=4, ratio_fraction=2, coarse_gt_fine=4, coarse_1x1=3, with_base=10),
    "subsample_add_bwd": dict(h_odd=3, h_even=3, w_odd=3, w_even=3, one_wide=3),
    "conv3x3s2_dgrad": dict(bn32_grid_y_gt1=2, bn64_grid_y_gt1=2, bn128_grid_y_gt1=4, k_gt_c=4, k_lt_c=4, real_512=1, h_odd=3, h_even=3,
                            w_odd=3, w_even=3, one_wide=2, class_wider_than_a_tile=2),
    "maxpool3s2_relu_bwd": dict({f"xcd_rem_{r}": 1 for r in range(8)}, nchunks_1=4, nchunks_2=2, nchunks_3=2, h_odd=3, h_even=3,
                                w_odd=3, w_even=3, one_wide=3),
    "relu_mask_add": dict(with_b=4, without_b=4, over_1024_lanes=2, ragged_block=4, c_only_multiple_of_4=4),
}
CASES = {"roi_align_bwd": 30, "rpn_scatter": 20, "upsample_add_bwd": 25, "subsample_add_bwd": 10, "conv3x3s2_dgrad": 16,
         "maxpool3s2_relu_bwd": 16, "relu_mask_add": 10}
