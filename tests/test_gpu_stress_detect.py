"""Stress of the detection post-process kernels (``csrc/seam_detect.hip``, ``csrc/seam_paste.h``) against the plain references of
``detect_refs.py``, in the manner of ``test_gpu_stress_rpn_train.py``: seeded, in-process, every output POISONED (a NaN pattern /
a sentinel integer) between two guard regions that are checked after the launch; every launch runs twice (once through the C
ABI into the guarded buffer, once through ``ops.*``, or twice into fresh guarded buffers where ``ops`` takes the outputs) and
the two results must be bit-identical.  A refused call must leave every output untouched.  Nothing here provokes a fault:
out-of-range arguments are refused on the host before any launch, and no label or index out of range is passed.

What is exact and what is bounded (the counts are derived in ``detect_refs``' docstring, none is measured on a kernel):

* NMS, ``batched_nms_images``: lattice boxes only; survivors EQUAL the sequential reference (the only rounding is one
  correctly rounded division, reproduced from exact integers).  Every random set holds >= 5 pairs exactly at 0.5 and at 0.25.
* RPN top-k: the index order EQUALS ``rpn_topk_ref`` (NaN ranks last, -0 ties with +0, ties lowest anchor first -- the rule at
  ``rpn_key``, which is not ``torch.sort``'s: that puts NaN first); boxes are bit-identical to ``ops.decode_boxes`` on the
  gathered rows; scores within SIGMOID_ROUNDINGS = 4 roundings of the float64 sigmoid, sigmoid(+inf) = 1, sigmoid(-inf) = 0
  and a NaN logit gives a NaN score (pinned as they are).
* decode_boxes: within DECODE_ROUNDINGS = 8 roundings x 2^-24 x the sum of the absolute terms, plus (|dw| + 2) x 2^-24 x |pw| / 2
  for the rounded exponent and a 1-ulp ``expf`` (HIP's math-API documentation; ``heads_refs.py`` uses the same figure).  A NaN
  dw / dh gives the clamped size (``fminf`` returns its other operand): pinned, torchvision would give NaN.
* mask_select: the 4-rounding sigmoid bound; paste_masks: PASTE_ROUNDINGS = 6 over the three interpolations, exact zeros
  outside the integer box; box_iou: bit-exact on lattice boxes (NaN at the same places), IOU_ROUNDINGS + 1 = 16 relative
  roundings on float boxes.
Each test prints its worst error / bound ratio; it must stay below 1."""
import numpy as np
import pytest
import torch

import detect_refs as DR
from stress_kit import POISON_WORD as POISON, Buf, P, st

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def _lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def _ops():
    import seam_match_rcnn_amd.ops as ops
    return ops


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


# ------------------------------------------------------------------------------------------------ NMS
def _nms(boxes, thr, max_keep=0):
    """boxes [B,N,4] numpy -> keep bool [B,N]: the C ABI into guarded buffers, then ops.nms_sorted; bit-identical."""
    lib, ops = _lib(), _ops()
    b, n = boxes.shape[:2]
    nb = (n + 63) // 64
    d = dev(boxes)
    keep = Buf((b, n), torch.int32)
    ws = Buf((b * n * nb,), torch.int64)
    rc = lib.seam_nms_sorted_topn_f32(P(d), P(keep.t), b, n, float(thr), int(max_keep), P(ws.t), st())
    torch.cuda.synchronize()
    assert rc == 0 and keep.guard_ok() and ws.guard_ok() and keep.filled(), (b, n, thr, max_keep)
    again = ops.nms_sorted(d if b > 1 else d[0], thr, max_keep=max_keep).reshape(b, n)
    got = keep.t.cpu()
    assert torch.equal(got, again.cpu()), (b, n, thr, max_keep)
    assert bool(((got == 0) | (got == 1)).all())
    words = ws.t.cpu().numpy().view(np.uint64).reshape(b, n, nb) if n <= 700 else None
    return got.numpy().astype(bool), words


def _nms_against_ref(boxes, thr, max_keep=0, require_ties=False):
    """Survivors against the sequential reference and, for the smaller sets, the workspace's bit matrix against the full table:
    word (i, jb) for jb >= i / 64 holds IoU(i, j) > thr for the columns j > i of its block and zeros elsewhere (the diagonal and
    everything left of it, columns >= N); the words left of the diagonal block are never written."""
    got, words = _nms(boxes, thr, max_keep)
    n = boxes.shape[1]
    for i in range(boxes.shape[0]):
        ref = DR.greedy_nms_ref(boxes[i], thr, max_keep)
        assert np.array_equal(got[i], ref), (boxes.shape, thr, max_keep, i, np.nonzero(got[i] != ref)[0][:8])
        if words is not None:
            table = np.triu(DR.nms_mask_ref(boxes[i], thr, require_ties=require_ties), 1)
            nb = words.shape[2]
            bits = ((words[i][:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(n, nb * 64)
            written = np.repeat(np.arange(nb)[None, :] >= (np.arange(n) // 64)[:, None], 64, 1)
            want = np.zeros((n, nb * 64), bool)
            want[:, :n] = table
            assert np.array_equal(bits[written], want[written]), (boxes.shape, thr, i)
            poison = np.uint64(POISON) | (np.uint64(POISON) << np.uint64(32))
            assert (words[i][~written[:, ::64]] == poison).all(), (boxes.shape, thr, i)
        elif require_ties:                                                  # ties among the first 1000 boxes are ties of the set
            DR.nms_mask_ref(boxes[i][:1000], thr, require_ties=True)
    return got


def _far_apart(n):
    """n unit squares, none touching another, none near the origin (where the chain goes)."""
    i = np.arange(n)
    x, y = 20 + 2 * (i % 20), 2 * (i // 20)
    return np.stack([x, y, x + 1, y + 1], 1).astype(np.float32)


THRESHOLDS = (0.5, 0.25, 0.3, 0.7, 0.0, 1.0, -1.0)


def test_stress_nms_sizes_and_thresholds():
    for n in (1, 2, 63, 64, 65, 127, 128, 129, 4097):
        for b in (1, 3):
            rng = np.random.RandomState(1000 * b + n)
            boxes = np.stack([DR.lattice_boxes(rng, n) for _ in range(b)])
            assert b == 1 or n == 1 or not np.array_equal(boxes[0], boxes[1])
            thrs = THRESHOLDS if (n < 4097 or b == 1) else (0.5, 0.25)
            for thr in thrs:
                # every random set of 63 or more boxes must hold >= MIN_TIES pairs exactly at 0.5 and at 0.25
                got = _nms_against_ref(boxes, thr, require_ties=n >= 63 and thr in DR.TIE_THRESHOLDS)
                assert got[:, 0].all()


def test_stress_nms_compositions():
    n = 130
    rng = np.random.RandomState(7)
    one = DR.lattice_boxes(rng, 1, zero_frac=0.0, plant=False)
    same = np.repeat(one, n, 0)[None]
    for thr in (0.5, 0.0, 0.7):
        assert _nms_against_ref(same, thr).sum() == 1                       # all identical: one survivor
    got = _nms_against_ref(same, 1.0)                                       # exact duplicates at 1.0: kept, > is strict
    assert got.all()
    apart = _far_apart(n)[None]
    for thr in (0.0, 0.5):
        assert _nms_against_ref(apart, thr).all()                           # all disjoint: all survive
    i = np.arange(n)
    tiles = np.stack([i % 13, i // 13, i % 13 + 1, i // 13 + 1], 1).astype(np.float32)[None]
    assert _nms_against_ref(tiles, 0.0).all()                               # touching edges: inter = 0 is not > 0
    assert _nms_against_ref(tiles, -1.0).sum() == 1                         # ... but 0 > -1
    pts = DR.lattice_boxes(rng, n, plant=False)
    pts[:, 2] = pts[:, 0]                                                   # zero width; every third one a point
    pts[::3, 3] = pts[::3, 1]
    pts[1::2] = pts[0]                                                      # many coincide: 0/0
    for thr in (0.5, 0.0, -1.0, 1.0):
        assert _nms_against_ref(pts[None], thr).all()                       # 0/0 is NaN: suppresses nothing, is not suppressed
    mixed = DR.lattice_boxes(rng, n)
    mixed[::5, 2] = mixed[::5, 0]
    _nms_against_ref(mixed[None], 0.25)
    _nms_against_ref(mixed[None], -1.0)
    # the non-transitive chain A > B, B ~ C, A !~ C across the 64-box block boundary: C survives
    for pa, pb, pc in ((62, 63, 64), (63, 64, 65), (64, 65, 66), (62, 64, 66), (0, 63, 129), (63, 127, 128)):
        boxes = _far_apart(n)
        boxes[[pa, pb, pc]] = DR.CHAIN
        for thr in (0.0, 0.25, 0.3):
            got = _nms_against_ref(boxes[None], thr)[0]
            assert got[pa] and not got[pb] and got[pc] and got.sum() == n - 1, (pa, pb, pc, thr)


def test_stress_nms_max_keep():
    """``max_keep`` against the reference's own cut (not against the full scan's).  What this pins is the result: the scan's early
    exit is an optimisation the output cannot show -- without it a later block finds no room left, drops all of its survivors
    and writes the same zeros -- so turning ``total >= max_keep`` into ``>`` changes the time, not a bit."""
    rng = np.random.RandomState(11)
    n = 200
    boxes = np.stack([DR.lattice_boxes(rng, n) for _ in range(2)])
    pt = np.array([3.25, 5.5, 3.25, 5.5], np.float32)
    boxes[:, 63], boxes[:, 64], boxes[:, 127], boxes[:, 128] = pt, pt, pt, pt          # points always survive at thr >= 0
    full = _nms_against_ref(boxes, 0.5, require_ties=True)
    assert full[:, [63, 64, 127, 128]].all()
    count = np.cumsum(full, 1)
    total = int(count[0, -1])
    assert 4 < total < n
    # 1; the survivor count and one less / more; the counts reached by the last box of a block and by the first of the next
    # (the early exit and the zero fill behind it); more than there are boxes
    for mk in sorted({1, 2, total - 1, total, total + 1, int(count[0, 63]), int(count[0, 64]), int(count[0, 127]),
                      int(count[0, 128]), int(count[1, 63]), int(count[1, 64]), n, n + 5}):
        got = _nms_against_ref(boxes, 0.5, max_keep=mk)
        assert np.array_equal(got, full & (count <= mk)), mk
    one = np.stack([DR.lattice_boxes(rng, 65)])
    for mk in (1, 64, 65, 70):
        _nms_against_ref(one, 1.0, max_keep=mk)                             # everything survives: the cut alone decides


def test_stress_nms_batched_classes():
    from seam_match_rcnn_amd.models.detection import batched_nms_images
    rng = np.random.RandomState(13)
    b, n = 2, 600
    boxes = np.stack([DR.lattice_boxes(rng, n) for _ in range(b)])
    scores = np.stack([rng.permutation(n) for _ in range(b)]).astype(np.float32) / n
    cls = rng.randint(0, 13, (b, n))
    cls[:, :13] = np.arange(13)
    valid = rng.rand(b, n) > 0.25
    valid[1, ::7] = False
    args = [dev(boxes), dev(scores), dev(cls), dev(valid)]
    for thr, top_n in ((0.5, 60), (0.25, 1000), (0.3, 17)):
        refs = [DR.batched_nms_ref(boxes[i], scores[i], cls[i], valid[i], thr, top_n) for i in range(b)]
        order, sel, exact = batched_nms_images(*args, thr, top_n)
        order2, sel2, _ = batched_nms_images(*args, thr, top_n)
        assert bool(exact.all()) and torch.equal(order, order2) and torch.equal(sel, sel2)
        for i in range(b):
            assert np.array_equal(order[i][sel[i]].cpu().numpy(), refs[i]), (thr, top_n, i)
        # the prefix form: exact where it says so, and always a leading part of the truth
        for prefix in (64, 200, 599, 600, 700):
            order_p, sel_p, exact_p = batched_nms_images(*args, thr, top_n, prefix=prefix)
            for i in range(b):
                got = order_p[i][sel_p[i]].cpu().numpy()
                assert np.array_equal(got, refs[i][:len(got)]), (thr, top_n, prefix, i)
                if bool(exact_p[i]):
                    assert len(got) == len(refs[i]), (thr, top_n, prefix, i)
            assert bool(exact_p.all()) or prefix < 600


def test_stress_nms_refusals():
    lib = _lib()
    z = torch.zeros((64,), device=DEV)
    for b_, n_, mk_ in ((1, 16385, 0), (1, 8, -1), (65536, 1, 0)):
        keep, ws = Buf((16,), torch.int32), Buf((16,), torch.int64)
        rc = lib.seam_nms_sorted_topn_f32(P(z), P(keep.t), b_, n_, 0.5, mk_, P(ws.t), st())
        torch.cuda.synchronize()
        assert rc != 0 and keep.untouched() and ws.untouched() and keep.guard_ok() and ws.guard_ok(), (b_, n_, mk_)


# ------------------------------------------------------------------------------------------------ RPN top-k
def _logits(rng, n, kind):
    f = np.float32
    if kind == "inf":
        x = rng.normal(0, 3, n).astype(f)
        x[rng.rand(n) < 0.1] = np.inf
        x[rng.rand(n) < 0.1] = -np.inf
    elif kind == "nan":
        x = (np.round(rng.normal(0, 3, n) * 2) / 2).astype(f)
        x[rng.rand(n) < 0.2] = np.nan
        x[rng.rand(n) < 0.05] = -np.inf                                     # NaN ties with -inf, lowest index first
    elif kind == "all_nan":
        x = np.full(n, np.nan, f)
    elif kind == "zeros":
        x = np.where(rng.rand(n) < 0.5, f(0.0), f(-0.0)).astype(f)
        x[rng.rand(n) < 0.1] = -1.0
    elif kind == "denormal":
        x = (rng.randint(-6, 7, n) * 2.0 ** -149).astype(f)                 # +-0 .. +-6 steps of the smallest denormal
        x[rng.rand(n) < 0.2] = -0.0
    elif kind == "equal":
        x = np.full(n, 0.25, f)
    else:
        assert kind == "two"
        x = np.where(rng.rand(n) < 0.3, f(1.5), f(-2.0)).astype(f)
    return x


def _tie_k(x, kmax):
    """A k <= kmax whose k-th and (k+1)-th winners tie (the cut falls inside a tie group), nearest to kmax / 2; or None."""
    order = DR.rpn_topk_ref(x, len(x))
    key = np.nan_to_num(x.astype(np.float64), nan=-np.inf)[order]
    ks = [k for k in range(1, min(kmax, len(x) - 1) + 1) if key[k - 1] == key[k]]
    return min(ks, key=lambda k: abs(k - kmax // 2)) if ks else None


def _rpn_case(rng, logits, a, k, worst, index=True):
    """logits [n_img, n] -> one level through ops.rpn_topk_decode into guarded buffers at a row offset, twice; all checks."""
    ops = _ops()
    n_img, n = logits.shape
    hgt = n // a
    dlt = (rng.normal(0, 0.5, (n_img, n, 4))).astype(np.float32)
    xy = rng.uniform(-30, 300, (n, 2))
    anc = np.concatenate([xy, xy + rng.uniform(0, 120, (n, 2))], 1).astype(np.float32)
    clip = np.array([[211.5, 300.25], [97.0, 130.75]], np.float32)[:n_img]
    head = np.concatenate([logits.reshape(n_img, hgt, 1, a), dlt.reshape(n_img, hgt, 1, 4 * a)], 3)
    d_head, d_anc, d_clip = dev(head), dev(anc), dev(clip)
    off, ktot = 5, k + 11
    runs = []
    for _ in range(2):
        bx, sc, ix = Buf((n_img, ktot, 4), torch.float32), Buf((n_img, ktot), torch.float32), Buf((n_img, ktot), torch.int64)
        ops.rpn_topk_decode(d_head, a, d_anc, d_clip, k, bx.t, sc.t, off, ix.t if index else None)
        torch.cuda.synchronize()
        assert bx.guard_ok() and sc.guard_ok() and ix.guard_ok(), (n, a, k)
        runs.append((bx, sc, ix))
    for x, y in zip(*runs):
        assert torch.equal(x.bits(), y.bits()), (n, a, k)
    bx, sc, ix = runs[0]
    for t in (bx.t, sc.t):                                                  # rows before and behind the level: untouched
        rows = torch.cat([t[:, :off], t[:, off + k:]], 1).contiguous().view(torch.int32)
        assert bool((rows == POISON).all()), (n, a, k)
        assert not bool((t[:, off:off + k].contiguous().view(torch.int32) == POISON).any()), (n, a, k)
    if not index:
        assert ix.untouched()
        return bx.t[:, off:off + k].cpu(), sc.t[:, off:off + k].cpu()
    iw = ix.t.view(torch.int32).view(n_img, ktot, 2)
    assert bool((torch.cat([iw[:, :off], iw[:, off + k:]], 1) == POISON).all()), (n, a, k)
    got_ix = ix.t[:, off:off + k].cpu().numpy()
    got_sc = sc.t[:, off:off + k].cpu().numpy()
    for i in range(n_img):
        ref = DR.rpn_topk_ref(logits[i], k)
        assert np.array_equal(got_ix[i], ref), (n, a, k, i, np.nonzero(got_ix[i] != ref)[0][:8])
        want = ops.decode_boxes(dev(dlt[i][ref]), dev(anc[ref]), (1., 1., 1., 1.), (float(clip[i, 0]), float(clip[i, 1])))
        assert torch.equal(bx.t[i, off:off + k], want), (n, a, k, i)
        lg = logits[i][ref]
        nan = np.isnan(lg)
        assert np.array_equal(np.isnan(got_sc[i]), nan), (n, a, k, i)       # NaN logit -> NaN score (pinned)
        assert (got_sc[i][lg == np.inf] == 1.0).all() and (got_sc[i][lg == -np.inf] == 0.0).all()
        sref, sbound = DR.sigmoid_ref(lg[~nan])
        ratio = np.abs(got_sc[i][~nan].astype(np.float64) - sref) / sbound
        if ratio.size:
            worst[0] = max(worst[0], float(ratio.max()))
            assert ratio.max() <= 1.0, (n, a, k, i, float(ratio.max()))
    return bx.t[:, off:off + k].cpu(), sc.t[:, off:off + k].cpu()


RPN_KINDS = ("inf", "nan", "all_nan", "zeros", "denormal", "equal", "two")


@pytest.mark.parametrize("kind", RPN_KINDS)
def test_stress_rpn_topk_contents_and_sizes(kind):
    """n in {1, A, 1023, 1024, 1025, 3 * 1024 + 1, 5000} (A = 1; A = 3 where it divides n, and 3 * 1025); k = 1, the largest
    allowed, and a cut inside a tie group; +-inf, NaN (scattered / everywhere), +-0 mixed, denormals, one value, two values."""
    worst = [0.0]
    cases = 0
    for n, a in ((1, 1), (3, 3), (3, 1), (1023, 1), (1023, 3), (1024, 1), (1025, 1), (3 * 1024 + 1, 1), (5000, 1), (3075, 3)):
        rng = np.random.RandomState(100 * n + 10 * a + RPN_KINDS.index(kind))
        logits = np.stack([_logits(rng, n, kind) for _ in range(2)])
        ks = {1, n if n <= 1024 else 1024}
        tk = _tie_k(logits[0], min(n, 1024))
        if tk is not None:
            ks.add(tk)
        assert tk is not None or n <= 3
        for k in sorted(ks):
            _rpn_case(rng, logits, a, k, worst)
            cases += 1
    print(f"rpn_topk[{kind}]: {cases} cases, worst score error / bound = {worst[0]:.4f}")
    assert worst[0] < 1.0


def test_stress_rpn_topk_long_tie_walk_and_arguments():
    lib, ops = _lib(), _ops()
    worst = [0.0]
    rng = np.random.RandomState(5)
    # 10 winners above the tie value in the first 1024 indices; the tie group (1134 members) starts after index 1024 and ends
    # after 4096.  Room for 700 of them: the walk takes the rounds at 0 (nothing), 1024, 2048, 3072 and stops there; for 1 of
    # them: it stops after the round at 1024; for 1014 (k = 1024): it goes on into the round at 4096
    n = 5000
    x = np.full((2, n), -3.0, np.float32)
    x[:, rng.choice(1024, 10, replace=False)] = rng.normal(4, 0.5, 10).astype(np.float32)
    members = np.arange(1100, 4500, 3)
    x[:, members] = 0.5
    x[1, members[::2]] = -0.0                                               # image 1: the group is +0 / -0 mixed
    x[1, members[1::2]] = 0.0
    for k in (10 + 700, 11, 1024):
        ref = DR.rpn_topk_ref(x[0], k)
        assert ref[9] < 1024 and ref[10] == 1100
        assert k != 710 or 3072 < ref[-1] < 4096
        assert k != 1024 or ref[-1] > 4096
        _rpn_case(rng, x, 1, k, worst)
    # index=None: boxes and scores as with an index
    lg = np.stack([_logits(rng, 1025, "nan") for _ in range(2)])
    state = rng.get_state()
    with_ix = _rpn_case(rng, lg, 1, 300, worst)
    rng.set_state(state)
    without = _rpn_case(rng, lg, 1, 300, worst, index=False)
    assert torch.equal(with_ix[0], without[0]) and torch.equal(with_ix[1].view(torch.int32), without[1].view(torch.int32))
    print(f"rpn_topk tie walk: worst score error / bound = {worst[0]:.4f}")
    # refusals through the C ABI: k above the cap, k above n, n not a multiple of A; outputs untouched
    z = torch.zeros((4096,), device=DEV)
    for n_, a_, k_ in ((2000, 1, 1025), (8, 1, 9), (8, 3, 2), (8, 0, 2)):
        bx, sc, ix = Buf((16, 4), torch.float32), Buf((16,), torch.float32), Buf((16,), torch.int64)
        rc = lib.seam_rpn_topk_decode_f32(P(z), P(z), P(z), P(z), P(bx.t), P(sc.t), P(ix.t), 1, n_, a_, k_, n_, 1, 4 * n_, 4, 16, 0, st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in (bx, sc, ix)), (n_, a_, k_)
    with pytest.raises(ValueError):
        ops.rpn_topk_decode(torch.zeros((1, 2000, 1, 5), device=DEV), 1, torch.zeros((2000, 4), device=DEV),
                            torch.ones((1, 2), device=DEV), 1025, torch.zeros((1, 1025, 4), device=DEV),
                            torch.zeros((1, 1025), device=DEV), 0)


# ------------------------------------------------------------------------------------------------ decode_boxes
def _decode(deltas, boxes, weights, clip):
    lib, ops = _lib(), _ops()
    n, c4 = deltas.shape
    d_d, d_b = dev(deltas), dev(boxes)
    out = Buf((n, c4), torch.float32)
    ch, cw = (0.0, 0.0) if clip is None else clip
    rc = lib.seam_decode_boxes_f32(P(d_d), P(d_b), P(out.t), n, c4 // 4, *[float(w) for w in weights], float(ch), float(cw), st())
    torch.cuda.synchronize()
    assert rc == 0 and out.guard_ok(), (n, c4)
    again = ops.decode_boxes(d_d, d_b, weights, clip)
    assert torch.equal(out.t.view(torch.int32), again.view(torch.int32)), (n, c4)
    return out.t.cpu().numpy()


def test_stress_decode_boxes():
    worst = 0.0
    clip_x = float(np.float32(DR.XFORM_CLIP))
    above = float(np.nextafter(np.float32(clip_x), np.float32(np.inf)))
    for ncls in (1, 2, 14, 91):
        for n in (1, 255, 256, 257):
            for weights in ((1., 1., 1., 1.), (10., 10., 5., 5.)):
                for clip in ((97.5, 130.25), None):
                    rng = np.random.RandomState(ncls * 1000 + n)
                    xy = rng.uniform(-40, 140, (n, 2))
                    wh = rng.uniform(0, 90, (n, 2))
                    wh[rng.rand(n) < 0.15, 0] = 0.0                          # zero-width proposals
                    boxes = np.concatenate([xy, xy + wh], 1).astype(np.float32)
                    deltas = rng.normal(0, 1, (n, ncls, 4)) * np.array(weights) * np.array([0.3, 0.3, 0.6, 0.6])
                    deltas = deltas.astype(np.float32)
                    special = np.array([clip_x * weights[2], above * weights[2], 1e4, np.inf, -1e4, np.nan, -np.inf], np.float32)
                    pick = rng.randint(0, len(special) + 6, (n, ncls))       # about half of the rows get a special dw
                    sel = pick < len(special)
                    deltas[..., 2][sel] = special[pick[sel]]
                    deltas = deltas.reshape(n, ncls * 4)
                    got = _decode(deltas, boxes, weights, clip)
                    ref, bound = DR.decode_ref(deltas, boxes, weights, clip)
                    assert np.isfinite(got).all(), (ncls, n)                 # +inf, 1e4 and NaN give the clamped finite size
                    ratio = np.abs(got.astype(np.float64) - ref) / bound
                    worst = max(worst, float(ratio.max()))
                    assert ratio.max() <= 1.0, (ncls, n, weights, clip, float(ratio.max()))
                    g = got.reshape(n, ncls, 4)
                    zero = np.isin(pick, (4, 6)) | (wh[:, 0] == 0)[:, None]  # -1e4, -inf or a zero-width proposal: zero width
                    assert (g[..., 0][zero] == g[..., 2][zero]).all(), (ncls, n)
                    big = np.isin(pick, (0, 1, 2, 3, 5)) & (wh[:, 0] > 1)[:, None] & (clip is None)
                    want = np.broadcast_to(62.5 * (boxes[:, 2] - boxes[:, 0])[:, None].astype(np.float64), big.shape)[big]
                    assert (np.abs((g[..., 2] - g[..., 0])[big] - want) <= 1e-4 * want).all()      # the clamped size: 1000/16 widths
    print(f"decode_boxes: worst error / bound = {worst:.4f}")
    assert worst < 1.0
    # boxes wholly outside each side clip to a zero-size box on the border
    boxes = np.array([[-50., 10., -20., 30.], [200., 10., 230., 30.], [10., -60., 30., -40.], [10., 150., 30., 190.]], np.float32)
    got = _decode(np.zeros((4, 4), np.float32), boxes, (10., 10., 5., 5.), (97.5, 130.25))
    assert got.tolist() == [[0., 10., 0., 30.], [130.25, 10., 130.25, 30.], [10., 0., 30., 0.], [10., 97.5, 30., 97.5]]


# ------------------------------------------------------------------------------------------------ mask_select
def test_stress_mask_select():
    lib, ops = _lib(), _ops()
    worst = 0.0
    special = np.array([np.inf, -np.inf, 88., -88., 104., -104., 0.], np.float32)
    for k in (1, 7, 300):
        for ncls in (2, 14, 91):
            rng = np.random.RandomState(k * 100 + ncls)
            labels = rng.randint(0, ncls, k)
            labels[0] = ncls - 1
            if k > 1:
                labels[1] = 0
            logits = np.random.default_rng(k * 100 + ncls).standard_normal((k, 14, 14, 4 * ncls), dtype=np.float32)
            logits *= np.float32(4)
            flat = logits.reshape(k, 196 * 4, ncls)
            for i in range(k):                                              # the specials go into the selected channel
                pos = rng.choice(196 * 4, 28, replace=False)
                flat[i, pos, labels[i]] = np.tile(special, 4)
            for dtype in (torch.float32, torch.float16):
                d_log = dev(logits, dtype)
                stored = d_log.cpu().numpy()
                d_lab = dev(labels.astype(np.int64))
                out = Buf((k, 1, 28, 28), torch.float32)
                fn = lib.seam_mask_select_f32 if dtype == torch.float32 else lib.seam_mask_select_f16
                rc = fn(P(d_log), P(d_lab), P(out.t), k, ncls, st())
                torch.cuda.synchronize()
                assert rc == 0 and out.guard_ok() and out.filled(), (k, ncls, dtype)
                again = ops.mask_select(d_log, d_lab, ncls)
                assert torch.equal(out.t.view(torch.int32), again.view(torch.int32)), (k, ncls, dtype)
                got = out.t.cpu().numpy().astype(np.float64)
                x = DR.mask_select_ref(stored, labels)
                ref, bound = DR.sigmoid_ref(x)
                assert int(np.isinf(x).sum()) == 8 * k
                assert (got[x == np.inf] == 1.0).all() and (got[x == -np.inf] == 0.0).all()
                ratio = np.abs(got - ref) / bound
                worst = max(worst, float(ratio.max()))
                assert ratio.max() <= 1.0, (k, ncls, dtype, float(ratio.max()))
    print(f"mask_select: worst error / bound = {worst:.4f}")
    assert worst < 1.0


# ------------------------------------------------------------------------------------------------ paste_masks
def _paste(masks, boxes, hw):
    lib, ops = _lib(), _ops()
    k = masks.shape[0]
    d_m, d_b = dev(masks), dev(boxes)
    out = Buf((k, 1, hw[0], hw[1]), torch.float32)
    rc = lib.seam_paste_masks_f32(P(d_m), P(d_b), P(out.t), k, int(hw[0]), int(hw[1]), st())
    torch.cuda.synchronize()
    assert rc == 0 and out.guard_ok(), (k, hw)
    assert out.filled() and not bool(torch.isnan(out.t).any()), (k, hw)     # every pixel written, no poison left
    again = ops.paste_masks(d_m, d_b, hw)
    assert torch.equal(out.t.view(torch.int32), again.view(torch.int32)), (k, hw)
    return out.t.cpu().numpy()


def _paste_boxes(h, w):
    return np.array([
        [0.6 * w, 0.2 * h, 0.1 * w, 0.8 * h],              # inverted in x
        [0.1 * w, 0.9 * h, 0.7 * w, 0.3 * h],              # inverted in y
        [0.8 * w, 0.8 * h, 0.2 * w, 0.1 * h],              # inverted in both
        [0.5 * w, 0.5 * h, 0.5 * w, 0.5 * h],              # zero-size
        [0.3 * w + 0.2, 0.4 * h + 0.3, 0.3 * w + 0.7, 0.4 * h + 0.6],      # sub-pixel
        [-3.0 * w - 9, 0.1 * h, -1.5 * w - 4, 0.9 * h],    # wholly outside: left, right, above, below
        [2.5 * w + 4, 0.1 * h, 4.0 * w + 9, 0.9 * h],
        [0.1 * w, -3.0 * h - 9, 0.9 * w, -1.5 * h - 4],
        [0.1 * w, 2.5 * h + 4, 0.9 * w, 4.0 * h + 9],
        [-50., -50., w + 50., h + 50.],                    # the whole canvas and more
        [0., 0., float(w), float(h)],
        [-1e6, -1e6, 1e6, 1e6],                            # corners at +-1e6
        [-1e6, 0.25 * h, 0.5 * w, 1e6],
        [0.5 * w, -1e6, 1e6, 0.75 * h],
        [-0.3 * w, -0.2 * h, 0.6 * w, 0.7 * h],            # over a corner, over an edge, inside
        [0.4 * w, 0.3 * h, 1.3 * w, 0.8 * h],
        [0.2 * w + 0.3, 0.25 * h + 0.1, 0.7 * w + 0.4, 0.8 * h + 0.9],
    ], np.float32)


def _paste_against_ref(masks, boxes, hw, worst):
    got = _paste(masks, boxes, hw)
    ref, bound = DR.paste_ref(masks, boxes, hw)
    err = np.abs(got.astype(np.float64) - ref)
    assert (got[bound == 0] == 0).all(), hw                                 # outside the integer box: exact zeros
    inside = bound > 0
    if inside.any():
        ratio = float((err[inside] / bound[inside]).max())
        worst[0] = max(worst[0], ratio)
        assert ratio <= 1.0, (hw, ratio)
    return got, ref


def test_stress_paste_masks():
    worst = [0.0]
    rng = np.random.RandomState(17)
    for hw in ((1, 1), (1, 37), (37, 1), (64, 40)):
        boxes = _paste_boxes(*hw)
        masks = rng.rand(boxes.shape[0], 1, 28, 28).astype(np.float32)
        got, ref = _paste_against_ref(masks, boxes, hw, worst)
        assert got[5:9].max() == 0                                          # wholly outside
        if hw == (64, 40):                                                  # inverted by many pixels: x1 < x0, nothing is pasted
            assert got[:3].max() == 0                                       # (by less than one, the integer box is one pixel)
        assert ref[9].min() > 0 and ref[10].max() > 0                        # covering boxes: not a sweep of zeros
        _paste_against_ref(masks[9:10], boxes[9:10], hw, worst)             # K = 1
    # K = 40 on 64 x 40: the list again with shifted copies
    boxes = _paste_boxes(64, 40)
    boxes = np.concatenate([boxes, boxes + np.float32(0.37), boxes[:6] - np.float32(1.61)])
    assert boxes.shape[0] == 40
    masks = (rng.rand(40, 1, 28, 28).astype(np.float32) - np.float32(0.25))    # some negative entries: the bound uses |map|
    got, ref = _paste_against_ref(masks, boxes, (64, 40), worst)
    assert np.abs(ref).max() > 0.5 and (np.abs(ref) > 0).sum() > 10000
    # solid maps: hand-countable areas, so that the sweep cannot pass by agreeing on zeros
    ones = np.ones((4, 1, 28, 28), np.float32)
    solid = np.array([[10., 10., 37., 37.], [-50., -50., 90., 114.], [38., 62., 41., 66.], [20., 30., 20., 30.]], np.float32)
    got, ref = _paste_against_ref(ones, solid, (64, 40), worst)
    # [10,37]^2 grows by 30/28 to the integer box 9..37 (29 x 29 px, about one padded cell per pixel): a 27 x 27 core of ones
    # inside a one-pixel ring that mixes in the zero border, each of its values > 0 and <= 0.5
    assert int((got[0] > 0).sum()) == 29 * 29 and int((got[0] == 1).sum()) >= 25 * 25 and int((got[0] > 0.5).sum()) == 27 * 27
    assert got[0, 0, 9:38, 9:38].min() > 0 and got[0, 0, :9].max() == 0 and got[0, 0, 38:].max() == 0 and got[0, 0, :, :9].max() == 0
    assert (got[1] == 1.0).all()                                            # the canvas lies deep inside the box
    # a box over the bottom-right corner: integer box x 37..41, y 61..66 -> the canvas holds columns 37..39, rows 61..63
    assert int((got[2] > 0).sum()) == 3 * 3 and got[2, 0, 61:64, 37:40].min() > 0
    # a zero-size box is one pixel (size max(.., 1)) that samples the padded map's centre
    assert int((got[3] > 0).sum()) == 1 and got[3, 0, 30, 20] == 1.0
    # 513 x 512 = 262 656 pixels is the smallest canvas above 1024 blocks x 256 threads = 262 144: the grid-stride loop takes a
    # second trip for the last 512 pixels (K = 2: both grid rows do)
    hw = (513, 512)
    boxes = np.array([[-50., -50., 562., 563.], [100.3, 400.2, 480.9, 530.7]], np.float32)
    masks = rng.rand(2, 1, 28, 28).astype(np.float32)
    got, ref = _paste_against_ref(masks, boxes, hw, worst)
    assert got[0, 0, 512].min() > 0 and got[1, 0, 512, 100:480].max() > 0   # the second trip's row holds values
    got, _ = _paste_against_ref(np.ones((2, 1, 28, 28), np.float32), boxes, hw, worst)
    assert (got[0] == 1.0).all()
    print(f"paste_masks: worst error / bound = {worst[0]:.4f}")
    assert worst[0] < 1.0


# ------------------------------------------------------------------------------------------------ box_iou
def _iou(a, b):
    lib, ops = _lib(), _ops()
    d_a, d_b = dev(a), dev(b)
    out = Buf((a.shape[0], b.shape[0]), torch.float32)
    rc = lib.seam_box_iou_f32(P(d_a), P(d_b), P(out.t), a.shape[0], b.shape[0], st())
    torch.cuda.synchronize()
    assert rc == 0 and out.guard_ok() and out.filled(), (a.shape, b.shape)
    again = ops.box_iou(d_a, d_b)
    assert torch.equal(out.t.view(torch.int32), again.view(torch.int32)), (a.shape, b.shape)
    return out.t.cpu().numpy()


def test_stress_box_iou():
    worst = 0.0
    nans = 0
    for na, nb in ((1, 1), (5, 51), (16, 16), (1, 257), (257, 3)):
        rng = np.random.RandomState(na * 1000 + nb)
        a, b = DR.lattice_boxes(rng, na, zero_frac=0.2), DR.lattice_boxes(rng, nb, zero_frac=0.2)
        if na > 1:
            a[0] = (3., 4., 3., 4.)                                         # a point against zero-area boxes: 0/0
            a[1] = (20., 4., 8., 12.)                                       # inverted in x: negative area, not clamped
            a[2] = (20., 12., 8., 4.)                                       # inverted in both: positive area, no intersection
        b[0] = (3., 4., 3., 9.)
        got = _iou(a, b)
        ref, _ = DR.box_iou_ref(a, b)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), (na, nb)       # zero-area pairs: NaN at the same places
        ok = ~np.isnan(ref)
        # bit for bit, the sign of a zero included: an inverted box has no intersection (the sides are clamped) and a negative
        # area (they are not), so its IoU is 0 / negative = -0 wherever the union is negative
        assert np.array_equal(got.view(np.int32)[ok], ref.view(np.int32)[ok]), (na, nb)
        nans += int(np.isnan(ref).sum())
        if na > 1:
            assert np.signbit(ref[1][ok[1]]).any() and not np.signbit(ref[2][ok[2]]).any()
        # float boxes: no inverted ones, sides >= 1
        xy = rng.uniform(0, 300, (na + nb, 2))
        wh = rng.uniform(1, 200, (na + nb, 2))
        fb = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        fa, fbb = fb[:na].copy(), fb[na:].copy()
        fbb[0] = fa[0]                                                      # IoU 1
        got = _iou(fa, fbb).astype(np.float64)
        ref, bound = DR.box_iou_ref(fa, fbb)
        assert ref[0, 0] == 1.0
        ratio = np.abs(got - ref) / bound
        worst = max(worst, float(ratio.max()))
        assert ratio.max() <= 1.0, (na, nb, float(ratio.max()))
    assert nans >= 4
    print(f"box_iou: worst error / bound on float boxes = {worst:.4f}")
    assert worst < 1.0
