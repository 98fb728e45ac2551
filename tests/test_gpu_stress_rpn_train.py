"""Random-shape stress of the RPN training kernels (``csrc/seam_rpn_train.hip``) through the C ABI, in the manner of
``test_gpu_stress_roi_train.py``: every output is POISONED and followed by a 1 MiB guard; each seeded case runs twice and the
two results must be bit-identical; each result is compared with the restatement of ``rpn_train_refs.py`` (exact for labels,
matches, sampled anchors and counts; the bounds of ``test_gpu_rpn_train.py`` for the rest).  The caps are visited from both
sides (A = 1 and A = 2^20, G = 128, M = 1); a refused call must leave every output untouched.  Nothing here provokes a fault:
out-of-range arguments are refused on the host before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

import rpn_train_refs as PR
from stress_kit import Buf, P, st

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MAX_A, MAX_G = 1 << 20, 128


def _lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def _boxes(rng, n, span):
    xy = rng.uniform(0, span, (n, 2))
    wh = rng.uniform(4, span / 2, (n, 2))
    return np.concatenate([xy, xy + wh], 1).astype(np.float32)


def _match(lib, anchors, gt, ngt, fg=0.7, bg=0.3):
    n, g = gt.shape[:2]
    a = anchors.shape[0]
    outs = [Buf((n, a), torch.int8), Buf((n, a), torch.int32)]
    ws = Buf((max(int(lib.seam_rpn_match_workspace_floats(n, a, g)), 1),), torch.float32)
    rc = lib.seam_rpn_match_f32(P(anchors), P(gt), P(ngt), n, a, g, fg, bg, P(outs[0].t), P(outs[1].t), P(ws.t), st())
    torch.cuda.synchronize()
    return rc, outs, ws


def _sample(lib, labels, matched, keys, anchors, gt, B, pm):
    n, a = labels.shape
    outs = [Buf((n, B), torch.int64), Buf((n, B), torch.int64), Buf((n, B), torch.int64), Buf((n, B, 4), torch.float32),
            Buf((n, 2), torch.int32)]
    ws = Buf((max(int(lib.seam_rpn_sample_workspace_bytes(n, B)), 4),), torch.uint8)
    rc = lib.seam_rpn_sample_f32(P(labels), P(matched), P(keys), P(anchors), P(gt), n, a, gt.shape[1], B, pm,
                                 *[P(o.t) for o in outs], P(ws.t), st())
    torch.cuda.synchronize()
    return rc, outs, ws


def test_stress_rpn_match_and_sample():
    lib = _lib()
    assert lib.seam_rpn_max_gt() == MAX_G
    rng = np.random.RandomState(0)
    shapes = [(1, 1, 1), (2, MAX_A, 3), (1, 5000, MAX_G), (3, 1023, 1), (2, 1025, 7), (1, 4097, 2)]
    for case in range(18):
        if case < len(shapes):
            n, A, G = shapes[case]
        else:
            n, A, G = int(rng.randint(1, 5)), int(rng.choice([2, 63, 256, 1024, 1025, 4095, 4096, 20000, 70001])), int(rng.randint(1, 20))
        B = int(rng.choice([1, 16, 256, 1000]))
        pm = int(rng.randint(0, B + 1))
        span = 600.0
        ngt = rng.randint(0, G + 1, n)
        ngt[0] = G                                             # the padded width is used by at least one image
        anchors = _boxes(rng, A, span)
        gt = np.zeros((n, G, 4), np.float32)
        for i in range(n):
            gt[i, :ngt[i]] = _boxes(rng, ngt[i], span)
            k = min(ngt[i], A, 4)
            if k:
                anchors[rng.choice(A, k, replace=False)] = gt[i, :k] if case % 2 else gt[i, :k] + np.float32(3.0)
        keys = rng.rand(n, A).astype(np.float32)
        if case % 3 == 0:
            keys = np.round(keys * 8) / 8                      # many exact ties
        d_anchors, d_gt, d_ngt, d_keys = [torch.from_numpy(x).to(DEV) for x in (anchors, gt, ngt.astype(np.int32), keys)]
        desc = (n, A, G, B, pm)
        rc, m1, w1 = _match(lib, d_anchors, d_gt, d_ngt)
        rc2, m2, w2 = _match(lib, d_anchors, d_gt, d_ngt)
        assert rc == 0 and rc2 == 0, desc
        assert all(b.guard_ok() for b in m1 + m2 + [w1, w2]), desc
        assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(m1, m2)), desc
        rc, s1, w1 = _sample(lib, m1[0].t, m1[1].t, d_keys, d_anchors, d_gt, B, pm)
        rc2, s2, w2 = _sample(lib, m1[0].t, m1[1].t, d_keys, d_anchors, d_gt, B, pm)
        assert rc == 0 and rc2 == 0, desc
        assert all(b.guard_ok() for b in s1 + s2 + [w1, w2]), desc
        assert all(torch.equal(a.bits(), b.bits()) for a, b in zip(s1, s2)), desc
        labels, matched = m1[0].t.cpu(), m1[1].t.cpu()
        idx, slab, smat, tg, cnt = [b.t.cpu() for b in s1]
        for i in range(n):
            r = PR.assign_and_sample(torch.from_numpy(anchors), torch.from_numpy(gt[i, :ngt[i]]), torch.from_numpy(keys[i]), B, pm)
            assert torch.equal(labels[i].to(torch.int64), r["labels_all"]), desc
            assert torch.equal(matched[i].to(torch.int64), r["matched_all"]), desc
            c = int(cnt[i, 0])
            assert c == len(r["idx"]) and int(cnt[i, 1]) == int((r["labels"] == 1).sum()), desc
            assert torch.equal(idx[i, :c], r["idx"]) and torch.equal(slab[i, :c], r["labels"]), desc
            assert torch.equal(smat[i, :c], r["matched"]), desc
            d = (tg[i, :c].double() - r["targets"].double()).abs()
            assert bool((d <= 4 * 2.0 ** -23 * r["targets"].double().abs() + 1e-30).all()), desc
            assert (idx[i, c:] == -1).all() and (slab[i, c:] == -1).all() and (tg[i, c:] == 0).all(), desc
    # refusals leave every output untouched
    z = torch.zeros((64,), device=DEV)
    one = torch.ones(4, dtype=torch.int32, device=DEV)
    for n_, a_, g_, fg_, bg_ in ((0, 4, 1, .7, .3), (1, 0, 1, .7, .3), (1, MAX_A + 1, 1, .7, .3), (1, 4, 0, .7, .3),
                                 (1, 4, MAX_G + 1, .7, .3), (1, 4, 1, .3, .7), (4097, 1, 1, .7, .3)):
        assert lib.seam_rpn_match_workspace_floats(n_, a_, g_) == 0 or bg_ > fg_
        outs = [Buf((4,), torch.int8), Buf((4,), torch.int32), Buf((16,), torch.float32)]
        rc = lib.seam_rpn_match_f32(P(z), P(z), P(one), n_, a_, g_, fg_, bg_, *[P(o.t) for o in outs], st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in outs), (n_, a_, g_)
    zl = torch.zeros((16,), dtype=torch.int8, device=DEV)
    for n_, a_, g_, b_, pm_ in ((0, 4, 1, 4, 2), (1, 0, 1, 4, 2), (1, MAX_A + 1, 1, 4, 2), (1, 4, 0, 4, 2), (1, 4, MAX_G + 1, 4, 2),
                                (1, 4, 1, 0, 0), (1, 4, 1, 1025, 2), (1, 4, 1, 4, 5), (1, 4, 1, 4, -1)):
        outs = [Buf((4,), torch.int64), Buf((4,), torch.int64), Buf((4,), torch.int64), Buf((4, 4), torch.float32),
                Buf((2,), torch.int32), Buf((4096,), torch.uint8)]
        rc = lib.seam_rpn_sample_f32(P(zl), P(one), P(z), P(z), P(z), n_, a_, g_, b_, pm_, *[P(o.t) for o in outs], st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in outs), (n_, a_, g_, b_, pm_)


def _gather(lib, maps, rows, n, c):
    m, l = rows.shape[0], len(maps)
    out = Buf((m, 3, 3, c), torch.float32)
    ptrs = (C.c_void_p * l)(*[f.data_ptr() for f in maps])
    hw = (C.c_int * (2 * l))(*[int(v) for f in maps for v in f.shape[1:3]])
    rc = lib.seam_rpn_gather_patches_f32(ptrs, hw, P(rows), m, n, l, c, P(out.t), st())
    torch.cuda.synchronize()
    return rc, out


def test_stress_rpn_gather_patches():
    lib = _lib()
    rng = np.random.RandomState(1)
    for case in range(20):
        n = int(rng.randint(1, 4))
        l = int(rng.randint(1, 6))
        c = int(rng.choice([4, 8, 64, 256, 260]))
        m = 1 if case == 0 else int(rng.choice([1, 2, 77, 600]))
        hws = [(int(rng.randint(1, 40)), int(rng.randint(1, 40))) for _ in range(l)]
        maps = [torch.from_numpy(rng.normal(0, 1, (n, h, w, c)).astype(np.float32)) for h, w in hws]
        lv = rng.randint(0, l, m)
        rows = np.stack([rng.randint(0, n, m), lv, [rng.randint(0, hws[v][0]) for v in lv], [rng.randint(0, hws[v][1]) for v in lv]], 1)
        if m > 4:                                              # corners, and rows out of range (zero patches, nothing read)
            rows[0, 2:] = 0
            rows[1, 2:] = (hws[lv[1]][0] - 1, hws[lv[1]][1] - 1)
            rows[2] = (n, 0, 0, 0)
            rows[3] = (0, l, 0, 0)
            rows[4] = (0, lv[4], -1, hws[lv[4]][1])
        d_maps = [f.to(DEV) for f in maps]
        d_rows = torch.from_numpy(rows.astype(np.int32)).to(DEV)
        rc, o1 = _gather(lib, d_maps, d_rows, n, c)
        rc2, o2 = _gather(lib, d_maps, d_rows, n, c)
        desc = (n, l, c, m)
        assert rc == 0 and rc2 == 0 and o1.guard_ok() and o2.guard_ok(), desc
        assert torch.equal(o1.bits(), o2.bits()), desc
        got = o1.t.cpu()
        for r, (i, v, y, x) in enumerate(rows):
            want = torch.zeros((3, 3, c))
            if 0 <= i < n and 0 <= v < l and 0 <= y < hws[v][0] and 0 <= x < hws[v][1]:
                padded = torch.nn.functional.pad(maps[v][i], (0, 0, 1, 1, 1, 1))
                want = padded[y:y + 3, x:x + 3]
            assert torch.equal(got[r], want), (desc, r)
    z = torch.zeros((64,), device=DEV)
    zi = torch.zeros((64,), dtype=torch.int32, device=DEV)
    ptrs = (C.c_void_p * 9)(*[z.data_ptr()] * 9)
    hw = (C.c_int * 18)(*[1] * 18)
    bad_hw = (C.c_int * 18)(*[0] * 18)
    for m_, n_, l_, c_, hw_ in ((0, 1, 1, 4, hw), ((1 << 20) + 1, 1, 1, 4, hw), (1, 0, 1, 4, hw), (1, 1, 0, 4, hw), (1, 1, 9, 4, hw),
                                (1, 1, 1, 0, hw), (1, 1, 1, 6, hw), (1, 1, 1, 4100, hw), (1, 1, 1, 4, bad_hw)):
        out = Buf((36,), torch.float32)
        rc = lib.seam_rpn_gather_patches_f32(ptrs, hw_, P(zi), m_, n_, l_, c_, P(out.t), st())
        torch.cuda.synchronize()
        assert rc != 0 and out.untouched() and out.guard_ok(), (m_, n_, l_, c_)


def test_stress_rpn_loss():
    lib = _lib()
    rng = np.random.RandomState(2)
    for case in range(30):
        M = 1 if case == 0 else int(rng.choice([1, 2, 63, 64, 255, 256, 257, 1000, 2048, 5000]))
        A = int(rng.choice([1, 3, 6]))
        hc = 5 * A + int(rng.choice([0, 1, 17]))
        gc = (5 * A + 31) // 32 * 32 if case % 2 else 5 * A
        head = rng.normal(0, 3, (M, hc)).astype(np.float32)
        head[:, A:] *= 0.1
        slot = rng.randint(0, A, M).astype(np.int32)
        lab = (rng.rand(M) < 0.4).astype(np.int64)
        tgt = rng.normal(0, 0.3, (M, 4)).astype(np.float32)
        dev = [torch.from_numpy(x).to(DEV) for x in (head, slot, lab, tgt)]
        res = []
        for _ in range(2):
            outs = [Buf((2,), torch.float32), Buf((M, gc), torch.float32)]
            rc = lib.seam_rpn_loss_fwd_bwd_f32(*[P(t) for t in dev], M, A, hc, gc, *[P(o.t) for o in outs], st())
            torch.cuda.synchronize()
            assert rc == 0 and all(o.guard_ok() for o in outs), (M, A, hc, gc)
            res.append([o.bits() for o in outs] + [o.t.cpu() for o in outs])
        assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]), (M, A, hc, gc)
        loss, grad = res[0][2], res[0][3]
        h64 = torch.from_numpy(head).double().requires_grad_(True)
        rows = torch.arange(M)
        sl = torch.from_numpy(slot).to(torch.int64)
        obj = h64[rows, sl]
        dl = h64[:, A:5 * A].reshape(M, A, 4)[rows, sl]
        lo, lb = PR.rpn_losses(obj, dl, torch.from_numpy(lab), torch.from_numpy(tgt).double())
        (gref,) = torch.autograd.grad(lo + lb, h64)
        lo, lb = lo.detach(), lb.detach()
        # a mean of M terms summed in fp32 (+ a few ulp of exp / log per term), as in test_gpu_stress_roi_train.py
        assert abs(float(loss[0]) - float(lo)) <= 4 * M * 2 ** -24 * float(lo) + 1e-7, (M, A)
        assert abs(float(loss[1]) - float(lb)) <= 4 * M * 2 ** -24 * float(lb) + 1e-7, (M, A)
        g = grad.double()
        assert float((g[:, :5 * A] - gref[:, :5 * A]).abs().max()) <= 8 * 2 ** -23 * max(float(gref.abs().max()), 1.0 / M), (M, A)
        assert float(g[:, 5 * A:].abs().max()) == 0.0 if gc > 5 * A else True
        assert int((g != 0).sum()) <= 5 * M
    # a slot or a label out of range: NaN losses, nothing out of bounds
    dev = [torch.zeros((2, 5), device=DEV), torch.tensor([0, 7], dtype=torch.int32, device=DEV),
           torch.tensor([1, 0], dtype=torch.int64, device=DEV), torch.zeros((2, 4), device=DEV)]
    outs = [Buf((2,), torch.float32), Buf((2, 32), torch.float32)]
    rc = lib.seam_rpn_loss_fwd_bwd_f32(*[P(t) for t in dev], 2, 1, 5, 32, *[P(o.t) for o in outs], st())
    torch.cuda.synchronize()
    assert rc == 0 and bool(torch.isnan(outs[0].t).all()) and all(o.guard_ok() for o in outs)
    z = torch.zeros(64, device=DEV)
    for m_, a_, hc_, gc_ in ((0, 1, 5, 5), ((1 << 20) + 1, 1, 5, 5), (1, 0, 5, 5), (1, 65, 325, 325), (1, 3, 14, 32), (1, 3, 15, 14),
                             (1, 3, 1025, 32), (1, 3, 15, 1025)):
        outs = [Buf((2,), torch.float32), Buf((32,), torch.float32)]
        rc = lib.seam_rpn_loss_fwd_bwd_f32(P(z), P(z), P(z), P(z), m_, a_, hc_, gc_, *[P(o.t) for o in outs], st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in outs), (m_, a_, hc_, gc_)
