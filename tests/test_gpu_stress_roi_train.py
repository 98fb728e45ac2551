"""Random-shape stress of the RoI-heads training kernels (``csrc/seam_roi_train.hip``) through the C ABI, in the style of
``test_gpu_stress.py``: every output is POISONED and followed by a 1 MiB guard; each seeded case runs twice and the two
results must be bit-identical (fixed-order reductions, no float atomics); each result is compared with the restatement
of ``roi_train_refs.py`` (exact for the sampler's indices, labels and matches; the bounds of ``test_gpu_roi_train.py``
for the rest).  Each launcher's refusals must leave every output untouched."""
import numpy as np
import pytest
import torch

import roi_train_refs as RR
from stress_kit import Buf, P, st

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NCASE = 40


def _lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def _sample(lib, cand, ncand, keys, gt, gl, ngt, B, pm):
    n, p = cand.shape[:2]
    outs = [Buf((n, B), torch.int64), Buf((n, B), torch.int64), Buf((n, B), torch.int64), Buf((n, B, 4), torch.float32),
            Buf((n, B, 4), torch.float32), Buf((n, 2), torch.int32)]
    rc = lib.seam_roi_sample_f32(P(cand), P(ncand), P(keys), P(gt), P(gl), P(ngt), n, p, gt.shape[1], B, pm,
                                 10.0, 10.0, 5.0, 5.0, *[P(o.t) for o in outs], st())
    torch.cuda.synchronize()
    return rc, outs


def test_stress_roi_sample():
    lib = _lib()
    rng = np.random.RandomState(0)
    for case in range(NCASE):
        n = int(rng.randint(1, 5))
        G = int(rng.randint(1, 12))
        Pn = int(rng.choice([1, 7, 64, 1023, 1025, 4097, 16384]))
        B = int(rng.choice([1, 16, 512, 600]))
        pm = int(rng.randint(0, B + 1))
        H, W = 400.0, 600.0
        ngt = np.minimum(rng.randint(1, G + 1, n), Pn)
        ncand = np.array([rng.randint(ngt[i], Pn + 1) for i in range(n)])
        cand = np.zeros((n, Pn, 4), np.float32)
        gt = np.zeros((n, G, 4), np.float32)
        for i in range(n):
            g = np.sort(rng.uniform(0, [W, H, W, H], (ngt[i], 4)).reshape(ngt[i], 2, 2), axis=1).reshape(ngt[i], 4)[:, [0, 2, 1, 3]]
            g[:, 2:] = np.maximum(g[:, 2:], g[:, :2] + 2)
            gt[i, :ngt[i]] = g
            k = ncand[i] - ngt[i]
            src = g[rng.randint(0, ngt[i], k)]
            pr = src + rng.normal(0, 20, (k, 4))
            pr[:, 2:] = np.maximum(pr[:, 2:], pr[:, :2] + 1)
            cand[i, :k] = pr
            cand[i, k:ncand[i]] = g
        keys = rng.rand(n, Pn).astype(np.float32)
        if case % 3 == 0:
            keys = np.round(keys * 8) / 8                         # many exact ties
        gl = rng.randint(0, 5, (n, G)).astype(np.int64)
        args = [torch.from_numpy(a).to(DEV) for a in (cand, ncand.astype(np.int32), keys, gt, gl, ngt.astype(np.int32))]
        rc, o1 = _sample(lib, *args, B, pm)
        rc2, o2 = _sample(lib, *args, B, pm)
        desc = (n, G, Pn, B, pm)
        assert rc == 0 and rc2 == 0, desc
        assert all(b.guard_ok() for b in o1 + o2), desc
        assert all(torch.equal(a.t.view(torch.int32) if a.t.dtype != torch.int64 else a.t,
                               b.t.view(torch.int32) if b.t.dtype != torch.int64 else b.t) for a, b in zip(o1, o2)), desc
        idx, lab, mat, bx, tg, cnt = [b.t.cpu() for b in o1]
        for i in range(n):
            k = ncand[i] - ngt[i]
            ref = RR.select_training_samples([torch.from_numpy(cand[i, :k])], [torch.from_numpy(gt[i, :ngt[i]])],
                                             [torch.from_numpy(gl[i, :ngt[i]])], [torch.from_numpy(keys[i])], B, pm)[0]
            c = int(cnt[i, 0])
            assert c == len(ref["idx"]), desc
            assert torch.equal(idx[i, :c], ref["idx"]) and torch.equal(lab[i, :c], ref["labels"]), desc
            assert torch.equal(mat[i, :c], ref["matched"]) and torch.equal(bx[i, :c], ref["boxes"]), desc
            fin = torch.isfinite(ref["targets"])
            assert torch.equal(fin, torch.isfinite(tg[i, :c])), desc
            d = (tg[i, :c][fin].double() - ref["targets"][fin].double()).abs()
            assert bool((d <= 4 * 2.0 ** -23 * ref["targets"][fin].double().abs() + 1e-30).all()), desc
            assert (idx[i, c:] == -1).all() and (lab[i, c:] == -1).all() and (tg[i, c:] == 0).all(), desc
    # refusals leave every output untouched
    z = torch.zeros((1, 4, 4), device=DEV)
    one = torch.ones(1, dtype=torch.int32, device=DEV)
    for p_, g_, b_, pm_ in ((0, 1, 4, 1), (16385, 1, 4, 1), (4, 0, 4, 1), (4, 1, 0, 0), (4, 1, 4, 5), (4, 1, 4, -1)):
        outs = [Buf((1, 4), torch.int64), Buf((1, 4), torch.int64), Buf((1, 4), torch.int64), Buf((1, 4, 4), torch.float32),
                Buf((1, 4, 4), torch.float32), Buf((1, 2), torch.int32)]
        rc = lib.seam_roi_sample_f32(P(z), P(one), P(z), P(z), P(z), P(one), 1, p_, g_, b_, pm_, 10.0, 10.0, 5.0, 5.0,
                                     *[P(o.t) for o in outs], st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in outs), (p_, g_, b_, pm_)


def test_stress_fastrcnn_loss():
    lib = _lib()
    rng = np.random.RandomState(1)
    for case in range(NCASE):
        R = int(rng.choice([1, 2, 63, 64, 255, 256, 257, 1000, 4096, 5000]))
        ncls = int(rng.choice([1, 2, 14, 91]))
        cl = torch.from_numpy(rng.normal(0, 4, (R, ncls)).astype(np.float32))
        br = torch.from_numpy(rng.normal(0, 0.2, (R, 4 * ncls)).astype(np.float32))
        lab = torch.from_numpy(rng.randint(0, ncls, R).astype(np.int64))
        tg = torch.from_numpy(rng.normal(0, 0.2, (R, 4)).astype(np.float32))
        dev = [t.to(DEV) for t in (cl, br, lab, tg)]
        res = []
        for _ in range(2):
            outs = [Buf((2,), torch.float32), Buf((R, ncls), torch.float32), Buf((R, 4 * ncls), torch.float32)]
            rc = lib.seam_fastrcnn_loss_fwd_bwd_f32(*[P(t) for t in dev], R, ncls, *[P(o.t) for o in outs], st())
            torch.cuda.synchronize()
            assert rc == 0 and all(o.guard_ok() for o in outs), (R, ncls)
            res.append([o.t.cpu() for o in outs])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res)), (R, ncls)
        loss, dcl, dbr = res[0]
        c64, b64 = cl.double().requires_grad_(True), br.double().requires_grad_(True)
        l1, l2 = RR.fastrcnn_loss(c64, b64, lab, tg.double())
        gc, gb = torch.autograd.grad(l1 + l2, (c64, b64))
        assert abs(float(loss[0]) - float(l1.detach())) <= 4 * R * 2 ** -24 * float(l1) + 1e-7, (R, ncls)
        assert abs(float(loss[1]) - float(l2.detach())) <= 4 * R * 2 ** -24 * float(l2) + 1e-7, (R, ncls)
        assert float((dcl.double() - gc).abs().max()) <= 8 * 2 ** -23 * float(gc.abs().max()) + 2 ** -24 / R, (R, ncls)
        assert float((dbr.double() - gb).abs().max()) <= 8 * 2 ** -23 * max(float(gb.abs().max()), 1.0 / R), (R, ncls)
    z = torch.zeros(16, device=DEV)
    for r_, n_ in ((0, 3), (3, 0), (-1, 3)):
        outs = [Buf((2,), torch.float32), Buf((4,), torch.float32), Buf((4,), torch.float32)]
        rc = lib.seam_fastrcnn_loss_fwd_bwd_f32(P(z), P(z), P(z), P(z), r_, n_, *[P(o.t) for o in outs], st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() for o in outs)


def test_stress_mask_loss():
    lib = _lib()
    rng = np.random.RandomState(2)
    for case in range(NCASE // 2):
        Pn = int(rng.choice([1, 2, 5, 17]))
        ncls = int(rng.choice([1, 2, 14]))
        H, W = int(rng.randint(8, 600)), int(rng.randint(8, 900))
        ng = int(rng.randint(1, 4))
        masks = (rng.rand(ng, H, W) < 0.5).astype(np.uint8)
        xy = rng.uniform(-20, [W, H], (Pn, 2))
        wh = rng.uniform(0.2, 1.2 * max(H, W), (Pn, 2))
        rois = np.concatenate([xy, xy + wh], 1).astype(np.float32)
        matched = rng.randint(0, ng, Pn)
        labels = rng.randint(0, ncls, Pn).astype(np.int64)
        logits = rng.normal(0, 3, (Pn, 14, 14, 4 * ncls)).astype(np.float32)
        dev = [torch.from_numpy(a).to(DEV) for a in (logits, labels, rois, masks.reshape(-1),
                                                       (matched * H * W).astype(np.int64), np.tile([[H, W]], (Pn, 1)).astype(np.int32))]
        res = []
        for _ in range(2):
            outs = [Buf((), torch.float32), Buf((Pn, 14, 14, 4 * ncls), torch.float32), Buf((Pn,), torch.float32)]
            rc = lib.seam_mask_loss_fwd_bwd_f32(*[P(t) for t in dev], Pn, ncls, *[P(o.t) for o in outs], st())
            torch.cuda.synchronize()
            assert rc == 0 and all(o.guard_ok() for o in outs), (Pn, ncls, H, W)
            res.append([o.t.cpu() for o in outs])
        assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res)), (Pn, ncls, H, W)
        loss, dl, _ = res[0]
        t28 = torch.from_numpy(RR.project_masks(masks, rois, matched))
        l64 = torch.from_numpy(logits).double().requires_grad_(True)
        ref = RR.maskrcnn_loss(l64, torch.from_numpy(labels), t28)
        (gref,) = torch.autograd.grad(ref, l64)
        n = Pn * 784
        # targets: within RR.target_error of the float64 ones
        terr = RR.target_error(rois, H, W)
        assert abs(float(loss) - float(ref)) <= 8 * n * 2 ** -24 * float(ref) + terr * float(l64.abs().mean()) + 1e-6, \
            (Pn, ncls, H, W)
        assert float((dl.double() - gref).abs().max()) <= (terr + 16 * 2 ** -23) / n, (Pn, ncls, H, W)
    z = torch.zeros(64, device=DEV)
    for p_, n_ in ((0, 2), (21400, 2), (2, 0)):
        outs = [Buf((), torch.float32), Buf((4,), torch.float32), Buf((4,), torch.float32)]
        rc = lib.seam_mask_loss_fwd_bwd_f32(P(z), P(z), P(z), P(z), P(z), P(z), p_, n_, *[P(o.t) for o in outs], st())
        torch.cuda.synchronize()
        assert rc != 0 and all(o.untouched() for o in outs)
