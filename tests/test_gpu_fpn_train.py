"""GPU: the adjoint kernels of ``csrc/seam_fpn_train.hip`` -- RoIAlign backward, the RPN window scatter, the top-down merge
backward, the LastLevelMaxPool backward -- and the chunked weight gradient, against the float64 scatter references of
``fpn_train_refs.py`` (tied to torch autograd of the oracle in ``test_fpn_train_references.py``).

Bounds are derived, not measured.  Every term of an output element is weight * gradient with a weight >= 0, so an fp32
evaluation of the same terms in any order stays within (T + c) * 2^-24 * A of the float64 sum, A = the sum of the absolute
terms, T = their number.  RoIAlign: c = 8 covers forming the two table entries of a term (<= n_y - 1 and n_x - 1 additions,
with n_y * n_x <= T), their product, the term's multiply-add and the final / sr^2.  Scatter and merge: c = 2.
The sample positions are fp32 on both sides, in torchvision's operation order (no fused multiply-add).

Adjoint identity <fwd(F), G> == <F, bwd(G)>: both sides run on the device in fp32, the two dot products are taken in float64 on
the host.  Each side is a sum of the same terms weight * F * G, so each is within sum_e (T_e + 8) 2^-24 A_e |F_e| of the exact
value and the two differ by at most twice that.  No reference enters: this catches a level or index disagreement between the
two kernels.  (The forward kernel forms `y1 + ph * bh` with a fused multiply-add, the backward does not: a sample of the forward
may sit an ulp of a coordinate away, which moves single terms by ~2^-20 of their size with either sign -- far inside the summed
bound; the figures are printed.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

import fpn_train_refs as FR
from oracle import detection as OD

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = FR.U
NAN = float("nan")


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def st():
    return torch.cuda.current_stream().cuda_stream


def randn(seed, *shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------ RoIAlign adjoint
def raw_roi_bwd(dout, rois, levels, hws, scales, n, p, sr, outs, c=None, k=None, ws="own"):
    from seam_match_rcnn_amd import _native
    lib = _native.lib()
    k = rois.shape[0] if k is None else k
    c = dout.shape[3] if c is None else c
    if isinstance(ws, str):
        ws = torch.empty((max(int(lib.seam_roi_align_bwd_workspace_bytes(n, max(k, 0))), 16),), dtype=torch.uint8, device=DEV)
    hw = (C.c_int * 8)(*[d for s in hws for d in s])
    return lib.seam_roi_align_bwd_f32(P(dout), P(rois), P(levels), hw, c, *scales, FR.K_MIN, n, k, p, sr,
                                      P(outs[0]), P(outs[1]), P(outs[2]), P(outs[3]), P(ws), st())


def poisoned(n, c, hws=FR.ROI_HWS):
    return [torch.full((n, h, w, c), NAN, device=DEV) for h, w in hws]


@pytest.mark.parametrize("p,sr", [(7, 2), (14, 2), (5, 1), (5, 3)])
@pytest.mark.parametrize("c", [64, 8])
def test_roi_align_bwd_vs_float64_scatter(c, p, sr):
    from seam_match_rcnn_amd import ops
    for image1, explicit in (("some", False), ("some", True), ("none", False)):
        rois = FR.roi_set(image1)
        k = rois.shape[0]
        mapped = OD.map_levels(rois[:, 1:], 2, 5)
        levels = FR.explicit_levels(k, rois[:, 0] == 1) if explicit else mapped
        dout = randn(100 * p + 10 * sr + c, k, p, p, c)
        ref = FR.roi_align_bwd_scatter(dout, rois, levels, FR.ROI_HWS, FR.ROI_SCALES, sr, 2)
        got = ops.roi_align_bwd(dout.to(DEV), rois.to(DEV), FR.ROI_HWS, 2, FR.ROI_SCALES, sr, FR.K_MIN,
                                levels.to(DEV) if explicit else None)
        # launched twice into NaN-poisoned maps: the same bits, nothing left unwritten
        again = poisoned(2, c)
        assert raw_roi_bwd(dout.to(DEV), rois.to(DEV), levels.to(DEV) if explicit else None, FR.ROI_HWS, FR.ROI_SCALES, 2, p, sr, again) == 0
        for l in range(4):
            assert not bool(torch.isnan(got[l]).any()) and torch.equal(got[l], again[l]), (image1, explicit, l)
            worst = FR.within(got[l], ref[l], 8)
            print(f"C{c} P{p} sr{sr} image1={image1} explicit={explicit} level {l}: worst error / bound {worst:.3f}")
        assert bool((got[3][1] == 0).all())                                   # image 1 owns no ROI of level 3
        if image1 == "none":
            assert all(bool((g[1] == 0).all()) for g in got)                  # ... and here no ROI at all


def test_roi_align_bwd_no_rois_and_bad_image_index():
    from seam_match_rcnn_amd import ops
    got = ops.roi_align_bwd(torch.zeros((0, 7, 7, 8), device=DEV), torch.zeros((0, 5), device=DEV), FR.ROI_HWS, 2, FR.ROI_SCALES)
    assert [tuple(g.shape) for g in got] == [(2, h, w, 8) for h, w in FR.ROI_HWS]
    outs = poisoned(2, 8)
    assert raw_roi_bwd(None, None, None, FR.ROI_HWS, FR.ROI_SCALES, 2, 7, 2, outs, c=8, k=0) == 0
    assert all(bool((g == 0).all()) for g in got) and all(bool((o == 0).all()) for o in outs)
    # image index outside [0, N), negative, NaN, infinite: nothing arrives, nothing outside the maps is touched
    rois = FR.roi_set("some")[:12].clone()
    good = rois.clone()
    rois[1, 0], rois[2, 0], rois[3, 0], rois[4, 0], rois[8, 0] = 2.0, -1.0, NAN, float("inf"), 7.0
    rois[5, 1:] = NAN                                                          # a box of NaNs
    keep = torch.tensor([i not in (1, 2, 3, 4, 5, 8) for i in range(12)])
    dout = randn(5, 12, 7, 7, 8)
    lv = OD.map_levels(good[:, 1:], 2, 5).to(torch.int32)
    got = ops.roi_align_bwd(dout.to(DEV), rois.to(DEV), FR.ROI_HWS, 2, FR.ROI_SCALES, 2, FR.K_MIN, lv.to(DEV))
    ref = FR.roi_align_bwd_scatter(dout[keep], good[keep], lv[keep], FR.ROI_HWS, FR.ROI_SCALES, 2, 2)
    for l in range(4):
        FR.within(got[l], ref[l], 8)


def test_roi_align_adjoint_identity():
    from seam_match_rcnn_amd import ops
    rois = FR.roi_set("some")
    k = rois.shape[0]
    lv = OD.map_levels(rois[:, 1:], 2, 5)
    for c, p, sr in ((64, 7, 2), (64, 14, 2), (8, 5, 3), (8, 5, 1)):
        feats = [randn(7 + l, 2, h, w, c) for l, (h, w) in enumerate(FR.ROI_HWS)]
        g = randn(17, k, p, p, c)
        fwd = ops.roi_align([f.to(DEV) for f in feats], rois.to(DEV), FR.ROI_SCALES, p, sr, FR.K_MIN)
        bwd = ops.roi_align_bwd(g.to(DEV), rois.to(DEV), FR.ROI_HWS, 2, FR.ROI_SCALES, sr, FR.K_MIN)
        lhs = float((fwd.cpu().double() * g.double()).sum())
        rhs = sum(float((b.cpu().double() * f.double()).sum()) for b, f in zip(bwd, feats))
        ref = FR.roi_align_bwd_scatter(g, rois, lv, FR.ROI_HWS, FR.ROI_SCALES, sr, 2)
        bound_b = sum(float(((t + 8) * U * a * f.double().abs()).sum()) for (s, a, t), f in zip(ref, feats))
        print(f"C{c} P{p} sr{sr}: <fwd(F),G> {lhs!r} <F,bwd(G)> {rhs!r} diff {abs(lhs - rhs):.3e} bound 2 x {bound_b:.3e}")
        assert abs(lhs - rhs) <= 2 * bound_b


@pytest.mark.parametrize("bad", ["c6", "c4100", "p0", "p33", "sr0", "n0", "k-1", "null_dout", "null_map", "null_ws", "h0"])
def test_roi_align_bwd_refusals_leave_the_maps_alone(bad):
    rois = FR.roi_set("some").to(DEV)
    k = rois.shape[0]
    dout = randn(1, k, 7, 7, 8).to(DEV)
    outs = [torch.full((2, h, w, 8), 3.25, device=DEV) for h, w in FR.ROI_HWS]
    kw = dict(dout=dout, rois=rois, levels=None, hws=FR.ROI_HWS, scales=FR.ROI_SCALES, n=2, p=7, sr=2, outs=list(outs))
    kw["ws"] = None if bad == "null_ws" else torch.empty((1 << 16,), dtype=torch.uint8, device=DEV)
    if bad == "c6": kw["c"] = 6
    if bad == "c4100": kw["c"] = 4100
    if bad == "p0": kw["p"] = 0
    if bad == "p33": kw["p"] = 33
    if bad == "sr0": kw["sr"] = 0
    if bad == "n0": kw["n"] = 0
    if bad == "k-1": kw["k"] = -1
    if bad == "null_dout": kw["dout"], kw["c"] = None, 8
    if bad == "null_map": kw["outs"][2] = None
    if bad == "h0": kw["hws"] = [(20, 24), (0, 12), (5, 6), (3, 3)]
    rc = raw_roi_bwd(**kw)
    torch.cuda.synchronize()
    assert rc != 0
    assert all(bool((o == 3.25).all()) for o in outs)


def test_roi_align_bwd_refuses_a_map_of_two_gib():
    outs = [torch.full((1, 2, 2, 8), 3.25, device=DEV) for _ in range(4)]          # never written: the call is refused
    rois = torch.zeros((1, 5), device=DEV)
    dout = torch.zeros((1, 7, 7, 4096), device=DEV)
    rc = raw_roi_bwd(dout, rois, None, [(400, 400), (10, 12), (5, 6), (3, 3)], FR.ROI_SCALES, 1, 7, 2, outs)
    torch.cuda.synchronize()
    assert rc != 0 and all(bool((o == 3.25).all()) for o in outs)


# ------------------------------------------------------------------------------ RPN window scatter
def raw_scatter(dp, rows, hws, n, outs, m=None, c=None, l=None):
    from seam_match_rcnn_amd import _native
    l = len(hws) if l is None else l
    maps = (C.c_void_p * len(hws))(*[None if o is None else o.data_ptr() for o in outs])
    hw = (C.c_int * (2 * len(hws)))(*[d for s in hws for d in s])
    return _native.lib().seam_rpn_scatter_patches_f32(P(dp), P(rows), dp.shape[0] if m is None else m, n, l,
                                                      dp.shape[3] if c is None else c, maps, hw, st())


@pytest.mark.parametrize("c", [8, 256])
def test_rpn_scatter_patches(c):
    from seam_match_rcnn_amd import ops
    rows = FR.scatter_rows()
    dp = randn(c, 37, 3, 3, c)
    ref = FR.scatter_patches_ref(dp, rows, FR.SCATTER_HWS, 2)
    got = ops.rpn_scatter_patches(dp.to(DEV), rows.to(DEV), FR.SCATTER_HWS, 2)
    again = [torch.full((2, h, w, c), NAN, device=DEV) for h, w in FR.SCATTER_HWS]
    assert raw_scatter(dp.to(DEV), rows.to(DEV), FR.SCATTER_HWS, 2, again) == 0
    for l in range(3):
        assert not bool(torch.isnan(got[l]).any()) and torch.equal(got[l], again[l])
        print(f"C{c} level {l}: worst error / bound {FR.within(got[l], ref[l], 2):.3f}")
    assert float(ref[0][2].max()) >= 6 and float(ref[2][2].min()) >= 1               # overlapping windows are the normal case
    # adjoint identity with the gather
    feats = [randn(40 + l, 2, h, w, c) for l, (h, w) in enumerate(FR.SCATTER_HWS)]
    patches = ops.rpn_gather_patches([f.to(DEV) for f in feats], rows.to(DEV))
    assert torch.equal(patches.cpu().double(), FR.gather_patches_ref(feats, rows))   # a gather is exact
    lhs = float((patches.cpu().double() * dp.double()).sum())
    rhs = sum(float((g.cpu().double() * f.double()).sum()) for g, f in zip(got, feats))
    bound = sum(float(((t + 2) * U * a * f.double().abs()).sum()) for (s, a, t), f in zip(ref, feats))
    print(f"C{c}: <gather(F),G> {lhs!r} <F,scatter(G)> {rhs!r} bound {bound:.3e}")
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("bad", ["m0", "l0", "l9", "c6", "n0", "null_rows", "null_map", "w0"])
def test_rpn_scatter_refusals_leave_the_maps_alone(bad):
    rows, dp = FR.scatter_rows().to(DEV), randn(2, 37, 3, 3, 8).to(DEV)
    outs = [torch.full((2, h, w, 8), 3.25, device=DEV) for h, w in FR.SCATTER_HWS]
    args = dict(dp=dp, rows=rows, hws=list(FR.SCATTER_HWS), n=2, outs=list(outs))
    if bad == "m0": args["m"] = 0
    if bad == "l0": args["l"] = 0
    if bad == "l9": args["l"] = 9
    if bad == "c6": args["c"] = 6
    if bad == "n0": args["n"] = 0
    if bad == "null_rows": args["rows"] = None
    if bad == "null_map": args["outs"][1] = None
    if bad == "w0": args["hws"][2] = (2, 0)
    rc = raw_scatter(**args)
    torch.cuda.synchronize()
    assert rc != 0 and all(bool((o == 3.25).all()) for o in outs)


# ------------------------------------------------------------------------------ top-down merge and pool adjoints
@pytest.mark.parametrize("fine,coarse", [((25, 21), (13, 11)), ((13, 11), (7, 6)), ((8, 10), (4, 5))])
@pytest.mark.parametrize("with_base", [False, True])
def test_upsample_add_bwd(fine, coarse, with_base):
    from seam_match_rcnn_amd import _native, ops
    c = 12
    dl = randn(1, 2, fine[0], fine[1], c)
    base = randn(2, 2, coarse[0], coarse[1], c) if with_base else None
    ref = FR.upsample_add_bwd_ref(dl, coarse, base)
    got = ops.upsample_add_bwd(dl.to(DEV), coarse, None if base is None else base.to(DEV))
    again = torch.full((2, coarse[0], coarse[1], c), NAN, device=DEV)
    assert _native.lib().seam_upsample_add_bwd_f32(P(dl.to(DEV)), P(None if base is None else base.to(DEV)), P(again), 2, fine[0], fine[1],
                                                   coarse[0], coarse[1], c, st()) == 0
    assert not bool(torch.isnan(got).any()) and torch.equal(got, again)
    print(f"{fine}->{coarse} base={with_base}: worst error / bound {FR.within(got, ref, 2):.3f}")
    # adjoint identity with the forward merge: <lat + up(top), G> - <lat, G> == <top, bwd(G)>
    top = randn(3, 2, coarse[0], coarse[1], c)
    up = ops.upsample_add_(torch.zeros((2, fine[0], fine[1], c), device=DEV), top.to(DEV))
    idx_y, idx_x = FR.nearest_src(fine[0], coarse[0]), FR.nearest_src(fine[1], coarse[1])
    assert torch.equal(up.cpu(), top[:, idx_y][:, :, idx_x])                       # one index rule on both sides
    plain = FR.upsample_add_bwd_ref(dl, coarse)
    bwd = got.cpu().double() - (base.double() if with_base else 0)
    lhs, rhs = float((up.cpu().double() * dl.double()).sum()), float((bwd * top.double()).sum())
    bound = float(((ref[2] + 2) * U * ref[1] * top.double().abs()).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert float(plain[2].min()) >= 1 and float(plain[2].max()) <= 4


def test_upsample_and_subsample_refusals():
    from seam_match_rcnn_amd import _native
    lib = _native.lib()
    dl, out = randn(1, 2, 8, 10, 12).to(DEV), torch.full((2, 4, 5, 12), 3.25, device=DEV)
    assert lib.seam_upsample_add_bwd_f32(P(dl), None, P(out), 2, 8, 10, 4, 5, 6, st()) != 0
    assert lib.seam_upsample_add_bwd_f32(P(dl), None, P(out), 0, 8, 10, 4, 5, 12, st()) != 0
    assert lib.seam_upsample_add_bwd_f32(None, None, P(out), 2, 8, 10, 4, 5, 12, st()) != 0
    assert lib.seam_upsample_add_bwd_f32(P(dl), None, P(out), 2, 8, 10, 0, 5, 12, st()) != 0
    d = torch.full((2, 7, 6, 12), 3.25, device=DEV)
    dp = randn(2, 2, 4, 3, 12).to(DEV)
    assert lib.seam_subsample_add_bwd_f32(P(d), P(dp), 2, 7, 6, 3, 3, 12, st()) != 0     # wrong pooled extent
    assert lib.seam_subsample_add_bwd_f32(P(d), P(dp), 2, 7, 6, 4, 3, 6, st()) != 0
    assert lib.seam_subsample_add_bwd_f32(P(d), None, 2, 7, 6, 4, 3, 12, st()) != 0
    torch.cuda.synchronize()
    assert bool((out == 3.25).all()) and bool((d == 3.25).all())


def test_subsample_add_bwd_is_exact():
    from seam_match_rcnn_amd import ops
    d, dp = randn(1, 2, 7, 6, 12), randn(2, 2, 4, 3, 12)
    want = d.clone()
    want[:, ::2, ::2] += dp
    a = ops.subsample_add_bwd(d.to(DEV), dp.to(DEV))
    b = ops.subsample_add_bwd(d.to(DEV), dp.to(DEV))
    assert torch.equal(a.cpu(), want) and torch.equal(a, b)
    # it is the adjoint of LastLevelMaxPool: max_pool2d(k=1, s=2) reads exactly those pixels
    assert tuple(ops.maxpool2d(d.to(DEV), 1, 2, 0).shape) == tuple(dp.shape)
    assert torch.equal(ops.maxpool2d(d.to(DEV), 1, 2, 0).cpu(), d[:, ::2, ::2])


# ------------------------------------------------------------------------------ chunked weight gradient
def test_chunked_conv_wgrad_splits_and_is_reproducible():
    from seam_match_rcnn_amd import ops, ops_train
    x, dy = randn(1, 5, 9, 11, 32).to(DEV), randn(2, 5, 9, 11, 64).to(DEV)
    whole = ops.conv_wgrad(x, dy, 3, 3, 1, 1)
    assert torch.equal(ops.conv_wgrad_chunked(x, dy, 3, 3, 1, 1), whole)           # within the limit: the plain call
    calls, plain = [], ops.conv_wgrad
    old = ops_train.WGRAD_MAX_OPERAND_BYTES
    try:
        ops_train.WGRAD_MAX_OPERAND_BYTES = 2 * dy[0].numel() * 4 + 100                  # two images per chunk: 2 + 2 + 1
        ops_train.conv_wgrad = lambda a, b, *r: (calls.append(a.shape[0]), plain(a, b, *r))[1]
        one = ops.conv_wgrad_chunked(x, dy, 3, 3, 1, 1)
        two = ops.conv_wgrad_chunked(x, dy, 3, 3, 1, 1)
        ops_train.WGRAD_MAX_OPERAND_BYTES = dy[0].numel() * 4 - 4
        with pytest.raises(ValueError):
            ops.conv_wgrad_chunked(x, dy, 3, 3, 1, 1)
    finally:
        ops_train.WGRAD_MAX_OPERAND_BYTES, ops_train.conv_wgrad = old, plain
    assert calls == [2, 2, 1, 2, 2, 1]
    assert torch.equal(one, two)
    FR.wgrad_close(one, whole)
