"""CPU: the float64 references of the FPN-training adjoints (``fpn_train_refs.py``) against torch autograd of the oracle, the
binding of the new entry points, and the argument checks the wrappers make before anything reaches the device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_train_refs as FR
from oracle import detection as OD


@pytest.mark.parametrize("p,sr", [(7, 2), (5, 1), (5, 3)])
@pytest.mark.parametrize("explicit", [False, True])
def test_explicit_roi_scatter_equals_autograd_of_the_oracle(p, sr, explicit):
    rois = FR.roi_set("some")
    k = rois.shape[0]
    levels = FR.explicit_levels(k, rois[:, 0] == 1) if explicit else OD.map_levels(rois[:, 1:], 2, 5)
    dout = torch.randn((k, p, p, 3), generator=torch.Generator().manual_seed(p * 10 + sr), dtype=torch.float64)
    ref = FR.roi_align_bwd_scatter(dout, rois, levels, FR.ROI_HWS, FR.ROI_SCALES, sr, 2)
    auto = FR.roi_align_bwd_autograd(dout, rois, levels, FR.ROI_HWS, FR.ROI_SCALES, sr, 2)
    seen = 0
    for (s, a, t), g in zip(ref, auto):
        # the oracle rounds each tap's weight product to fp32 (one rounding per term); the scatter keeps it in float64
        assert bool(((s - g).abs() <= 2 * FR.U * a + 1e-300).all()), float(((s - g).abs() - 2 * FR.U * a).max())
        assert bool((s[t == 0] == 0).all()) and bool((a[t > 0] >= 0).all())
        seen += int((t > 0).any())
    assert seen == 4                                           # every level receives something
    if not explicit:
        assert set(levels.tolist()) == {0, 1, 2, 3}
        # the fp32 neighbours of 112 / 224 / 448 sit on both sides of their boundary
        b = levels[11:29].reshape(3, len(FR.BOUNDARY_STEPS))
        assert b[:, 0].tolist() == [0, 1, 2] and b[:, -1].tolist() == [1, 2, 3] and bool((b[:, 1:] >= b[:, :-1]).all())
    assert not bool(((rois[:, 0] == 1) & (torch.as_tensor(levels) == 3)).any())
    assert bool((ref[3][2][1] == 0).all())                     # image 1 owns nothing on level 3


def test_roi_set_contents():
    rois = FR.roi_set("some")
    assert 36 <= rois.shape[0] <= 44 and set(rois[:, 0].tolist()) == {0.0, 1.0}
    assert set(FR.roi_set("none")[:, 0].tolist()) == {0.0}
    assert torch.equal(rois[8], rois[9])
    lv = OD.map_levels(rois[:, 1:], 2, 5)
    ref = FR.roi_align_bwd_scatter(torch.ones((rois.shape[0], 2, 2, 1), dtype=torch.float64), rois, lv, FR.ROI_HWS, FR.ROI_SCALES, 2, 2)
    one = FR.roi_align_bwd_scatter(torch.ones((1, 2, 2, 1), dtype=torch.float64), rois[:1], lv[:1], FR.ROI_HWS, FR.ROI_SCALES, 2, 2)
    assert all(float(t.sum()) == 0 for _, _, t in one)         # the far-away ROI reaches nothing
    whole = FR.roi_align_bwd_scatter(torch.ones((1, 7, 7, 1), dtype=torch.float64), rois[7:8], lv[7:8], FR.ROI_HWS, FR.ROI_SCALES, 2, 2)
    assert bool((whole[0][2][0] > 0).all())                    # the whole-map ROI reaches every pixel of level 0
    assert float(ref[0][0].sum()) > 0


def test_scatter_and_merge_references_equal_autograd():
    rows = FR.scatter_rows()
    assert rows.shape == (37, 4)
    g = torch.Generator().manual_seed(3)
    feats = [torch.randn((2, h, w, 4), generator=g, dtype=torch.float64).requires_grad_(True) for h, w in FR.SCATTER_HWS]
    dp = torch.randn((37, 3, 3, 4), generator=g, dtype=torch.float64)
    # gather as differentiable torch ops: pad, then index
    loss = 0
    for m, (img, lvl, y, x) in enumerate(rows.tolist()):
        if lvl >= len(feats):
            continue
        pad = F.pad(feats[lvl][img], (0, 0, 1, 1, 1, 1))
        loss = loss + (pad[y:y + 3, x:x + 3] * dp[m]).sum()
    loss.backward()
    for f, (s, a, t) in zip(feats, FR.scatter_patches_ref(dp, rows, FR.SCATTER_HWS, 2)):
        assert torch.allclose(f.grad, s, rtol=0, atol=1e-12)
    assert torch.equal(FR.gather_patches_ref([f.detach() for f in feats], rows)[9], torch.zeros((3, 3, 4), dtype=torch.float64))
    for (h, w), (ht, wt) in (((25, 21), (13, 11)), ((13, 11), (7, 6)), ((8, 10), (4, 5))):
        top = torch.randn((2, 3, ht, wt), generator=g, dtype=torch.float64).requires_grad_(True)
        up = F.interpolate(top, size=(h, w), mode="nearest")
        dl = torch.randn((2, h, w, 3), generator=g, dtype=torch.float64)
        up.backward(dl.permute(0, 3, 1, 2))
        s, a, t = FR.upsample_add_bwd_ref(dl, (ht, wt))
        assert torch.allclose(top.grad.permute(0, 2, 3, 1), s, rtol=0, atol=1e-12)
        assert 1 <= float(t.min()) and float(t.max()) <= 4


def test_new_entry_points_are_bound_and_wrapped():
    from seam_match_rcnn_amd import _native, ops, ops_train
    for name in ("seam_roi_align_bwd_workspace_bytes", "seam_roi_align_bwd_f32", "seam_rpn_scatter_patches_f32",
                 "seam_upsample_add_bwd_f32", "seam_subsample_add_bwd_f32"):
        assert name in _native.SIGNATURES, name
    for name in ("roi_align_bwd", "rpn_scatter_patches", "upsample_add_bwd", "subsample_add_bwd", "conv_wgrad_chunked"):
        assert callable(getattr(ops, name)), name
    assert isinstance(ops_train.WGRAD_MAX_OPERAND_BYTES, int) and ops_train.WGRAD_MAX_OPERAND_BYTES < 2 ** 31
    from seam_match_rcnn_amd import autograd
    for name in ("RoIAlignFunction", "RPNPatchesFunction", "FPNFunction"):
        assert issubclass(getattr(autograd, name), torch.autograd.Function), name


def test_wrappers_refuse_host_tensors_and_bad_shapes():
    """No CPU path exists: a host tensor is refused before the library is touched, like the forward twins."""
    from seam_match_rcnn_amd import _native, ops
    x = torch.zeros((2, 7, 7, 8))
    with pytest.raises(_native.SeamNativeError):
        ops.roi_align_bwd(x, torch.zeros((2, 5)), FR.ROI_HWS, 2, FR.ROI_SCALES)
    with pytest.raises(_native.SeamNativeError):
        ops.rpn_scatter_patches(torch.zeros((2, 3, 3, 8)), torch.zeros((2, 4), dtype=torch.int32), FR.SCATTER_HWS, 2)
    with pytest.raises(_native.SeamNativeError):
        ops.upsample_add_bwd(x, (4, 4))
    with pytest.raises(_native.SeamNativeError):
        ops.subsample_add_bwd(x, torch.zeros((2, 4, 4, 8)))
    with pytest.raises(_native.SeamNativeError):
        ops.conv_wgrad_chunked(x, x, 1, 1)


def test_host_side_refusals_launch_nothing():
    """The refusals of include/seam_hip.h are host-side checks made before any launch, so they can be exercised without a
    device: every pointer below is a host buffer that a launched kernel would fault on."""
    import ctypes as C
    from seam_match_rcnn_amd import _native
    lib = _native.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    hw = (C.c_int * 8)(20, 24, 10, 12, 5, 6, 3, 3)
    sc = FR.ROI_SCALES

    def roi(c=8, n=2, k=3, pp=7, sr=2, dout=p, rois=p, d0=p, ws=p, hw_=hw):
        return lib.seam_roi_align_bwd_f32(dout, rois, None, hw_, c, *sc, 2, n, k, pp, sr, d0, p, p, p, ws, None)

    assert roi(c=6) != 0 and roi(c=4100) != 0 and roi(c=0) != 0
    assert roi(pp=0) != 0 and roi(pp=33) != 0 and roi(sr=0) != 0 and roi(sr=-1) != 0
    assert roi(n=0) != 0 and roi(k=-1) != 0
    assert roi(dout=None) != 0 and roi(rois=None) != 0 and roi(d0=None) != 0 and roi(ws=None) != 0
    assert roi(hw_=(C.c_int * 8)(0, 24, 10, 12, 5, 6, 3, 3)) != 0
    assert roi(c=4096, n=1, hw_=(C.c_int * 8)(400, 400, 10, 12, 5, 6, 3, 3)) != 0          # 400*400*4096*4 B = 2.4 GiB
    assert lib.seam_roi_align_bwd_workspace_bytes(0, 5) == 0 and lib.seam_roi_align_bwd_workspace_bytes(2, -1) == 0
    assert lib.seam_roi_align_bwd_workspace_bytes(2, 0) > 0
    assert lib.seam_roi_align_bwd_workspace_bytes(2, 40) >= 40 * 40 + 2 * 4 * 8

    maps = (C.c_void_p * 3)(p.value, p.value, p.value)
    hw3 = (C.c_int * 6)(6, 7, 3, 4, 2, 2)

    def scat(m=5, n=2, l=3, c=8, dp=p, rows=p, maps_=maps, hw_=hw3):
        return lib.seam_rpn_scatter_patches_f32(dp, rows, m, n, l, c, maps_, hw_, None)

    assert scat(m=0) != 0 and scat(m=(1 << 20) + 1) != 0 and scat(n=0) != 0 and scat(l=0) != 0 and scat(l=9) != 0
    assert scat(c=6) != 0 and scat(c=4100) != 0 and scat(dp=None) != 0 and scat(rows=None) != 0
    assert scat(maps_=(C.c_void_p * 3)(p.value, None, p.value)) != 0 and scat(hw_=(C.c_int * 6)(6, 7, 0, 4, 2, 2)) != 0
    up = lib.seam_upsample_add_bwd_f32
    assert up(p, None, p, 1, 8, 8, 4, 4, 6, None) != 0 and up(None, None, p, 1, 8, 8, 4, 4, 8, None) != 0
    assert up(p, None, None, 1, 8, 8, 4, 4, 8, None) != 0 and up(p, None, p, 0, 8, 8, 4, 4, 8, None) != 0
    sub = lib.seam_subsample_add_bwd_f32
    assert sub(p, p, 1, 7, 6, 3, 3, 8, None) != 0 and sub(p, p, 1, 7, 6, 4, 3, 6, None) != 0 and sub(None, p, 1, 7, 6, 4, 3, 8, None) != 0
