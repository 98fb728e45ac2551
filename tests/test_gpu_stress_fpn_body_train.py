"""Seeded stress of the adjoint kernels that carry the gradient from the heads down through the FPN, the ResNet body and the stem
(``csrc/seam_fpn_train.hip``, ``csrc/seam_body_train.hip``) through the C ABI, in the form of ``test_gpu_stress_roi_train.py``:
every output is POISONED and followed by a 1 MiB guard; each case of ``fpn_body_stress_cases.py`` runs twice and the two results
must be bit-identical (fixed-order sums, no float atomics); after each case the guards are intact and no element of an output
that must be written completely still holds the poison.  Each launcher's refusals must leave every output untouched.

References and bounds (derived, none measured)
  roi_align_bwd        ``fpn_train_refs.roi_align_bwd_scatter`` under (T + 8) 2^-24 A per element, the bound test_gpu_fpn_train.py
                       justifies; on eight cases also the adjoint identity with ``ops.roi_align`` under that file's 2 x bound rule
  rpn_scatter          ``scatter_patches_ref`` under (T + 2) 2^-24 A; adjoint identity with ``ops.rpn_gather_patches``
  upsample_add_bwd     ``upsample_add_bwd_ref`` under (T + 2) 2^-24 A; a coarse pixel nothing maps to is ``base`` or zero, exactly
  subsample_add_bwd    exact: d[:, ::2, ::2] += dpool is one fp32 addition per element
  conv3x3s2_dgrad      float64 ``F.conv2d(...).backward``.  The kernel is an fp32 fma chain in a fixed order over T = taps * K
                       terms (1, 2, 2 or 4 taps by the pixel's row and column parity), so |err| <= (T + 3) 2^-24 A with A the same
                       transposed convolution of |dy| with |w * scale|: T roundings of the chain, and 3 for folding the scale into
                       the packed weight, the term's product and the final value.  Also the project's ``close`` (rtol 2e-4, atol
                       2e-5 of the largest element; every reduction here is at most 4 * 512 = 2048 terms, below the 4608
                       test_gpu_stress_igemm.py cites for it), which alone judges the zero-stuffed composition (selector 0).
  maxpool3s2_relu_bwd  torch's CPU gradient of max_pool2d(relu(y), 3, 2, 1), ``torch.equal``: y on k/4 and dpool on k/64 make every
                       sum exact
  relu_mask_add        ``torch.where(y > 0, a + b, 0)`` bit for bit (compared as int32)

The roi workspace is handed over zero-filled: a list slot the compaction failed to write then names ROI 0 -- a wrong sum that
the comparison reports, never an index outside the arrays.
"""
import ctypes as C
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_body_stress_cases as SC
import fpn_train_refs as FR
from stress_kit import Buf, P, st

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
U = FR.U
# The whole module took 4.0 s on the MI355X (the float64 references on the host included); the limit is three times that,
# rounded up to 10 s, for a shared and loaded machine.
SWEEP_LIMIT_S = 20.0


def _lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def close(got, want, rtol=2e-4, atol_frac=2e-5, msg=""):
    """``close`` of tests/test_gpu_train.py."""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape, msg)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_frac * (float(np.abs(want).max()) + 1e-30) + 1e-9, err_msg=msg)


@pytest.fixture(scope="module", autouse=True)
def module_clock():
    return {"t0": time.perf_counter()}


def _twice(launch, desc, fully_written=True):
    """Run ``launch`` (-> rc, [Buf]) twice: accepted, guards intact, everything written, the same bits.  Returns the first run."""
    a_rc, a = launch()
    b_rc, b = launch()
    assert a_rc == 0 and b_rc == 0, (desc, a_rc, b_rc)
    assert all(o.guard_ok() for o in a + b), desc
    if fully_written:
        assert all(o.filled() for o in a + b), desc
    assert all(torch.equal(x.bits(), y.bits()) for x, y in zip(a, b)), desc
    return a


# ------------------------------------------------------------------------------------------------ RoIAlign adjoint
def _roi_launch(lib, cs, dev, **over):
    n, c, k, p, sr, hws = (over.get(x, cs[x]) for x in ("N", "C", "K", "P", "sr", "hws"))
    outs = over["outs"] if "outs" in over else [Buf((cs["N"], h, w, cs["C"])) for h, w in cs["hws"]]
    nws = max(int(lib.seam_roi_align_bwd_workspace_bytes(cs["N"], cs["K"])), 16)
    ws = over["ws"] if "ws" in over else torch.zeros((nws,), dtype=torch.uint8, device=DEV)
    hw = (C.c_int * 8)(*[d for s in hws for d in s])
    ptrs = [P(o.t) for o in outs]
    if "null_map" in over:
        ptrs[over["null_map"]] = None
    rc = lib.seam_roi_align_bwd_f32(P(over.get("dout", dev["dout"])), P(over.get("rois", dev["rois"])), P(dev["levels"]), hw, c,
                                    *cs["scales"], FR.K_MIN, n, k, p, sr, *ptrs, P(ws), st())
    torch.cuda.synchronize()
    return rc, outs


ROI_ADJOINT_TAGS = ["k_gt_256", "c_second_chunk", "c_ragged_chunk", "p32", "one_by_one_level", "many_tiles", "tile_border_edges",
                    "mapped_levels"]


def test_stress_roi_align_bwd():
    from seam_match_rcnn_amd import ops
    lib = _lib()
    worst, adjoint_left, n_adjoint, last, failed = 0.0, list(ROI_ADJOINT_TAGS), 0, None, []
    for cs in SC.roi_align_bwd_cases():
        desc = (cs["name"], sorted(cs["tags"]))
        dev = dict(dout=cs["dout"].to(DEV), rois=cs["rois"].to(DEV), levels=None if cs["levels"] is None else cs["levels"].to(DEV))
        outs = _twice(lambda: _roi_launch(lib, cs, dev), desc)
        ref = SC.roi_reference(cs)
        last = (cs, dev)
        try:
            ratio = max(FR.within(o.t, r, 8) for o, r in zip(outs, ref))
        except AssertionError as e:                                # every failing case is named, not the first alone
            failed.append((desc, e.args))
            print(f"{cs['name']}: FAILED {e.args}")
            continue
        worst = max(worst, ratio)
        print(f"{cs['name']}: worst error / bound {ratio:.3f}")
        # the adjoint identity <fwd(F), G> == <F, bwd(G)> on the ROIs the forward may be given (a level inside the pyramid)
        tag = next((t for t in adjoint_left if t in cs["tags"]), None)
        if tag is None or "bad_rois" in cs["tags"]:
            continue
        adjoint_left.remove(tag)
        n_adjoint += 1
        ok = (cs["ref_levels"] >= 0) & (cs["ref_levels"] <= 3)
        rois, g = cs["rois"][ok].contiguous(), cs["dout"][ok].contiguous()
        lv = None if cs["levels"] is None else cs["levels"][ok].contiguous().to(DEV)
        gen = torch.Generator().manual_seed(cs["K"])
        feats = [torch.randn((cs["N"], h, w, cs["C"]), generator=gen) for h, w in cs["hws"]]
        fwd = ops.roi_align([f.to(DEV) for f in feats], rois.to(DEV), cs["scales"], cs["P"], cs["sr"], FR.K_MIN, lv)
        bwd = ops.roi_align_bwd(g.to(DEV), rois.to(DEV), cs["hws"], cs["N"], cs["scales"], cs["sr"], FR.K_MIN, lv)
        assert all(torch.equal(b, o.t) for b, o in zip(bwd, outs)), desc          # dropping the out-of-range levels changes nothing
        lhs = float((fwd.cpu().double() * g.double()).sum())
        rhs = sum(float((b.cpu().double() * f.double()).sum()) for b, f in zip(bwd, feats))
        bound = sum(float(((t + 8) * U * a * f.double().abs()).sum()) for (s, a, t), f in zip(ref, feats))
        print(f"{cs['name']} [{tag}]: <fwd(F),G> {lhs!r} <F,bwd(G)> {rhs!r} diff {abs(lhs - rhs):.3e} bound 2 x {bound:.3e}")
        assert abs(lhs - rhs) <= 2 * bound, desc
    print(f"roi_align_bwd: worst error / bound over the sweep {worst:.3f}; adjoint identity on {n_adjoint} cases")
    assert not failed, failed
    assert n_adjoint >= 6 and worst <= 1.0
    # refusals: nothing is written
    cs, dev = last
    small = torch.zeros((1 << 16,), dtype=torch.uint8, device=DEV)
    for bad in (dict(C=6), dict(C=4100), dict(P=0), dict(P=33), dict(sr=0), dict(sr=65), dict(N=0), dict(K=-1), dict(K=(1 << 20) + 1),
                dict(dout=None), dict(rois=None), dict(null_map=2), dict(ws=None), dict(hws=[(20, 24), (0, 12), (5, 6), (3, 3)]),
                dict(hws=[(20, 24), (10, 12), (5, -1), (3, 3)])):
        rc, outs = _roi_launch(lib, cs, dev, **dict(dict(ws=small), **bad))
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in outs), bad


# ------------------------------------------------------------------------------------------------ RPN window scatter
def _scatter_launch(lib, cs, dev, **over):
    m, n, l, c = (over.get(x, cs[x]) for x in ("M", "N", "L", "C"))
    hws = over.get("hws", cs["hws"])
    outs = [Buf((cs["N"], h, w, cs["C"])) for h, w in cs["hws"]]
    ptrs = [o.t.data_ptr() for o in outs]
    if "null_map" in over:
        ptrs[over["null_map"]] = None
    maps = (C.c_void_p * len(outs))(*ptrs)
    hw = (C.c_int * (2 * len(hws)))(*[d for s in hws for d in s])
    rc = lib.seam_rpn_scatter_patches_f32(P(over.get("dpatch", dev["dpatch"])), P(over.get("rows", dev["rows"])), m, n, l, c,
                                          None if over.get("null_maps") else maps, hw, st())
    torch.cuda.synchronize()
    return rc, outs


def test_stress_rpn_scatter():
    from seam_match_rcnn_amd import ops
    lib = _lib()
    worst, n_adjoint, last, failed = 0.0, 0, None, []
    for cs in SC.rpn_scatter_cases():
        desc = (cs["name"], sorted(cs["tags"]))
        dev = dict(dpatch=cs["dpatch"].to(DEV), rows=cs["rows"].to(DEV))
        outs = _twice(lambda: _scatter_launch(lib, cs, dev), desc)
        ref = FR.scatter_patches_ref(cs["dpatch"], cs["rows"], cs["hws"], cs["N"])
        try:
            ratio = max(FR.within(o.t, r, 2) for o, r in zip(outs, ref))
        except AssertionError as e:
            failed.append((desc, e.args))
            print(f"{cs['name']}: FAILED {e.args}")
            continue
        worst = max(worst, ratio)
        print(f"{cs['name']}: worst error / bound {ratio:.3f}, largest T {max(float(t.max()) for s, a, t in ref):.0f}")
        if cs["L"] == 3:
            last = (cs, dev)
        if "bad_rows" in cs["tags"]:
            continue
        gen = torch.Generator().manual_seed(cs["M"] + cs["C"])
        feats = [torch.randn((cs["N"], h, w, cs["C"]), generator=gen) for h, w in cs["hws"]]
        patches = ops.rpn_gather_patches([f.to(DEV) for f in feats], dev["rows"])
        assert torch.equal(patches.cpu().double(), FR.gather_patches_ref(feats, cs["rows"])), desc       # a gather is exact
        lhs = float((patches.cpu().double() * cs["dpatch"].double()).sum())
        rhs = sum(float((o.t.cpu().double() * f.double()).sum()) for o, f in zip(outs, feats))
        bound = sum(float(((t + 2) * U * a * f.double().abs()).sum()) for (s, a, t), f in zip(ref, feats))
        assert abs(lhs - rhs) <= bound, (desc, lhs, rhs, bound)
        n_adjoint += 1
    print(f"rpn_scatter: worst error / bound over the sweep {worst:.3f}; adjoint identity on {n_adjoint} cases")
    assert not failed, failed
    assert n_adjoint >= 10 and worst <= 1.0
    cs, dev = last
    for bad in (dict(M=0), dict(M=-3), dict(L=0), dict(L=9), dict(C=6), dict(C=4100), dict(N=0), dict(rows=None), dict(dpatch=None),
                dict(null_map=1), dict(null_maps=True), dict(hws=[cs["hws"][0], cs["hws"][1], (2, 0)]), dict(hws=[(0, 3)] + cs["hws"][1:])):
        rc, outs = _scatter_launch(lib, cs, dev, **bad)
        assert rc != 0 and all(o.untouched() and o.guard_ok() for o in outs), bad


# ------------------------------------------------------------------------------------------------ top-down merge and pool adjoints
def test_stress_upsample_add_bwd():
    lib = _lib()
    worst, failed = 0.0, []
    for cs in SC.upsample_add_bwd_cases():
        desc = (cs["name"], sorted(cs["tags"]))
        n, (h, w), (ht, wt), c = cs["N"], cs["fine"], cs["coarse"], cs["C"]
        dl, base = cs["dlat"].to(DEV), None if cs["base"] is None else cs["base"].to(DEV)

        def launch():
            out = Buf((n, ht, wt, c))
            rc = lib.seam_upsample_add_bwd_f32(P(dl), P(base), P(out.t), n, h, w, ht, wt, c, st())
            torch.cuda.synchronize()
            return rc, [out]
        (out,) = _twice(launch, desc)
        try:
            ratio = FR.within(out.t, FR.upsample_add_bwd_ref(cs["dlat"], cs["coarse"], cs["base"]), 2)
        except AssertionError as e:
            failed.append((desc, e.args))
            print(f"{cs['name']}: FAILED {e.args}")
            continue
        worst = max(worst, ratio)
        print(f"{cs['name']}: worst error / bound {ratio:.3f}")
        if "coarse_gt_fine" in cs["tags"]:                         # a coarse pixel nothing maps to: base, or zero, exactly
            empty = FR.upsample_add_bwd_ref(cs["dlat"], cs["coarse"])[2] == 0
            assert bool(empty.any()), desc
            got = out.t.cpu()
            want = cs["base"] if cs["base"] is not None else torch.zeros_like(got)
            assert torch.equal(got[empty], want[empty]), desc
    print(f"upsample_add_bwd: worst error / bound over the sweep {worst:.3f}")
    assert not failed, failed
    assert worst <= 1.0
    dl = torch.zeros((2, 8, 10, 12), device=DEV)
    for dims, null in (((2, 8, 10, 4, 5, 6), None), ((2, 8, 10, 4, 5, 0), None), ((0, 8, 10, 4, 5, 12), None), ((-1, 8, 10, 4, 5, 12), None),
                       ((2, 0, 10, 4, 5, 12), None), ((2, 8, 0, 4, 5, 12), None), ((2, 8, 10, 0, 5, 12), None), ((2, 8, 10, 4, 0, 12), None),
                       ((2, 8, 10, 4, 5, 12), "dlat"), ((2, 8, 10, 4, 5, 12), "dtop")):
        out = Buf((2, 4, 5, 12))
        rc = lib.seam_upsample_add_bwd_f32(None if null == "dlat" else P(dl), None, None if null == "dtop" else P(out.t), *dims, st())
        torch.cuda.synchronize()
        assert rc != 0 and out.untouched() and out.guard_ok(), (dims, null)


def test_stress_subsample_add_bwd():
    lib = _lib()
    for cs in SC.subsample_add_bwd_cases():
        n, h, w, c = (cs[x] for x in "NHWC")
        hp, wp = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        dp = cs["dpool"].to(DEV)

        def launch():
            d = Buf((n, h, w, c))
            d.t.copy_(cs["d"])                          # updated in place: the whole result is compared
            rc = lib.seam_subsample_add_bwd_f32(P(d.t), P(dp), n, h, w, hp, wp, c, st())
            torch.cuda.synchronize()
            return rc, [d]
        (d,) = _twice(launch, cs["name"])
        want = cs["d"].clone()
        want[:, ::2, ::2] += cs["dpool"]
        mism = int((d.t.cpu() != want).sum())
        print(f"{cs['name']}: mismatches {mism}")
        assert torch.equal(d.t.cpu(), want), cs["name"]
    print("subsample_add_bwd: exact on every case")
    dp = torch.zeros((2, 4, 3, 12), device=DEV)
    for dims, null in (((2, 7, 6, 3, 3, 12), None), ((2, 7, 6, 4, 4, 12), None), ((2, 7, 6, 4, 3, 6), None), ((2, 7, 6, 4, 3, 0), None),
                       ((0, 7, 6, 4, 3, 12), None), ((2, 0, 6, 0, 3, 12), None), ((2, 7, 0, 4, 0, 12), None), ((2, 7, 6, 4, 3, 12), "dpool"),
                       ((2, 7, 6, 4, 3, 12), "d")):
        d = Buf((2, 7, 6, 12))
        rc = lib.seam_subsample_add_bwd_f32(None if null == "d" else P(d.t), None if null == "dpool" else P(dp), *dims, st())
        torch.cuda.synchronize()
        assert rc != 0 and d.untouched() and d.guard_ok(), (dims, null)


# ------------------------------------------------------------------------------------------------ stride-2 input gradient
def test_stress_conv3x3s2_dgrad():
    from seam_match_rcnn_amd import _native, ops
    lib = _lib()
    worst = 0.0
    before = _native.get_option("SEAM_S2_DGRAD")
    try:
        for cs in SC.conv3x3s2_dgrad_cases():
            n, h, w, c, k = (cs[x] for x in "NHWCK")
            dy, wt, mask_d = cs["dy"].to(DEV), cs["w"].to(DEV), cs["mask"].to(DEV)
            for with_scale in (False, True):
                want, a, t = SC.dgrad_reference(cs, with_scale)
                scale = cs["scale"].to(DEV) if with_scale else None
                wp = Buf((9, c, k))
                assert lib.seam_pack_conv3x3s2_dgrad_f32(P(wt), P(scale), P(wp.t), k, c, st()) == 0
                torch.cuda.synchronize()
                assert wp.filled() and wp.guard_ok()
                pk = ops.pack_conv3x3s2_dgrad(wt, scale)
                assert torch.equal(pk.wp, wp.t)
                for with_mask in (False, True):
                    desc = (cs["name"], sorted(cs["tags"]), with_scale, with_mask)
                    mask = mask_d if with_mask else None

                    def launch():
                        dx = Buf((n, h, w, c))
                        rc = lib.seam_conv3x3s2_dgrad_f32(P(dy), P(wp.t), P(mask), P(dx.t), n, h, w, c, k, st())
                        torch.cuda.synchronize()
                        return rc, [dx]
                    (dx,) = _twice(launch, desc)
                    keep = (cs["mask"] > 0) if with_mask else torch.ones_like(cs["mask"], dtype=torch.bool)
                    got = dx.t.cpu()
                    ref = torch.where(keep, want, torch.zeros_like(want))
                    err, bound = (got.double() - ref).abs(), torch.where(keep, (t + 3) * U * a, torch.zeros_like(a))
                    ratio = float((err / bound.clamp(min=1e-300)).max())
                    worst = max(worst, ratio)
                    print(f"{cs['name']} scale={with_scale} mask={with_mask}: worst error / bound {ratio:.3f}, "
                          f"max err {float(err.max()):.3e} of {float(ref.abs().max()):.3e}")
                    assert bool((err <= bound).all()), desc
                    assert bool((got[~keep] == 0).all()), desc                       # masked elements are exactly zero
                    close(got, ref.float(), msg=str(desc))
                    _native.set_option("SEAM_S2_DGRAD", 1)                           # the wrapper's kernel route: the same launch
                    assert torch.equal(ops.conv3x3s2_dgrad(dy, pk, (h, w), mask=mask), dx.t), desc
                    _native.set_option("SEAM_S2_DGRAD", 0)                           # the zero-stuffed composition, under `close`
                    comp = ops.conv3x3s2_dgrad(dy, pk, (h, w), mask=mask)
                    close(comp, ref.float(), msg=str(desc) + " composition")
                    assert bool((comp[~keep.to(DEV)] == 0).all()), desc
    finally:
        _native.set_option("SEAM_S2_DGRAD", before)
    print(f"conv3x3s2_dgrad: worst error / bound over the sweep {worst:.3f}")
    assert worst <= 1.0
    dy, wp = torch.zeros((1, 2, 2, 32), device=DEV), torch.zeros((9, 32, 32), device=DEV)
    for dims, null in (((0, 4, 4, 32, 32), None), ((-1, 4, 4, 32, 32), None), ((1, 0, 4, 32, 32), None), ((1, 4, 0, 32, 32), None),
                       ((1, 4, 4, 48, 32), None), ((1, 4, 4, 32, 40), None), ((1, 4, 4, 0, 32), None), ((1, 4, 4, 32, 0), None),
                       ((1, 4, 4, 32, 32), "dy"), ((1, 4, 4, 32, 32), "wp"), ((1, 4, 4, 32, 32), "dx")):
        dx = Buf((1, 4, 4, 32))
        rc = lib.seam_conv3x3s2_dgrad_f32(None if null == "dy" else P(dy), None if null == "wp" else P(wp), None,
                                          None if null == "dx" else P(dx.t), *dims, st())
        torch.cuda.synchronize()
        assert rc != 0 and dx.untouched() and dx.guard_ok(), (dims, null)
    for kk, cc, null in ((40, 32, None), (32, 48, None), (0, 32, None), (32, 0, None), (32, 32, "w"), (32, 32, "out")):
        out = Buf((9, 32, 32))
        rc = lib.seam_pack_conv3x3s2_dgrad_f32(None if null == "w" else P(wp), None, None if null == "out" else P(out.t), kk, cc, st())
        torch.cuda.synchronize()
        assert rc != 0 and out.untouched() and out.guard_ok(), (kk, cc, null)


# ------------------------------------------------------------------------------------------------ stem pool adjoint, ReLU mask
def test_stress_maxpool3s2_relu_bwd():
    lib = _lib()
    for cs in SC.maxpool3s2_relu_bwd_cases():
        desc = (cs["name"], sorted(cs["tags"]))
        n, h, w, c = (cs[x] for x in "NHWC")
        y, dpool = cs["y"].to(DEV), cs["dpool"].to(DEV)

        def launch():
            dy = Buf((n, h, w, c))
            rc = lib.seam_maxpool3s2_relu_bwd_f32(P(y), P(dpool), P(dy.t), n, h, w, c, st())
            torch.cuda.synchronize()
            return rc, [dy]
        (dy,) = _twice(launch, desc)
        z = cs["y"].permute(0, 3, 1, 2).contiguous().requires_grad_(True)
        F.max_pool2d(torch.relu(z), 3, 2, 1).backward(cs["dpool"].permute(0, 3, 1, 2).contiguous())
        want = z.grad.permute(0, 2, 3, 1).contiguous()
        got = dy.t.cpu()
        print(f"{cs['name']} {sorted(t for t in cs['tags'] if t[0] in 'xn')}: mismatches {int((got != want).sum())}")
        assert torch.equal(got, want), desc
        assert bool((got[cs["y"] <= 0] == 0).all()), desc           # the negative zero counts as not positive
    print("maxpool3s2_relu_bwd: exact on every case")
    y, dpool = torch.ones((1, 4, 4, 8), device=DEV), torch.ones((1, 2, 2, 8), device=DEV)
    for dims, null in (((1, 4, 4, 6), None), ((0, 4, 4, 8), None), ((-1, 4, 4, 8), None), ((1, 0, 4, 8), None), ((1, 4, 0, 8), None),
                       ((1, 4, 4, 0), None), ((1, 4, 4, 8), "y"), ((1, 4, 4, 8), "dpool"), ((1, 4, 4, 8), "dy")):
        dy = Buf((1, 4, 4, 8))
        rc = lib.seam_maxpool3s2_relu_bwd_f32(None if null == "y" else P(y), None if null == "dpool" else P(dpool),
                                              None if null == "dy" else P(dy.t), *dims, st())
        torch.cuda.synchronize()
        assert rc != 0 and dy.untouched() and dy.guard_ok(), (dims, null)


def test_stress_relu_mask_add():
    lib = _lib()
    for cs in SC.relu_mask_add_cases():
        m, c = cs["M"], cs["C"]
        y, a, b = cs["y"].to(DEV), cs["a"].to(DEV), None if cs["b"] is None else cs["b"].to(DEV)

        def launch():
            out = Buf((m, c))
            rc = lib.seam_relu_mask_add_f32(P(y), P(a), P(b), P(out.t), m, c, st())
            torch.cuda.synchronize()
            return rc, [out]
        (out,) = _twice(launch, cs["name"])
        want = torch.where(cs["y"] > 0, cs["a"] + cs["b"] if cs["b"] is not None else cs["a"], torch.zeros(()))
        mism = int((out.bits().cpu().view(-1) != want.view(torch.int32).view(-1)).sum())
        print(f"{cs['name']}: mismatching bit patterns {mism}")
        assert torch.equal(out.bits().cpu().view(-1), want.view(torch.int32).view(-1)), cs["name"]
    print("relu_mask_add: bit for bit on every case")
    z = torch.zeros((8, 4), device=DEV)
    for mm, cc, null in ((0, 4, None), (-1, 4, None), (8, 6, None), (8, 0, None), (8, 4, "y"), (8, 4, "a"), (8, 4, "out")):
        out = Buf((8, 4))
        rc = lib.seam_relu_mask_add_f32(None if null == "y" else P(z), None if null == "a" else P(z), None,
                                        None if null == "out" else P(out.t), mm, cc, st())
        torch.cuda.synchronize()
        assert rc != 0 and out.untouched() and out.guard_ok(), (mm, cc, null)


def test_stress_fpn_body_sweep_is_fast(module_clock):
    """The wall time of the whole module (this test runs last), references on the host included."""
    secs = time.perf_counter() - module_clock["t0"]
    print(f"test_gpu_stress_fpn_body_train.py: {secs:.1f} s of wall time, limit {SWEEP_LIMIT_S:.0f} s")
    assert secs <= SWEEP_LIMIT_S, secs
