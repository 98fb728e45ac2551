"""CPU: the case generators of ``fpn_body_stress_cases.py`` -- deterministic, with every corner of ``REQUIRED`` reached -- the
float64 references at the new extremes against torch autograd, and the conditions the GPU sweep
(``test_gpu_stress_fpn_body_train.py``) relies on, shown here on the references alone."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_body_stress_cases as SC
import fpn_train_refs as FR

ROI_COST_MAX = 60e6        # products one einsum of roi_align_bwd_scatter visits per case: well under a second


def _same(a, b):
    if isinstance(a, torch.Tensor):
        if not isinstance(b, torch.Tensor) or a.dtype != b.dtype or a.shape != b.shape:
            return False
        if a.dtype == torch.float32:                              # bit for bit: NaNs and signed zeros included
            return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
        return torch.equal(a, b)
    return a == b


def _first(kernel, tag, without=()):
    for cs in SC.GENERATORS[kernel]():
        if tag in cs["tags"] and not any(t in cs["tags"] for t in without):
            return cs
    raise AssertionError((kernel, tag))


@pytest.mark.parametrize("kernel", sorted(SC.GENERATORS))
def test_generators_are_deterministic_and_meet_required(kernel):
    one, two = list(SC.GENERATORS[kernel]()), list(SC.GENERATORS[kernel]())
    assert len(one) == len(two) == SC.CASES[kernel]
    assert len({cs["name"] for cs in one}) == len(one)
    for a, b in zip(one, two):
        assert sorted(a) == sorted(b)
        assert all(_same(a[k], b[k]) for k in a), a["name"]
    counts = {}
    for cs in one:
        for t in cs["tags"]:
            counts[t] = counts.get(t, 0) + 1
    print(kernel, dict(sorted(counts.items())))
    for tag, least in SC.REQUIRED[kernel].items():
        assert counts.get(tag, 0) >= least, (kernel, tag, counts.get(tag, 0), least)


def test_case_tables_hold_what_the_kernels_ask_for():
    """The value sets the sweep is meant to vary over, and the size limits that keep it quick."""
    roi = list(SC.roi_align_bwd_cases())
    assert {cs["N"] for cs in roi} == {1, 2, 3, 4, 5} and {cs["P"] for cs in roi} == {1, 2, 5, 7, 14, 32}
    assert {cs["sr"] for cs in roi} == {1, 2, 3, 4} and {cs["C"] for cs in roi} == {4, 8, 64, 256, 260, 512}
    for cs in roi:
        assert all(1 <= h <= 41 and 1 <= w <= 41 for h, w in cs["hws"]) and cs["scales"] == list(FR.ROI_SCALES), cs["name"]
        if cs["C"] > 256:
            assert cs["K"] <= 64 and all(h <= 16 and w <= 16 for h, w in cs["hws"]), cs["name"]
        if "k_gt_256" in cs["tags"]:
            assert 257 <= cs["K"] <= 700
        assert cs["roi_reference_cost"] <= ROI_COST_MAX, (cs["name"], cs["roi_reference_cost"])
    sc = list(SC.rpn_scatter_cases())
    assert {cs["L"] for cs in sc} == set(range(1, 9)) and {cs["N"] for cs in sc} == {1, 2, 3, 4}
    assert {cs["C"] for cs in sc} == {4, 8, 64, 72, 256} and {cs["M"] for cs in sc} == {1, 37, 300, 2000}
    assert all(1 <= h <= 12 and 1 <= w <= 15 for cs in sc for h, w in cs["hws"])
    up = list(SC.upsample_add_bwd_cases())
    assert {cs["C"] for cs in up} == {4, 12, 256} and {cs["N"] for cs in up} == {1, 2, 3}
    assert any(cs["fine"] == (25, 18) and cs["coarse"] == (9, 7) for cs in up)
    sub = list(SC.subsample_add_bwd_cases())
    assert {cs["C"] for cs in sub} == {4, 12, 256} and all(1 <= cs["H"] <= 19 and 1 <= cs["W"] <= 19 for cs in sub)
    dg = list(SC.conv3x3s2_dgrad_cases())
    assert {cs["C"] for cs in dg} == {32, 64, 96, 128, 192, 256, 512} and {cs["K"] for cs in dg} == {32, 64, 96, 256, 512}
    assert all(cs["H"] <= 9 and cs["W"] <= 11 for cs in dg if cs["C"] >= 512 or cs["K"] >= 512)
    assert all(4 * cs["K"] <= 4608 for cs in dg)                   # the reduction length `close` is the project's figure for
    pool = list(SC.maxpool3s2_relu_bwd_cases())
    assert any(cs["H"] == 1 for cs in pool) and any(cs["W"] == 1 for cs in pool)
    relu = list(SC.relu_mask_add_cases())
    lanes = sorted(cs["M"] * cs["C"] // 4 for cs in relu)
    assert lanes[0] == 1 and 1024 < lanes[-1] <= 1100 and {cs["C"] for cs in relu} == {4, 12, 36, 64}


# ------------------------------------------------------------------------------ what the GPU sweep relies on
@functools.lru_cache(maxsize=None)
def roi_stats():
    """Per roi case: (name, the bound (T + 8) U A is finite everywhere, number of levels with a non-zero A)."""
    out = []
    for cs in SC.roi_align_bwd_cases():
        ref = SC.roi_reference(cs)
        finite = all(bool(torch.isfinite((t + 8) * FR.U * a).all()) and bool(torch.isfinite(s).all()) for s, a, t in ref)
        out.append((cs["name"], finite, sum(int(bool((a > 0).any())) for s, a, t in ref)))
    return out


def test_every_roi_bound_is_finite_and_most_cases_reach_two_levels():
    stats = roi_stats()
    assert all(fin for _, fin, _ in stats), [n for n, fin, _ in stats if not fin]
    two = sum(1 for _, _, lv in stats if lv >= 2)
    print(f"{two} of {len(stats)} roi cases have a non-zero A on at least two levels")
    assert two >= 0.9 * len(stats), stats


def test_pile_up_reaches_two_hundred_terms_on_a_pixel():
    seen = 0
    for cs in SC.rpn_scatter_cases():
        if "pile_up" not in cs["tags"]:
            continue
        ref = FR.scatter_patches_ref(cs["dpatch"], cs["rows"], cs["hws"], cs["N"])
        worst = max(float(t.max()) for s, a, t in ref)
        print(cs["name"], "largest T", worst)
        assert worst >= 200, cs["name"]
        seen += 1
    assert seen >= SC.REQUIRED["rpn_scatter"]["pile_up"]


def test_coarse_gt_fine_leaves_pixels_without_a_term():
    for cs in SC.upsample_add_bwd_cases():
        s, a, t = FR.upsample_add_bwd_ref(cs["dlat"], cs["coarse"])
        assert int(t.sum()) == cs["N"] * cs["fine"][0] * cs["fine"][1] * cs["C"]      # every fine pixel lands exactly once
        assert bool((t == 0).any()) == ("coarse_gt_fine" in cs["tags"]), cs["name"]


# ------------------------------------------------------------------------------ the references against autograd at the new extremes
@pytest.mark.parametrize("tag", ["p32", "one_by_one_level", "many_tiles"])
def test_roi_scatter_equals_autograd_of_the_oracle(tag):
    cs = _first("roi_align_bwd", tag, without=("bad_rois",))
    lv = cs["ref_levels"]
    ok = cs["keep"] & (lv >= 0) & (lv <= 3)                        # the oracle takes no level outside the pyramid
    dout, rois, lv = cs["dout"][ok][..., :3].double(), cs["rois"][ok], lv[ok]
    ref = FR.roi_align_bwd_scatter(dout, rois, lv, cs["hws"], cs["scales"], cs["sr"], cs["N"])
    auto = FR.roi_align_bwd_autograd(dout, rois, lv, cs["hws"], cs["scales"], cs["sr"], cs["N"])
    seen = 0
    for (s, a, t), g in zip(ref, auto):
        # the oracle rounds each tap's weight product to fp32 (one rounding per term); the scatter keeps it in float64
        assert bool(((s - g).abs() <= 2 * FR.U * a + 1e-300).all()), (cs["name"], float(((s - g).abs() - 2 * FR.U * a).max()))
        assert bool((s[t[..., :3] == 0] == 0).all())
        seen += int((t > 0).any())
    assert seen >= 2, cs["name"]


@pytest.mark.parametrize("tag", ["ratio1", "ratio2", "ratio2_odd", "ratio_ge3", "ratio_fraction", "coarse_gt_fine", "coarse_1x1"])
def test_merge_reference_equals_fp32_autograd_on_integers(tag):
    cs = _first("upsample_add_bwd", tag)
    n, (h, w), (ht, wt) = cs["N"], cs["fine"], cs["coarse"]
    g = torch.Generator().manual_seed(h * 100 + w)
    dl = torch.randint(-8, 9, (n, h, w, 4), generator=g).float()     # integers: every sum is exact in fp32 and in float64
    top = torch.zeros((n, 4, ht, wt), requires_grad=True)
    F.interpolate(top, size=(h, w), mode="nearest").backward(dl.permute(0, 3, 1, 2))
    s, a, t = FR.upsample_add_bwd_ref(dl, (ht, wt))
    assert torch.equal(top.grad.permute(0, 2, 3, 1).double(), s), cs["name"]


def test_scatter_reference_equals_autograd_of_the_gather_on_eight_levels():
    cs = _first("rpn_scatter", "l8")
    g = torch.Generator().manual_seed(8)
    feats = [torch.randn((cs["N"], h, w, 4), generator=g, dtype=torch.float64).requires_grad_(True) for h, w in cs["hws"]]
    dp = cs["dpatch"][..., :4].double()
    (FR.gather_patches_ref(feats, cs["rows"]) * dp).sum().backward()
    ref = FR.scatter_patches_ref(dp, cs["rows"], cs["hws"], cs["N"])
    assert len(ref) == 8
    for f, (s, a, t) in zip(feats, ref):
        grad = f.grad if f.grad is not None else torch.zeros_like(f)
        assert torch.allclose(grad, s, rtol=0, atol=1e-12)


def test_dgrad_reference_counts_the_taps():
    cs = _first("conv3x3s2_dgrad", "k_lt_c")
    dx, a, t = SC.dgrad_reference(cs, True)
    k = cs["K"]
    assert float(t[0, 0, 0, 0]) == k and float(t.max()) == (4 * k if min(cs["H"], cs["W"]) > 1 else 2 * k)
    assert bool((a >= dx.abs() - 1e-12).all()) and dx.shape == (cs["N"], cs["H"], cs["W"], cs["C"])
    plain = SC.dgrad_reference(cs, False)[0]
    assert not torch.equal(plain, dx)
