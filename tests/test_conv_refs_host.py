"""CPU: the float64 references of tests/conv_refs.py against torch's own float64 operators, the host mirror of the implicit GEMM's
indexing against those references, and the case generator of tests/test_gpu_stress_igemm.py against the launchers' acceptance
rule and the corner counts it promises -- all before anything is launched on a GPU."""
import math

import pytest
import torch
import torch.nn.functional as F

import conv_refs as CR
import test_gpu_stress_igemm as G


def rnd(seed, *shape):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def nhwc(t):
    return t.permute(0, 2, 3, 1)


# (n, h, w, c, k, R, S, stride, pad, crop): R != S, stride 3, pad >= R, the crop, one-pixel maps, kernels as large as the padded input
CONV_SHAPES = [
    (2, 9, 11, 4, 5, 3, 3, 1, 1, None), (1, 7, 5, 12, 3, 1, 3, 1, 0, None), (2, 8, 13, 8, 6, 3, 1, 2, 1, None),
    (1, 10, 17, 20, 4, 1, 7, 3, 3, None), (3, 11, 6, 6, 7, 7, 1, 3, 2, None), (2, 6, 7, 5, 3, 2, 3, 2, 0, None),
    (1, 5, 5, 3, 2, 1, 1, 1, 3, None), (2, 4, 6, 7, 5, 2, 2, 3, 3, None), (1, 1, 1, 9, 4, 3, 3, 1, 1, None),
    (1, 13, 13, 4, 8, 7, 7, 2, 3, (4, 6)), (2, 9, 8, 24, 3, 5, 5, 1, 2, (1, 1)), (1, 12, 9, 28, 2, 2, 3, 1, 1, (12, 8)),
    (2, 3, 3, 2, 3, 5, 5, 3, 1, None), (1, 16, 16, 12, 64, 4, 4, 1, 2, (15, 15)),
]


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_nhwc_f64_matches_conv2d(shape):
    n, h, w, c, k, R, S, stride, pad, crop = shape
    x, wt = rnd(1, n, h, w, c), rnd(2, k, c, R, S)
    ref = nhwc(F.conv2d(nchw(x), wt, None, stride, pad))
    if crop:
        ref = ref[:, :crop[0], :crop[1]]
    got = CR.conv_nhwc_f64(x, wt, R, S, stride, pad, *(crop or (None, None)))
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert float((got - ref).abs().max()) <= 1e-12 * max(float(ref.abs().max()), 1.0)
    # float32 operands are taken exactly
    got32 = CR.conv_nhwc_f64(x.float(), wt.float(), R, S, stride, pad, *(crop or (None, None)))
    ref32 = nhwc(F.conv2d(nchw(x.float().double()), wt.float().double(), None, stride, pad))
    if crop:
        ref32 = ref32[:, :crop[0], :crop[1]]
    assert float((got32 - ref32).abs().max()) <= 1e-12 * max(float(ref32.abs().max()), 1.0)


def test_epilogue_f64_modes():
    acc, res = rnd(3, 2, 3, 4, 5), rnd(4, 2, 3, 4, 5)
    scale, shift = rnd(5, 5).abs() + 0.5, rnd(6, 5)
    base = acc * scale + shift
    assert torch.equal(CR.epilogue_f64(acc, scale, shift, None, 0), base)
    assert torch.equal(CR.epilogue_f64(acc, None, None, None, 0), acc)
    assert torch.equal(CR.epilogue_f64(acc, None, shift, res, 0), acc + shift + res)
    assert torch.equal(CR.epilogue_f64(acc, scale, shift, res, 1), F.relu(base + res))
    assert torch.equal(CR.epilogue_f64(acc, scale, shift, None, 1), F.relu(base))
    m2 = CR.epilogue_f64(acc, scale, shift, res, 2)
    assert torch.equal(m2, base * (res > 0)) and bool((m2[res <= 0] == 0).all()) and bool((m2 != 0).any())
    # mode 2 is the gradient of relu(z) at z = res: autograd agrees
    z = res.clone().requires_grad_(True)
    F.relu(z).backward(base)
    assert torch.equal(z.grad, m2)
    # a float32 accumulator is widened, not re-rounded
    assert CR.epilogue_f64(acc.float(), scale.float(), shift.float(), res.float(), 1).dtype == torch.float64


@pytest.mark.parametrize("sizes", [(25, 13), (7, 3), (5, 5), (9, 1), (40, 17), (12, 4), (3, 2), (1, 1), (31, 30)])
def test_nearest_up_f64_matches_interpolate(sizes):
    out, inp = sizes
    top = rnd(7, 2, inp, max(1, inp - 1), 3)
    wo = out + 2
    got = CR.nearest_up_f64(top, out, wo)
    ref = nhwc(F.interpolate(nchw(top), size=(out, wo), mode="nearest"))
    assert torch.equal(got, ref)
    idx = CR.nearest_index(out, inp)
    assert int(idx.max()) == inp - 1 or out < inp
    assert int(idx.min()) == 0 and bool((idx[1:] >= idx[:-1]).all())


def test_nearest_index_is_float32_arithmetic():
    """seam_fpn::nearest_src multiplies in float32; the clamp is what keeps the last index inside for ratios that round up."""
    for out, inp in [(25, 13), (7, 3), (40, 17), (5, 5), (9, 1), (200, 100), (199, 100)]:
        scale = torch.tensor(float(inp), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
        want = [min(int(math.floor(float(torch.tensor(float(d), dtype=torch.float32) * scale))), inp - 1) for d in range(out)]
        assert CR.nearest_index(out, inp).tolist() == want


@pytest.mark.parametrize("case", [(2, 5, 7, 32, 64, 1, 0, 0), (1, 4, 3, 64, 32, 2, 0, 0), (2, 3, 5, 32, 96, 2, 3, 1), (1, 6, 2, 96, 64, 3, 1, 3),
                                  (3, 1, 1, 64, 32, 3, 2, 2)])
def test_dual_f64_matches_two_convs(case):
    n, ho, wo, c1, c2, stride2, eh, ew = case
    h2, w2 = (ho - 1) * stride2 + 1 + eh, (wo - 1) * stride2 + 1 + ew
    x1, x2, wt = rnd(8, n, ho, wo, c1), rnd(9, n, h2, w2, c2), rnd(10, 7, c1 + c2)
    ref = nhwc(F.conv2d(nchw(x1), wt[:, :c1, None, None]) + F.conv2d(nchw(x2), wt[:, c1:, None, None], None, stride2)[:, :, :ho, :wo])
    got = CR.dual_f64(x1, x2, wt, stride2)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("case", [(2, 5, 7, 6, 3), (1, 1, 1, 32, 16), (3, 4, 2, 10, 1)])
def test_conv_transpose_subpixel_f64(case):
    n, h, w, cin, cout = case
    x, wt = rnd(11, n, h, w, cin), rnd(12, cin, cout, 2, 2)
    ref = F.conv_transpose2d(nchw(x), wt, None, 2)
    got = CR.subpixel_to_nchw(CR.conv_transpose2x2_subpixel_f64(x, wt), cout)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


@pytest.mark.parametrize("case", [(2, 7, 9, 5, 6, 3, 1), (1, 6, 6, 12, 3, 3, 0), (2, 5, 8, 4, 7, 1, 0), (1, 9, 7, 3, 4, 5, 2), (2, 4, 4, 6, 5, 2, 1),
                                  (1, 8, 5, 2, 3, 5, 4)])
def test_dgrad_f64_matches_autograd(case):
    n, h, w, cin, cout, R, pad = case
    x = rnd(13, n, cin, h, w).requires_grad_(True)
    wt = rnd(14, cout, cin, R, R)
    y = F.conv2d(x, wt, None, 1, pad)
    dy = rnd(15, *y.shape)
    y.backward(dy)
    got = CR.dgrad_f64(nhwc(dy), wt, pad)
    ref = nhwc(x.grad)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ the kernels' index arithmetic
# (c, R, S, stride, pad, f16): every small C the launchers accept with a fractional number of taps per chunk, the chunked order
# at C = one and three chunks, 7x7 and R != S, the reduction tail (kr >= R inside the last chunk)
MIRROR_SHAPES = [(4, 7, 7, 2, 3, False), (12, 3, 3, 1, 1, False), (20, 1, 3, 1, 0, False), (24, 3, 1, 2, 1, False), (28, 7, 7, 1, 3, False),
                 (12, 2, 3, 1, 1, False), (28, 1, 7, 3, 2, False), (20, 5, 5, 1, 3, False), (32, 3, 3, 1, 1, False), (96, 2, 3, 2, 0, False),
                 (8, 3, 3, 1, 1, True), (24, 7, 7, 2, 3, True), (40, 1, 3, 1, 1, True), (56, 2, 3, 1, 0, True), (56, 7, 1, 1, 3, True),
                 (64, 3, 1, 1, 1, True), (128, 2, 2, 1, 0, True)]


@pytest.mark.parametrize("shape", MIRROR_SHAPES)
def test_igemm_index_mirror_matches_reference(shape):
    """The packed order (seam_pack::igemm_value) and the gather walk (setup() / advance_k()) meet tap for tap: a wrong tap order
    for C < one chunk, or a tail that reads past R, shows here without a GPU."""
    c, R, S, stride, pad, f16 = shape
    bke, epv = (64, 8) if f16 else (32, 4)
    x, wt = rnd(16, 2, 8, 7, c), rnd(17, 5, c, R, S)
    ref = CR.conv_nhwc_f64(x, wt, R, S, stride, pad)
    got = CR.igemm_mirror_f64(x, wt, R, S, stride, pad, bke, epv)
    assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    crop = (max(1, ref.shape[1] - 1), 1)
    got = CR.igemm_mirror_f64(x, wt, R, S, stride, pad, bke, epv, *crop)
    assert float((got - ref[:, :crop[0], :crop[1]]).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_igemm_pack_mirror_modes():
    """Pack modes 1 and 2 in the mirror: the sub-pixel ConvTranspose2d and the input gradient, with Cin below the stored width."""
    x, wt = rnd(18, 2, 4, 5, 12), rnd(19, 10, 3, 2, 2)          # Cin 10 stored as 12
    ref = CR.conv_transpose2x2_subpixel_f64(x[..., :10], wt)
    got = CR.igemm_mirror_f64(x, wt, 1, 1, 1, 0, 32, 4, mode=1, K=12, Cin=10)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    for cout, cstore, R, pad_fwd in [(5, 8, 3, 1), (30, 32, 2, 0), (12, 12, 5, 3)]:
        dy, wt = rnd(20, 2, 6, 5, cstore), rnd(21, cout, 7, R, R)
        ref = CR.dgrad_f64(dy[..., :cout], wt, pad_fwd)
        got = CR.igemm_mirror_f64(dy, wt, R, R, 1, R - 1 - pad_fwd, 32, 4, mode=2, K=7, Cin=cout)
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


# ------------------------------------------------------------------------------------------------ the sweep's cases, on the CPU
@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def cases(lib):
    return {fam: G.generate(fam, lib, G.SEED) for fam in G.FAMILIES}


def test_divfast_grid_is_where_split_row_divides(lib):
    ho, wo = G.DIVFAST_GRID
    assert lib.seam_fastdiv_exact(wo, ho * wo) == 0 and lib.seam_fastdiv_exact(wo, (ho - 1) * wo) == 1
    # ... and no narrower grid of that height has to
    for w in range(1, wo):
        assert lib.seam_fastdiv_exact(w, ho * w) == 1, w


@pytest.mark.parametrize("fam", sorted(G.FAMILIES))
def test_generated_cases_are_accepted_and_reach_the_corners(cases, fam):
    cs = cases[fam]
    assert len(cs) >= G.FAMILIES[fam][1]
    f16 = fam in ("f16", "f16dual")
    for c in cs:
        assert G.accepts(c), G.describe(c)
        assert c["R"] * c["S"] * (c["c"] + c.get("c2", 0)) <= G.MAX_KRED, G.describe(c)
        assert c["k"] in G.K_ALL or fam == "pack", G.describe(c)
        assert (c["R"], c["S"]) in G.RS or fam == "pack", G.describe(c)
        assert c["stride"] in (1, 2, 3) and 0 <= c["pad"] <= 4 and c["h"] + 2 * c["pad"] >= c["R"] and c["w"] + 2 * c["pad"] >= c["S"]
        assert c["bm"] in (64, 128, 256) and c["bn"] in (64, 128) and c["bn"] <= G._slab(c["k"]), G.describe(c)
        if c["force"]:
            assert c["force"] == c["bm"] * 1000 + c["bn"] or (fam == "f16dual" and c["force"] // 1000 == 256), G.describe(c)
        if c["kind"] != "div_fast0":       # every tensor of a case stays small (the over-slots cases need ~70 000 output pixels)
            cap = (10 << 20) if c["kind"] == "over_slots" else (5 << 20)
            assert c["n"] * c["h"] * c["w"] * c["c"] <= cap and c["m"] * c["k"] <= cap, G.describe(c)
            assert c["div_fast"] == 1, G.describe(c)
        else:
            assert (c["ho"], c["wo"]) == G.DIVFAST_GRID and c["div_fast"] == 0 and c["c"] == (8 if f16 else 4)
    counts = G.corner_counts(cs)
    for key, need in G.REQUIRED[fam].items():
        assert counts.get(key, 0) >= need, (fam, key, need, counts)
    assert counts.get("div_fast0", 0) == G.REQUIRED[fam].get("div_fast0", 0), counts
    if "div_fast0" in G.REQUIRED[fam]:
        assert sorted(c["stride"] for c in cs if c["div_fast"] == 0) == [1, 2]


def test_generator_is_deterministic(lib, cases):
    for fam in ("f32", "upres", "pack"):
        again = G.generate(fam, lib, G.SEED)
        assert [G.describe(c) for c in again] == [G.describe(c) for c in cases[fam]]
        assert [c["tseed"] for c in again] == [c["tseed"] for c in cases[fam]]


def test_accepts_is_the_launchers_rule():
    """the refusals of the sweep, in the host rule: each of these is outside it"""
    base = dict(family="f32", n=1, h=8, w=8, c=32, k=64, R=3, S=3, stride=1, pad=1, full=(8, 8), ho=8, wo=8, relu=0, res=False)
    assert G.accepts(base)
    for edit in (dict(c=6), dict(c=36), dict(k=0), dict(full=(0, 8), ho=0), dict(crop=(9, 8)), dict(relu=2), dict(n=0)):
        assert not G.accepts(dict(base, **edit)), edit
    f16 = dict(base, family="f16", c=64, y_f32=0)
    assert G.accepts(f16)
    for edit in (dict(c=4), dict(c=72), dict(crop=(4, 4), res=True)):
        assert not G.accepts(dict(f16, **edit)), edit
    up = dict(base, family="upres", res=True, rh=4, rw=4)
    assert G.accepts(up)
    for edit in (dict(k=6), dict(relu=2), dict(res=False), dict(rh=0)):
        assert not G.accepts(dict(up, **edit)), edit
    du = dict(base, family="dual", R=1, S=1, pad=0, h=5, w=5, full=(5, 5), ho=5, wo=5, c2=64, h2=9, w2=9, stride2=2)
    assert G.accepts(du)
    for edit in (dict(h2=8), dict(w2=8), dict(c2=48), dict(R=3, S=3), dict(c=16)):
        assert not G.accepts(dict(du, **edit)), edit
    assert G.accepts(dict(base, family="sx6", terms=6)) and not G.accepts(dict(base, family="sx6", terms=5))
