"""CPU: the case list of ``w24sx_stress_cases.py`` at the sweep's own arguments (100 cases, seed 6) -- every case served and laid
out by the library with the signature it carries, every class floor met, the budgets kept, the list a pure function of its
arguments, the fp32 plan on the same layout -- and the child's own tools on CPU tensors: ``normal`` against ``synth.normal``,
``reference64`` against ATen's float64 convolutions, ``check`` on a clean result and on five planted faults.  Nothing is launched:
``seam_wino24_layout`` and the predicates are host code."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import stress_child_w24sx as CH
import w24_layout_cases as T
import w24sx_stress_cases as SC

NCASE, SEED = 100, 6


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def query(lib):
    return functools.partial(T.query, lib)


@pytest.fixture(scope="module")
def listed(query):
    return SC.cases(NCASE, SEED, query)


# ------------------------------------------------------------------------------------------------ the case list
def test_every_case_is_served_and_laid_out_as_it_says(lib, query, listed):
    assert len(listed) == NCASE
    for c in listed:
        args = (c["n"], c["h"], c["w"], c["c"], c["k"], c["pad"])
        assert lib.seam_conv3x3_wino24sx_supported(*args, 1) == 1, SC.describe(c)
        lay = query(*args)
        assert lay is not None and SC.layout_pair(lay, *args[:3], c["pad"]) == c["pair"], SC.describe(c)
        assert c["pair"] not in SC.UNREACHABLE and c["tags"] == SC.classify(c, lay)
        assert lay["nt"] == 2 and lay["tiles_n"] == c["k"] // 64 and lay["nsplit"] == 1
        assert lay["grid_blocks"] == SC.grid_blocks(lay, c["k"]) == lib.seam_conv3x3_wino24sx_blocks(*args)
        assert 8 <= c["cin"] <= c["c"] and c["cin"] % 8 == 0 and c["mode"] in (0, 2) and not (c["mode"] == 2 and c["cin"] < c["c"])
        assert c["c"] in SC.CS and c["k"] in SC.KS and c["epilogue"] in SC.EPILOGUES


def test_the_fp32_plan_shares_the_layout(query, listed):
    same = ("nreg", "stack", "G", "PH", "per_img", "TX", "TY", "bx", "by", "patch_blocks")
    for c in listed:
        args = (c["n"], c["h"], c["w"], c["c"], c["k"], c["pad"])
        sx, f32 = query(*args), query(*args, sx=0)
        assert f32 is not None and {k: f32[k] for k in same} == {k: sx[k] for k in same} and f32["nt"] in (1, 2), SC.describe(c)


def test_class_floors(listed):
    counts = SC.count_tags(c["tags"] for c in listed)
    print(dict(sorted(counts.items())))
    for tag, least in SC.REQUIRED.items():
        assert counts.get(tag, 0) >= least, (tag, counts.get(tag, 0), least)


def test_the_floors_are_the_issues():
    r = SC.REQUIRED
    table = {"C>=256": 40, "K>=512": 25, "N>=64": 20, "N>=512": 8, "stacked&patch-blocks>=8": 8, "blocks%8!=0": 20, "blocks<CUs": 20,
             "long-walk": 3, "mask": 8, "Cin<Cstore": 10, "mode2": 6, "pad0": 30, "pad1": 30}
    assert all(r[tag] >= least for tag, least in table.items())
    assert all(r[f"C={c}"] >= 10 for c in (64, 128, 192, 256, 320, 384, 512)) and all(r[f"K={k}"] >= 10 for k in (64, 128, 192, 256, 512, 1024))
    assert all(r[f"epi:{e}"] >= 8 for e in ("none", "shift", "scale_shift", "residual", "relu", "residual_relu", "mask"))
    pairs = {(cls, hs) for cls in SC.LAYOUTS for hs in SC.HS_CLASSES}
    assert len(pairs) == 28 and SC.UNREACHABLE < pairs
    assert all(r[SC.pair_tag(p)] >= 3 for p in pairs - SC.UNREACHABLE) and not any(SC.pair_tag(p) in r for p in SC.UNREACHABLE)


def test_unreachable_is_exactly_what_the_scan_shows_empty(query):
    pool = SC.scan(query)
    assert sum(len(v) for v in pool.values()) == len(SC.SCAN["images"]) * SC.SCAN["tiles_x"] * SC.SCAN["tiles_y"]
    pairs = {(cls, hs) for cls in SC.LAYOUTS for hs in SC.HS_CLASSES}
    assert pairs - set(pool) == SC.UNREACHABLE, sorted(pairs - set(pool), key=str)


def test_budgets(listed):
    walks = [c for c in listed if c["long"]]
    assert [c["index"] for c in walks] == [16, 32, 49, 65, 82, 98]
    assert sum("long-walk" in c["tags"] for c in walks) == 3 and sum("CUs<blocks<2CUs" in c["tags"] for c in walks) == 3
    for c in listed:
        worst = max(SC.operand_bytes(c).values())
        assert worst <= (SC.LONG_BUDGET if c["long"] else SC.BUDGET), (SC.describe(c), worst)
        assert 1 <= c["n"] <= SC.N_MAX
        if c["long"]:
            assert c["c"] <= 128, SC.describe(c)


def test_the_list_is_a_pure_function_of_its_arguments(query, listed):
    assert SC.cases(NCASE, SEED, query) == listed
    assert SC.cases(NCASE, SEED + 1, query) != listed
    assert SC.cases(10, SEED, query) == listed[:10]
    assert len({c["data_seed"] for c in listed}) == NCASE


def test_classify_recounts_with_the_cu_count(query, listed):
    c = next(c for c in listed if "CUs<blocks<2CUs" in c["tags"])
    lay = query(c["n"], c["h"], c["w"], c["c"], c["k"], c["pad"])
    blocks = SC.grid_blocks(lay, c["k"])
    assert "blocks<CUs" in SC.classify(c, lay, cus=blocks + 1) and "CUs<blocks<2CUs" not in SC.classify(c, lay, cus=blocks + 1)


def test_edges_cross_the_layout_classes(listed):
    """the schedules are coprime: every layout class meets both paddings, several channel counts and epilogues"""
    for cls in set(p[0] for p in (c["pair"] for c in listed)):
        mine = [c for c in listed if c["pair"][0] == cls]
        assert {c["pad"] for c in mine} == {0, 1} and len({c["c"] for c in mine}) >= 4 and len({c["k"] for c in mine}) >= 4, cls
        assert len({c["epilogue"] for c in mine}) >= 5, cls
    lengths = (28, len(SC.SIZES), len(SC.CS), len(SC.KS), len(SC.PADS), len(SC.EDGES), len(SC.EPI_SCHEDULE), SC.PACKS)
    assert all(math.gcd(a, b) == 1 for i, a in enumerate(lengths) for b in lengths[i + 1:]), lengths


def test_a_forced_split_leaves_a_ragged_partition(lib, query, listed):
    """among the cases the child runs under forced splits, some patch-block count is no multiple of the partition count"""
    forced = [c for c in listed if c["k"] >= 256 and c["index"] % 5 == 0]
    assert len(forced) >= 5
    before = lib.seam_conv3x3_wino24sx_get_nsplit()
    ragged, seen = 0, set()
    try:
        for ns in CH.FORCED:
            assert lib.seam_conv3x3_wino24sx_set_nsplit(ns) == 0
            for c in forced:
                lay = query(c["n"], c["h"], c["w"], c["c"], c["k"], c["pad"])
                assert lay is not None and lay["nsplit"] == min(ns, c["k"] // 64), (ns, SC.describe(c))
                seen.add(lay["nsplit"])
                parts = 8 // lay["nsplit"]
                ragged += lay["patch_blocks"] % parts != 0
                assert lay["grid_blocks"] == 8 * -(-lay["patch_blocks"] // parts) * (lay["tiles_n"] // lay["nsplit"])
    finally:
        lib.seam_conv3x3_wino24sx_set_nsplit(before)
    assert ragged >= 1 and seen == {2, 4, 8}
    assert lib.seam_conv3x3_wino24sx_get_nsplit() == before


def test_the_refusals_are_refused_on_the_host(lib, query):
    for name, change in CH.REFUSED_LAUNCHES:
        a = dict(n=1, h=8, w=8, c=64, k=64, pad=1, stride=1)
        assert lib.seam_conv3x3_wino24sx_supported(*(a[key] for key in ("n", "h", "w", "c", "k", "pad", "stride"))) == 1
        a.update(change)
        assert lib.seam_conv3x3_wino24sx_supported(*(a[key] for key in ("n", "h", "w", "c", "k", "pad", "stride"))) == 0, name
    for name, change in CH.REFUSED_LAUNCHES_F32:        # the fp32 entry's own contract, read from its plan
        a = dict(n=1, h=8, w=8, c=64, k=64, pad=1)
        assert query(*a.values(), sx=0) is not None
        a.update(change)
        assert query(*a.values(), sx=0) is None, name
    (_, big), (_, many) = CH.REFUSED_PREDICATES
    assert 4 * big[1] * big[2] * big[3] >= 1 << 31 and big[3] % 64 == 0 and 144 * big[3] * big[4] < 1 << 31
    assert lib.seam_conv3x3_wino24sx_supported(*big, 1) == 0 and query(*big) is None
    assert lib.seam_conv3x3_wino24sx_supported(*many, 1) == 0 and query(*many) is None
    fewer = (many[0] // 2,) + many[1:]                  # ... for its block count alone: half the batch is served
    assert lib.seam_conv3x3_wino24sx_supported(*fewer, 1) == 1
    assert (1 << 23) <= query(*fewer)["grid_blocks"] < (1 << 24)


# ------------------------------------------------------------------------------------------------ the child's tools, on the CPU
@pytest.mark.parametrize("shape", [(3, 5, 7), ((1 << 22) + 17,)], ids=["small", "two-chunks"])
def test_normal_is_synth_normal(shape):
    import seam_match_rcnn_amd.synth as synth
    stream = synth.stream_id(123456789, "x")
    assert torch.equal(CH.normal(stream, shape, "cpu"), torch.from_numpy(synth.normal(stream, shape)))


REFERENCE_CASES = [  # (n, h, w, c, cin, k, pad, mode, epilogue)
    (1, 5, 6, 8, 8, 4, 1, 0, "none"), (2, 5, 6, 8, 8, 4, 0, 0, "shift"), (2, 4, 7, 16, 16, 8, 1, 0, "scale_shift"),
    (1, 6, 5, 16, 8, 8, 0, 0, "residual"), (3, 3, 3, 8, 8, 8, 1, 0, "relu"), (2, 7, 4, 8, 8, 12, 1, 0, "residual_relu"),
    (2, 5, 5, 8, 8, 4, 1, 0, "mask"), (2, 5, 6, 8, 8, 4, 1, 2, "none"), (1, 6, 6, 8, 8, 12, 0, 2, "residual_relu"),
    (2, 4, 9, 16, 16, 8, 0, 2, "mask"), (2, 5, 4, 24, 8, 8, 1, 0, "mask"), (1, 3, 8, 24, 16, 4, 0, 0, "scale_shift")]


@pytest.mark.parametrize("case", REFERENCE_CASES, ids=[f"{c[7]}-pad{c[6]}-cin{c[4]}of{c[3]}-{c[8]}" for c in REFERENCE_CASES])
def test_reference64_is_atens_float64_convolution(case):
    n, h, w, c, cin, k, pad, mode, epi = case
    g = torch.Generator().manual_seed(REFERENCE_CASES.index(case))
    x = torch.randn((n, h, w, c), generator=g)
    x[..., cin:] = float("nan")                         # the reference reads the first Cin channels only
    wt = torch.randn((k, cin, 3, 3) if mode == 0 else (cin, k, 3, 3), generator=g)
    has_scale, has_shift, has_res, relu = SC.EPI_FLAGS[epi]
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    scale = torch.rand(k, generator=g) + 0.5 if has_scale else None
    shift = torch.randn(k, generator=g) if has_shift else None
    res = torch.randn((n, ho, wo, k), generator=g) if has_res else None
    if relu == 2:
        res[res.abs() < 0.3] = 0.0
    got = CH.reference64(x, wt, pad, mode, scale, shift, res, relu)
    xn = x[..., :cin].permute(0, 3, 1, 2).double()
    want = F.conv2d(xn, wt.double(), None, 1, pad) if mode == 0 else F.conv_transpose2d(xn, wt.double(), None, 1, 2 - pad)
    want = want.permute(0, 2, 3, 1)
    if has_scale:
        want = want * scale.double()
    if has_shift:
        want = want + shift.double()
    if relu == 2:
        want = want * (res > 0)
    elif has_res:
        want = want + res.double()
    if relu == 1:
        want = F.relu(want)
    assert got.dtype == torch.float64 and got.shape == (n, ho, wo, k)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_the_reference_cases_cover_what_they_must():
    assert len(REFERENCE_CASES) >= 12 and {c[6] for c in REFERENCE_CASES} == {0, 1} and {c[7] for c in REFERENCE_CASES} == {0, 2}
    assert {c[8] for c in REFERENCE_CASES} == set(SC.EPILOGUES) and sum(c[4] < c[3] for c in REFERENCE_CASES) >= 2


@pytest.fixture(scope="module")
def clean():
    """a mask-epilogue case of the child's own operands on the CPU, its float64 reference and a correct fp32 result"""
    c = {"n": 3, "h": 9, "w": 11, "c": 64, "k": 64, "pad": 1, "cin": 64, "mode": 0, "epilogue": "mask", "data_seed": 77, "index": 0}
    o = CH.operands(c, "cpu")
    y64 = CH.reference64(o["x"], o["w"], 1, 0, o["scale"], o["shift"], o["res"], o["relu"])

    def fp32(x, w, as_add=False):
        v = F.conv2d(x.permute(0, 3, 1, 2), w, None, 1, 1).permute(0, 2, 3, 1) * o["scale"] + o["shift"]
        return (v + o["res"] if as_add else torch.where(o["res"] > 0, v, torch.zeros_like(v))).contiguous()
    return o, y64, fp32


def test_check_accepts_a_correct_fp32_result(clean):
    o, y64, fp32 = clean
    y = fp32(o["x"], o["w"])
    assert bool((o["res"] == 0).any()) and bool((o["res"] < 0).any()) and bool((o["res"] > 0).any())
    why, f = CH.check("clean", y, y64, y, y)
    assert why == [] and f["e_new"] <= 1e-5 and f["d_ex"] == 0.0
    assert CH.check_f32(y, y64) == []


FAULTS = ("shifted-one-pixel-in-x", "two-images-swapped", "last-16-channels-left-out", "mask-applied-as-an-add", "one-row-left-at-its-poison-nan",
          "one-row-left-at-its-poison-3e4")


@pytest.mark.parametrize("fault", FAULTS)
def test_check_catches_a_planted_fault(clean, fault):
    o, y64, fp32 = clean
    good = fp32(o["x"], o["w"])
    if fault == "shifted-one-pixel-in-x":
        bad = torch.roll(good, 1, dims=2)
    elif fault == "two-images-swapped":
        bad = good[[1, 0, 2]].contiguous()
    elif fault == "last-16-channels-left-out":
        bad = fp32(o["x"][..., :48].contiguous(), o["w"][:, :48].contiguous())
    elif fault == "mask-applied-as-an-add":
        bad = fp32(o["x"], o["w"], as_add=True)
    else:
        bad = good.clone()
        bad[1, 4] = stress_poison(fault)
    assert not torch.equal(bad, good)
    why, _ = CH.check(fault, bad, y64, good, good)
    assert why, fault
    assert CH.check_f32(bad, y64), fault                # ... and the fp32 family's gate sees it as well


def stress_poison(fault):
    import stress_kit
    return stress_kit.POISON_FLOAT[0 if fault.endswith("nan") else 1]
