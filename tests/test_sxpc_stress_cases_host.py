"""CPU: the case lists of ``sxpc_stress_cases.py`` at the sweep's own arguments (100 cases, seed 6) -- every case served by the
library's predicates, every class minimum met, the byte budgets kept, the list a pure function of its arguments.  Nothing is
launched: the predicates and the geometry rules are host code."""
import pytest

import sxpc_stress_cases as SC

NCASE, SEED = 100, 6


def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


@pytest.fixture(scope="module", params=SC.FAMILIES)
def listed(request):
    return request.param, SC.cases(request.param, NCASE, SEED)


def served(l, family, c):
    """the entry's own ``*_supported`` predicate and, where the launch checks more than the predicate, that rule"""
    from seam_match_rcnn_amd import ops
    m, k = c["M"], c["K"]
    if family == "sxpc":
        return l.seam_conv1x1_sxpc_supported(m, c["C"], k) == 1
    if family == "sxpc_short":
        return l.seam_conv1x1_sxpc_short_supported(m, c["C"], k) == 1
    if family == "sxpc64":
        return l.seam_conv1x1_sxpc64_supported(m, c["C"], k) == 1
    if family == "stem_sxpc":
        return l.seam_stem_sxpc_supported(c["N"], c["Ho"], c["Wo"]) == 1 and (c["C"], k) == (192, 64)
    if family == "sxpc_up":
        return l.seam_conv1x1_sxpc_up_supported(m, c["N"], c["Ho"], c["Wo"], c["C"], k, c["rH"], c["rW"]) == 1
    # the two-source forms: the predicate decides the channel counts and M, the launch the geometry -- (Ho - 1) s < H2 and the
    # same for W (the documented rule), the images of one tile inside a descriptor and the exact division by Wo (its Python twin)
    pred = l.seam_conv1x1_sxpc_dual_supported if family == "sxpc_dual" else l.seam_conv1x1_sxpc_dual_short_supported
    s = c["stride2"]
    return (pred(m, c["C1"], c["C2"], k) == 1 and c["C1"] + c["C2"] == c["C"] and s >= 1 and (family == "sxpc_dual" or s == 1)
            and (c["Ho"] - 1) * s < c["H2"] and (c["Wo"] - 1) * s < c["W2"]
            and ops._sxpc_dual_map_ok(c["N"], c["Ho"], c["Wo"], c["H2"], c["W2"], c["C2"]))


def test_every_case_is_served(listed):
    family, cs = listed
    l = lib()
    assert len(cs) == NCASE
    for c in cs:
        assert served(l, family, c), SC.describe(c)
        assert c["nchunks"] * SC.CK == c["C"] and c["M"] >= 1
        if family in SC.SECOND:
            assert c["M"] == c["N"] * c["Ho"] * c["Wo"], SC.describe(c)


def test_channel_counts_are_the_plans(listed):
    family, cs = listed
    for c in cs:
        if family in ("sxpc", "sxpc_up", "sxpc_dual"):
            assert c["C"] in SC.C_LONG and c["K"] in SC.K_LONG
        elif family in ("sxpc_short", "sxpc_dual_short"):
            assert c["C"] == 128 and c["K"] in SC.K_LONG
        elif family == "sxpc64":
            assert c["C"] in SC.C_64 and c["K"] == 64
        if family == "sxpc_dual":
            assert c["C1"] % 64 == 0 and c["C2"] % 64 == 0 and 1 <= c["C1"] // 64 <= c["nchunks"] - 1
        if family == "sxpc_dual_short":
            assert (c["C1"], c["C2"]) == (64, 64)
    if family in ("sxpc", "sxpc_up", "sxpc_dual"):
        assert {c["C"] for c in cs} == set(SC.C_LONG) and {c["K"] for c in cs} == set(SC.K_LONG)
    if family == "sxpc_dual":                   # the switch between the sources at the first, at the last and at inner chunks
        assert {1} < {c["C1"] // 64 for c in cs} and any(c["C2"] == 64 for c in cs)
    if family == "sxpc64":
        assert {c["C"] for c in cs} == set(SC.C_64)


def test_class_minimums(listed):
    family, cs = listed
    for c in cs:
        assert c["tags"] == SC.classify(family, c)
    counts = SC.count_tags(c["tags"] for c in cs)
    print(family, dict(sorted(counts.items())))
    for tag, least in SC.REQUIRED[family].items():
        assert counts.get(tag, 0) >= least, (family, tag, counts.get(tag, 0), least)


def test_the_issues_minimums_are_in_required():
    for family in SC.FAMILIES:
        r = SC.REQUIRED[family]
        assert r["tiles>3CUs&tiles%CUs!=0"] >= 3
        for tag in ("M<128", "M%128==0", "M%128in{1,127}", "M==1", "tiles<=8", "tiles<CUs&tiles%8!=0", "epi-none", "epi-shift",
                    "epi-scale+shift", "relu0", "relu1"):
            assert r[tag] >= 1, (family, tag)
        if family in SC.SECOND:
            assert all(r[tag] >= 10 for tag in SC.T_SECOND[:4]) and all(r[tag] >= 1 for tag in SC.T_SECOND[4:])
        if family in SC.RESIDUAL:
            assert r["res"] >= 1
    assert all(SC.REQUIRED["sxpc_dual"][t] >= 1 for t in ("stride2==1", "stride2==2", "stride2==3", "x2-min", "x2-slack"))
    assert all(SC.REQUIRED["sxpc_up"][t] >= 1 for t in ("ratio2", "ratio-frac", "ratio1", "coarse>out", "rH==1|rW==1"))
    assert all(SC.REQUIRED[f]["nchunks-odd"] >= 1 and SC.REQUIRED[f]["nchunks-even"] >= 1 for f in ("sxpc", "sxpc_dual", "sxpc_up"))
    assert all(SC.REQUIRED[f]["nchunks==2"] >= 1 for f in ("sxpc_short", "sxpc_dual_short", "sxpc64"))
    assert SC.REQUIRED["stem_sxpc"]["nchunks==3"] >= 1


def test_byte_budgets(listed):
    family, cs = listed
    walks = [c for c in cs if c["long"]]
    assert len(walks) <= 6                       # a handful
    for c in cs:
        worst = max(SC.operand_bytes(family, c).values())
        assert worst <= (SC.LONG_BUDGET if c["long"] else SC.BUDGET), (SC.describe(c), worst)
        assert c["M"] <= SC.m_limit(family, c), SC.describe(c)
        if c["long"]:                            # the smallest channel counts
            assert c["C"] == {"sxpc": 256, "sxpc_up": 256, "sxpc_dual": 256, "sxpc64": 128, "stem_sxpc": 192}.get(family, 128)
    over = [c for c in cs if c["M"] > SC.M_MAX]
    assert (len(over) == 3 and all("tiles>3CUs&tiles%CUs!=0" in c["tags"] for c in over)) if family in ("sxpc64", "stem_sxpc") else not over


def test_the_list_is_a_pure_function_of_its_arguments(listed):
    family, cs = listed
    assert SC.cases(family, NCASE, SEED) == cs
    assert SC.cases(family, NCASE, SEED + 1) != cs
    assert SC.cases(family, 10, SEED) == cs[:10]                 # a shorter list is a prefix: a family can be cut without moving its cases
    assert len({c["data_seed"] for c in cs}) == NCASE


def test_classify_recounts_with_the_cu_count():
    c = dict(SC.cases("sxpc", 1, SEED)[0], M=128 * 300, K=128)
    assert "CUs<tiles<2CUs" in SC.classify("sxpc", c) and "CUs<tiles<2CUs" not in SC.classify("sxpc", c, cus=304)
    assert "tiles<CUs&tiles%8!=0" in SC.classify("sxpc", c, cus=304)
