"""CPU: every case of tests/w24_layout_cases.py against the layout the library reports for it (``seam_wino24_layout``, sx = 1: the
very arguments ``seam_conv3x3_wino24sx_f32`` would launch with), and the coverage the table promises -- before anything is launched.
Run with -s to see, per case, the signature the library reported."""
import pytest

import w24_layout_cases as T

# what below 110 x 110 outputs and eight images no layout has: a bottom strip of the HS = 3 class.  A bottom strip is as wide as
# the main region: best_uniform gives one wider than two tiles a wider patch than TX = 2, and under a main region one or two tiles
# wide a strip saves no block over the uniform layout, so none is made.  The search below shows it for every grid in the bound.
UNREACHABLE = {("bottom", 3)}
SEARCH = dict(ho=110, wo=110, images=(1, 8))


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def sigs(lib):
    out = {}
    for c in T.CASES:
        lay = T.query(lib, c.n, c.h, c.w, c.c, c.k, c.pad)
        assert lay is not None, c
        out[c.id] = T.signature(lay, c.n, c.h, c.w, c.pad)
    return out


def test_ids_are_unique_and_the_table_is_small():
    assert len(T.BY_ID) == len(T.CASES) <= 60
    for c in T.CASES:
        assert 1 <= c.n <= 8 and c.h * c.w <= 12000 and c.pad in (0, 1) and c.epilogue in T.EPILOGUES, c
        assert c.c % 64 == 0 and c.k % 64 == 0, c


@pytest.mark.parametrize("case", T.CASES, ids=[c.id for c in T.CASES])
def test_case_reaches_its_layout(lib, sigs, case):
    sig = sigs[case.id]
    print(f"\n{case.id}: {case.n} x {case.h} x {case.w}, {case.c} -> {case.k}, pad {case.pad}: {T.describe(sig)}")
    assert T.meets(sig, case.expect), (case.expect, T.describe(sig))
    lay = T.query(lib, case.n, case.h, case.w, case.c, case.k, case.pad)
    assert lay["nt"] == 2 and lay["tiles_n"] == case.k // 64 and lay["nsplit"] == 1
    assert lay["grid_blocks"] == lay["patch_blocks"] * lay["tiles_n"] == lib.seam_conv3x3_wino24sx_blocks(case.n, case.h, case.w, case.c, case.k, case.pad)
    # the fp32 kernels the sweep runs on the same inputs share the layout; only the n-tiles per block differ
    f32 = T.query(lib, case.n, case.h, case.w, case.c, case.k, case.pad, sx=0)
    same = ("nreg", "stack", "G", "PH", "per_img", "TX", "TY", "bx", "by", "patch_blocks")
    assert {k: f32[k] for k in same} == {k: lay[k] for k in same} and f32["nt"] in (1, 2)
    # the layout depends on the output grid alone: the other padding with the same grid gives the same one
    other = T.query(lib, case.n, case.h + 4 * case.pad - 2, case.w + 4 * case.pad - 2, case.c, case.k, 1 - case.pad)
    assert {k: other[k] for k in same} == {k: lay[k] for k in same}


def test_every_hs_class_in_every_position(lib, sigs):
    seen = {(kd, hs) for s in sigs.values() for kd, hs in zip(s["kinds"], s["hs"])}
    want = {(kd, hs) for kd in ("one", "main", "right", "bottom", "stack") for hs in (9, 5, 3, T.RT)}
    assert want - seen == UNREACHABLE, sorted(want - seen)
    # ... and the missing one is missing from every grid inside the search bound, whatever the batch (one query per tile grid)
    assert len(UNREACHABLE) <= 1
    for n in SEARCH["images"]:
        for ho in range(1, SEARCH["ho"] + 1, 2):
            for wo in range(1, SEARCH["wo"] + 1, 4):
                s = T.signature(T.query(lib, n, ho, wo, 64, 64, 1), n, ho, wo, 1)
                assert not (set(zip(s["kinds"], s["hs"])) & UNREACHABLE), (n, ho, wo, T.describe(s))


def test_production_signatures(lib, sigs):
    """The two layouts the product runs: 100 x 100 and 200 x 200 maps, as the library lays them out today."""
    s100 = T.signature(T.query(lib, 1, 100, 100, 128, 128, 1), 1, 100, 100, 1)
    s200 = T.signature(T.query(lib, 1, 200, 200, 256, 256, 1), 1, 200, 200, 1)
    assert (s100["hs"], s100["strips"], s100["TX"], s100["TY"]) == ((9, 3, T.RT), "RB", (8, 1, 12), (4, 25, 2))
    assert (s200["hs"], s200["strips"], s200["TX"], s200["TY"]) == ((9, 3), "R", (8, 2), (4, 15))
    for prod, tag in ((s100, "100sq"), (s200, "200sq")):
        mine = [sigs[c.id] for c in T.CASES if tag in c.id]
        assert len(mine) == 4 and all((m["hs"], m["strips"], m["stack"]) == (prod["hs"], prod["strips"], 0) for m in mine)


def test_edges_paddings_and_widths(sigs):
    multi = [c for c in T.CASES if sigs[c.id]["nreg"] > 1]
    assert {sigs[c.id]["wo"] % 4 for c in multi} == {0, 1, 2, 3}
    assert 2 * sum(sigs[c.id]["ho"] % 2 for c in multi) >= len(multi)
    assert 3 * sum(c.pad == 0 for c in T.CASES) >= len(T.CASES)
    # every signature at C = 64; the production ones and two stacked ones also at C = 128 and C = 192
    key = lambda c: (sigs[c.id]["stack"], sigs[c.id]["hs"], sigs[c.id]["strips"])
    assert {key(c) for c in T.CASES} == {key(c) for c in T.CASES if c.c == 64}
    for cc in (128, 192):
        at = [key(c) for c in T.CASES if c.c == cc]
        assert (0, (9, 3, T.RT), "RB") in at and (0, (9, 3), "R") in at and len({k for k in at if k[0] == 1}) >= 2, (cc, at)
    for kk in (64, 128, 192):
        assert sum(c.k == kk for c in multi) >= 3, kk
    for mode in T.EPILOGUES[1:]:
        assert [c for c in multi if c.epilogue == mode] and [c for c in T.CASES if sigs[c.id]["stack"] and c.epilogue == mode], mode
    nsplit = [c for c in T.CASES if c.role == "nsplit"]
    assert sorted(sigs[c.id]["hs"] for c in nsplit) == [(9, 3), (9, 3, T.RT)] and all(c.k == 256 for c in nsplit)


def test_every_stacked_case_has_a_many_image_sibling(lib, sigs):
    stacked = [c for c in T.CASES if sigs[c.id]["stack"] and not c.role and c.c == 64]
    assert len(stacked) >= 6 and {sigs[c.id]["hs"][0] for c in stacked} == {9, 5, 3, T.RT}
    assert max(sigs[c.id]["G"] for c in stacked) > 3
    for c in T.CASES:
        assert bool(sigs[c.id]["stack"]) == c.id.startswith("st-"), c.id
    for c in stacked:
        sib = [s for s in T.CASES if s.role == "sibling:" + c.id]
        assert len(sib) == 1, c.id
        s = sib[0]
        assert (s.h, s.w, s.c, s.k, s.pad) == (c.h, c.w, c.c, c.k, c.pad) and s.n > c.n
        g = sigs[s.id]
        assert g["stack"] == 1 and g["patch_blocks"] >= 2 and (s.n * g["tiles"][1]) % g["TY"][0] != 0, T.describe(g)
        # one image alone is laid out differently, so "image alone == image in the batch" compares two layouts
        for b in (c, s):
            alone = T.query(lib, 1, b.h, b.w, b.c, b.k, b.pad)
            assert alone["stack"] == 0 and (alone["TX"], alone["TY"]) != (sigs[b.id]["TX"] + (0, 0), sigs[b.id]["TY"] + (0, 0))


def test_query_refuses_what_the_launcher_refuses(lib):
    for args in ((1, 8, 8, 96, 64, 1), (1, 8, 8, 64, 32, 1), (0, 8, 8, 64, 64, 1), (1, 2, 2, 64, 64, 0), (1, 8, 8, 64, 64, 2)):
        assert T.query(lib, *args) is None and lib.seam_conv3x3_wino24sx_supported(*args, 1) == 0, args
    assert T.query(lib, 1, 8, 8, 8, 32, 1, sx=0) is not None and T.query(lib, 1, 8, 8, 7, 32, 1, sx=0) is None
    assert T.query(lib, 1, 8, 8, 64, 64, 1, sx=2) is None
