"""The fixed case table of the F(2x4) Winograd layout sweep (tests/test_gpu_w24sx_layouts.py), and the host helpers that read a
launch's block layout from the library (``seam_wino24_layout``, csrc/seam_wino24sx.hip).  Pure Python: no torch, no device.

How a launch of ``conv3x3_wino24sx`` / ``conv3x3_wino24<NT>`` is laid out is decided by ``choose_layout``
(csrc/seam_wino_layout.h, form F24) from the output grid alone: tiles_x = ceil(Wo / 4), tiles_y = ceil(Ho / 2) and, for the stacked form,
the batch.  ``w24_tile`` then picks one of four instantiations of ``w24_block`` per region from HS = (TX + 1) | 1: 9, 5, 3 or the
run-time form (``RT`` below).  Every case names the layout it exists for in ``expect``; tests/test_w24_layout_cases_host.py asks
the library for each case's layout and fails where a case does not reach its branch, before anything is launched.

Shapes are written by their OUTPUT grid (Ho, Wo) and the padding, the input is H = Ho + 2 - 2 pad: the same grid with pad 0 and
pad 1 gives the same layout and different halo handling.  They are the smallest grids that give each signature (found with the
query over all grids below 110 x 110), moved within their tile count so that Wo % 4 takes every value and Ho is odd and even.

Stacked cases: a 3 x 3 map (tiles 1 x 2) stacks 17 tile rows per block, more than the 16 rows of eight images, so the many-image
form of the G > 3 case is a 5 x 3 map (19 rows per block, seven images per patch; seven images are 21 rows, two blocks)."""
import collections
import ctypes

RT = 0          # HS class of the run-time form (TX 5, 6 or > 8)
EPILOGUES = ("", "scale_shift", "residual", "relu", "residual_relu")

Case = collections.namedtuple("Case", "id n h w c k pad epilogue expect role")


def _case(cid, n, ho, wo, pad, hs, c=64, k=64, epi="", stack=0, g_min=1, ragged=False, strips="", role=""):
    """ragged: non-stacked -- some region's last block is partly filled; stacked -- the last block is (N * tiles_y % TY != 0).
    strips: which strips follow the main region ("R" right, "B" bottom).  role: "" | "sibling:<id of the stacked case>" | "nsplit"."""
    expect = dict(stack=stack, nreg=len(hs), hs=tuple(hs), g_min=g_min, ragged=ragged, strips=strips)
    return Case(cid, n, ho + 2 - 2 * pad, wo + 2 - 2 * pad, c, k, pad, epi, expect, role)


CASES = [
    # ---- one region, not stacked: each instantiation alone in a block
    _case("one-hs3", 1, 3, 3, 0, (3,), ragged=False),
    _case("one-hs5", 1, 3, 10, 1, (5,)),
    _case("one-rt-tx5", 1, 4, 19, 0, (RT,)),
    _case("one-hs9", 1, 3, 27, 1, (9,)),
    # ... and with a partly filled last block (the region is no multiple of the patch)
    _case("one-hs3-ragged-1col", 1, 53, 1, 1, (3,), ragged=True),                              # one output column
    _case("one-hs5-ragged", 1, 9, 25, 0, (5,), ragged=True),
    _case("one-rt-ragged", 1, 13, 17, 1, (RT,), ragged=True),
    _case("one-hs9-ragged", 1, 19, 26, 0, (9,), ragged=True),
    # ---- main region + one strip
    _case("r2-9-3r-200sq", 1, 47, 33, 1, (9, 3), strips="R"),                                  # the 200 x 200 layout
    _case("r2-9-3r-200sq-c128", 1, 47, 34, 0, (9, 3), c=128, k=128, strips="R"),
    _case("r2-9-3r-200sq-c192", 1, 48, 35, 1, (9, 3), c=192, k=192, epi="residual_relu", strips="R"),
    _case("r2-9-3r-200sq-k256", 1, 47, 36, 1, (9, 3), k=256, strips="R", role="nsplit"),
    _case("r2-9-3r-ragged", 1, 79, 37, 1, (9, 3), strips="R", ragged=True),                     # ... with its partly filled last strip block
    _case("r2-rt-3r", 1, 23, 42, 1, (RT, 3), epi="scale_shift", strips="R"),
    _case("r2-3-rtb", 1, 41, 23, 0, (3, RT), k=128, strips="B"),
    _case("r2-9-rtr", 1, 23, 52, 1, (9, RT), k=192, strips="R"),
    _case("r2-rt-9b", 1, 17, 93, 0, (RT, 9), strips="B"),
    _case("r2-9-5r", 1, 39, 41, 1, (9, 5), epi="relu", strips="R"),
    _case("r2-3-5b", 1, 52, 22, 0, (3, 5), strips="B"),
    _case("r2-5-rtb", 1, 25, 35, 1, (5, RT), strips="B"),
    _case("r2-rt-9r", 1, 23, 71, 0, (RT, 9), k=128, strips="R"),
    # ---- main region + right strip + bottom strip
    _case("r3-9-3-rt-100sq", 1, 25, 69, 1, (9, 3, RT), strips="RB"),                            # the 100 x 100 layout
    _case("r3-9-3-rt-100sq-c128", 1, 25, 70, 1, (9, 3, RT), c=128, k=128, strips="RB"),
    _case("r3-9-3-rt-100sq-c192", 1, 26, 71, 0, (9, 3, RT), c=192, k=192, strips="RB"),
    _case("r3-9-3-rt-100sq-k256", 1, 25, 72, 0, (9, 3, RT), k=256, strips="RB", role="nsplit"),
    _case("r3-9-3-9", 1, 43, 33, 1, (9, 3, 9), epi="residual", strips="RB"),
    _case("r3-9-rt-9", 1, 21, 50, 0, (9, RT, 9), k=128, strips="RB", ragged=True),
    _case("r3-9-5-9", 1, 38, 43, 1, (9, 5, 9), strips="RB", ragged=True),
    _case("r3-rt-5-9", 1, 17, 105, 1, (RT, 5, 9), k=192, strips="RB"),
    _case("r3-3-3-rt", 1, 41, 27, 0, (3, 3, RT), strips="RB"),
    _case("r3-rt-3-rt-ragged", 1, 57, 25, 1, (RT, 3, RT), strips="RB", ragged=True),
    _case("r3-rt-9-rt-ragged", 1, 21, 69, 0, (RT, 9, RT), strips="RB", ragged=True),
    # ---- stacked: TY consecutive tile rows of the whole batch per block; each with its many-image sibling
    _case("st-hs3-g7", 2, 5, 3, 1, (3,), stack=1, g_min=4, ragged=True, epi="scale_shift"),       # the patch reaches past the batch
    _case("st-hs3-g7-many", 7, 5, 3, 1, (3,), stack=1, g_min=4, ragged=True, role="sibling:st-hs3-g7"),
    _case("st-hs3-ty24", 2, 23, 3, 1, (3,), stack=1, g_min=2),
    _case("st-hs3-ty24-many", 3, 23, 3, 1, (3,), stack=1, g_min=2, ragged=True, role="sibling:st-hs3-ty24"),
    _case("st-rt-g3", 2, 3, 17, 0, (RT,), stack=1, g_min=3, ragged=True, epi="residual"),
    _case("st-rt-g3-many", 3, 3, 17, 0, (RT,), stack=1, g_min=3, ragged=True, role="sibling:st-rt-g3"),
    _case("st-rt-g3-c128", 2, 3, 18, 1, (RT,), c=128, stack=1, g_min=3, ragged=True),
    _case("st-rt-g3-c192", 2, 4, 19, 0, (RT,), c=192, stack=1, g_min=3, ragged=True),
    _case("st-rt-g2", 2, 3, 21, 1, (RT,), stack=1, g_min=2, epi="relu"),
    _case("st-rt-g2-many", 3, 3, 21, 1, (RT,), stack=1, g_min=2, ragged=True, role="sibling:st-rt-g2"),
    _case("st-hs9-ho1", 2, 1, 25, 0, (9,), stack=1, g_min=3, ragged=True),                          # one half-filled tile row
    _case("st-hs9-ho1-many", 4, 1, 25, 0, (9,), stack=1, g_min=3, ragged=True, role="sibling:st-hs9-ho1"),
    _case("st-hs5", 2, 9, 9, 1, (5,), stack=1, g_min=2, epi="residual_relu"),
    _case("st-hs5-many", 3, 9, 9, 1, (5,), stack=1, g_min=2, ragged=True, role="sibling:st-hs5"),
    _case("st-hs5-c128", 2, 9, 11, 0, (5,), c=128, stack=1, g_min=2),
    _case("st-hs5-c192", 2, 10, 12, 0, (5,), c=192, stack=1, g_min=2),
]

BY_ID = {c.id: c for c in CASES}

_HEAD = ("nreg", "stack", "G", "PH", "nt", "tiles_n", "nsplit", "per_img")


def hs_class(tx):
    hs = (tx + 1) | 1
    return hs if hs in (3, 5, 9) else RT


def query(lib, n, h, w, c, k, pad, sx=1):
    """seam_wino24_layout as a dict, or None where the launcher refuses the shape (and then nothing may have been written)."""
    out = (ctypes.c_int * 24)(*([-7] * 24))
    if lib.seam_wino24_layout(n, h, w, c, k, pad, sx, out) != 0:
        assert all(v == -7 for v in out), "a refused shape wrote into the output array"
        return None
    o = list(out)
    lay = dict(zip(_HEAD, o[:8]))
    lay.update(TX=tuple(o[8:11]), TY=tuple(o[11:14]), bx=tuple(o[14:17]), by=tuple(o[17:20]), patch_blocks=o[20], grid_blocks=o[21])
    assert o[22:] == [0, 0]
    return lay


def signature(lay, n, h, w, pad):
    """What a layout means for the kernel: the regions in order with their HS class, which strips there are, ragged blocks."""
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    tiles_x, tiles_y = (wo + 3) // 4, (ho + 1) // 2
    nreg = lay["nreg"]
    tx, ty, bx, by = (lay[key][:nreg] for key in ("TX", "TY", "bx", "by"))
    hs = tuple(hs_class(t) for t in tx)
    if lay["stack"]:
        strips, kinds = "", ("stack",)
        ragged = (n * tiles_y) % ty[0] != 0
        extents = ((tiles_x, tiles_y),)
    else:
        wm, hm = (bx[0] * tx[0], by[0] * ty[0]) if nreg > 1 else (tiles_x, tiles_y)        # a main region holds whole blocks only
        strips = ("R" if wm < tiles_x else "") + ("B" if hm < tiles_y else "")
        extents = ((wm, hm),) + ((tiles_x - wm, tiles_y),) * ("R" in strips) + ((wm, tiles_y - hm),) * ("B" in strips)
        kinds = ("main" if nreg > 1 else "one",) + tuple({"R": "right", "B": "bottom"}[s] for s in strips)
        ragged = any(ew % a or eh % b for (ew, eh), a, b in zip(extents, tx, ty))
    assert len(kinds) == nreg and len(extents) == nreg, (lay, kinds)
    for (ew, eh), a, b, nx, ny in zip(extents, tx, ty, bx, by):              # the regions tile the grid: every tile in one block
        assert lay["stack"] or (nx == -(-ew // a) and ny == -(-eh // b)), (lay, extents)
    return dict(stack=lay["stack"], nreg=nreg, hs=hs, strips=strips, kinds=kinds, G=lay["G"], ragged=ragged, TX=tx, TY=ty,
                tiles=(tiles_x, tiles_y), ho=ho, wo=wo, patch_blocks=lay["patch_blocks"], per_img=lay["per_img"])


def describe(sig):
    name = lambda v: "rt" if v == RT else str(v)
    regs = " ".join(f"{kd}:hs{name(v)}:{a}x{b}" for kd, v, a, b in zip(sig["kinds"], sig["hs"], sig["TX"], sig["TY"]))
    return f"stack={sig['stack']} nreg={sig['nreg']} [{regs}] G={sig['G']} blocks={sig['patch_blocks']} ragged={int(sig['ragged'])}"


def meets(sig, expect):
    return (sig["stack"] == expect["stack"] and sig["nreg"] == expect["nreg"] and sig["hs"] == expect["hs"] and sig["G"] >= expect["g_min"]
            and sig["ragged"] == expect["ragged"] and sig["strips"] == expect["strips"])
