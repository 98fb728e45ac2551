"""Seeded stress of the implicit-GEMM convolution family (csrc/seam_conv.hip: ``conv_igemm``, ``conv_igemm_bx3``, ``conv_igemm_sx``)
through the C ABI, against the float64 references of tests/conv_refs.py.

These kernels take every convolution no specialised kernel serves, and they are what the specialised kernels are judged against,
so they get the generic shapes here: small-C tap packing (C = 12 ... 28 / 24 ... 56), R != S, strides 1-3, pad >= R, K off the
64-row slab, every tile instance (forced through the SEAM_CONV_TILE selector where the cost model would not pick it), persistent
launches with more tiles than block slots and a ragged XCD split, tiles that span hundreds of images, the output grid on which
``split_row()`` must divide (``div_fast == 0``), the upsampled-residual epilogue at non-integer ratios, the top-left crop, the dual
source with a larger second input, the ReLU-mask epilogue and the weight pack modes 1 and 2.

``generate(family, lib)`` is pure host code (the tile choice comes from the library's host functions), so
tests/test_conv_refs_host.py runs it without a GPU and proves that every case is inside the launchers' acceptance rule
(``accepts``) and that the corner counts of ``REQUIRED`` are met before anything is launched.

The sweep runs in ONE child process (this file as a script) under a wall-clock timeout: every case is announced with a ``START``
line first, so a hang is a failure that names its shape.  Every case is launched twice, onto NaN- and 3e4-poisoned outputs that
must come back bit-identical, finite, with the 1 MiB guard behind them intact.

Tolerances (max|got - ref| / max|ref| against float64) are the project's: 3e-5 for fp32 outputs (test_gpu_stress.py's figure for
the fp32 3x3 kernels at reductions up to 4608 -- the generator draws none longer), 2e-3 for fp16 outputs, test_gpu_bx3.py's
3e-5 (and 1e-5 in the L2 norm) for the split-bf16 kernel, and for the three-plane split additionally the gate
e_sx <= 2 e_f32 + 1e-7 with e_f32 measured on the same case.
"""
import math
import os
import random
import sys
import time

import pytest

import stress_kit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 11
WALL_S = 240          # a hang shows as this timeout; the sweep itself takes well under 90 s

P_F32, P_F16, P_BX3, P_SX = 0, 1, 2, 3
# family -> (precision of the tile table, number of cases)
FAMILIES = {"f32": (P_F32, 150), "upres": (P_F32, 60), "crop": (P_F32, 60), "dual": (P_F32, 60), "f16": (P_F16, 150),
            "f16dual": (P_F16, 60), "bx3": (P_BX3, 100), "sx6": (P_SX, 100), "sx9": (P_SX, 100), "pack": (P_F32, 30)}
C_F32 = [4, 8, 12, 16, 20, 24, 28, 32, 64, 96, 160, 256]
C_F16 = [8, 16, 24, 40, 56, 64, 128, 192]
SMALL_C = {False: [12, 20, 24, 28], True: [24, 40, 56]}       # tap packing with a fractional number of taps per chunk
K_ALL = [1, 3, 4, 15, 60, 63, 64, 65, 100, 128, 129, 192, 256, 320]
RS = [(1, 1), (2, 2), (3, 3), (5, 5), (7, 7), (1, 3), (3, 1), (1, 7), (7, 1), (2, 3)]
PRIMES = [2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37]
MAX_KRED = 4608            # the fp32 tolerance is the project's figure for reductions up to this length
BUDGET = 3 << 18           # elements of the input and of the output of one case (3 MB of fp32 each)
DIVFAST_GRID = (122, 5958)  # the smallest output grid (Wo < 6000) on which split_row() has to divide (seam_fastdiv.h's rule)
TOL_F32, TOL_F16, TOL_BX3, TOL_BX3_L2 = 3e-5, 2e-3, 3e-5, 1e-5

# corner counts every family must reach (checked on the CPU by test_conv_refs_host.py and again from the child's SUMMARY lines)
GENERIC = {"over_slots_ragged": 5, "ntiles_lt8": 10, "small_c": 20, "small_c_7x7": 2, "small_c_r_ne_s": 5, "many_images": 10,
           "r_ne_s": 10, "stride3": 5, "pad_ge_r": 5, "relu2": 5}
REQUIRED = {
    "f32": dict(GENERIC, div_fast0=2, over_slots_wide=3, tile_256x128=5, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5),
    "f16": dict(GENERIC, div_fast0=2, over_slots_wide=3, tile_256x128=5, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5,
                y_f32=30, y_f16=30, crop_entry=15),
    "bx3": dict(GENERIC, tile_256x128=5, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5),
    # conv_igemm_sx has four instances: there is no 8-wave 256 x 128 form of it
    "sx6": dict(GENERIC, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5),
    "sx9": dict(GENERIC, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5),
    "upres": dict(over_slots_ragged=2, ratio_integer=8, ratio_fraction=8, ratio_one=5, coarse_one=5, many_images=10, ntiles_lt8=5,
                  tile_128x128=3, tile_128x64=3, tile_64x128=3, tile_64x64=3),
    "crop": dict(crop_full=3, crop_one=3, crop_inside=20, ntiles_lt8=5),
    # the dual form has four instances per precision (a 256-row choice runs as 128 x 128)
    "dual": dict(over_slots_ragged=2, stride2_1=8, stride2_2=8, stride2_3=8, x2_larger=20, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5),
    "f16dual": dict(over_slots_ragged=2, stride2_1=8, stride2_2=8, stride2_3=8, x2_larger=20, tile_128x128=5, tile_128x64=5, tile_64x128=5, tile_64x64=5),
    "pack": dict(mode1=15, mode2=15, cin_padded=10, k_padded=10, relu2=3),
}


# ------------------------------------------------------------------------------------------------ the case generator (host only)
def _instances(prec, dual=False):
    t = [(128, 128), (128, 64), (64, 128), (64, 64)]
    return t if (dual or prec == P_SX) else [(256, 128)] + t


def _slab(k):
    return 128 if (((k + 63) // 64) * 64) % 128 == 0 else 64


def _dim(rng, lo=1, hi=40):
    lo = max(lo, 1)
    hi = max(hi, lo)
    if rng.random() < 0.35:
        return rng.choice([p for p in PRIMES if lo <= p <= hi] or [lo])
    return rng.randint(lo, hi)


def _pick_n(rng, per_img, budget=BUDGET):
    nmax = max(1, min(3000, budget // max(per_img, 1)))
    r = rng.random()
    if r < 0.3:
        return rng.randint(1, min(3, nmax))
    if r < 0.4:
        return nmax
    return rng.randint(1, nmax)


def _out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def _renew_n(rng, b):
    """a batch size for a case whose geometry was edited after the draw"""
    ho, wo = _out(b["h"], b["R"], b["stride"], b["pad"]), _out(b["w"], b["S"], b["stride"], b["pad"])
    b["n"] = _pick_n(rng, max(b["h"] * b["w"] * b["c"], ho * wo * b["k"]))
    return b


def _epilogue(rng, allow_res=True, allow_relu2=True):
    epi = rng.choice(["none", "bias", "bn"])
    relu = rng.choice([0, 1, 2] if (allow_res and allow_relu2) else [0, 1])
    res = True if relu == 2 else (allow_res and rng.random() < 0.5)
    return epi, relu, res


def _conv_case(rng, f16, kind="rand", k_choices=None, need_slab128=False):
    """One generic convolution: dict(n, h, w, c, k, R, S, stride, pad).  kind: rand | small_c | many_images | over_slots | tiny."""
    clist = C_F16 if f16 else C_F32
    for _ in range(10000):
        ks = [k for k in (k_choices or K_ALL) if not need_slab128 or _slab(k) == 128]
        k = rng.choice(ks)
        R, S = rng.choice(RS)
        stride, pad = rng.choice([1, 1, 2, 3]), rng.randint(0, 3)
        c = rng.choice(clist)
        if kind == "small_c":
            c = rng.choice(SMALL_C[f16])
        elif kind == "over_slots":
            c, (R, S), stride = clist[0], rng.choice([(1, 1), (3, 3)]), 1
            pad = R // 2
            k = rng.choice([kk for kk in ks if kk <= 64] or ks)
        if R * S * c > MAX_KRED:
            continue
        if kind == "many_images":       # 1 <= Ho*Wo <= 7 under N in [100, 3000]: a tile spans many images
            ho, wo = rng.choice([(1, 1), (1, 2), (2, 1), (1, 3), (3, 1), (2, 2), (1, 5), (5, 1), (2, 3), (3, 2), (1, 7), (7, 1), (1, 4)])
            h = (ho - 1) * stride + R - 2 * pad + rng.randint(0, stride - 1)
            w = (wo - 1) * stride + S - 2 * pad + rng.randint(0, stride - 1)
            if h < 1 or w < 1:
                continue
            nmax = min(3000, BUDGET // max(h * w * c, ho * wo * k))
            if nmax < 100:
                continue
            n = rng.randint(100, nmax)
        elif kind == "over_slots":      # ~70 000 output pixels of a 4-channel map: more tiles than block slots
            h = w = rng.choice([31, 33, 35, 37, 39])      # odd: the tile count moves off the multiples of 8 with the batch
            n = -(-rng.randint(66000, 72000) // (h * w))
        elif kind == "tiny":
            h, w = _dim(rng, R - 2 * pad, 6), _dim(rng, S - 2 * pad, 6)
            n = 1
        else:
            h, w = _dim(rng, R - 2 * pad), _dim(rng, S - 2 * pad)
            ho, wo = _out(h, R, stride, pad), _out(w, S, stride, pad)
            n = _pick_n(rng, max(h * w * c, ho * wo * k))
        ho, wo = _out(h, R, stride, pad), _out(w, S, stride, pad)
        if ho < 1 or wo < 1:
            continue
        return dict(n=n, h=h, w=w, c=c, k=k, R=R, S=S, stride=stride, pad=pad)
    raise RuntimeError("no case found")


def _finish(lib, fam, prec, case, dual=False):
    """Derived figures of a case: output grid, M, the tile the launcher will run, its tile count, slots and div_fast."""
    c = case
    c["family"] = fam
    c.setdefault("force", 0)
    full = (_out(c["h"], c["R"], c["stride"], c["pad"]), _out(c["w"], c["S"], c["stride"], c["pad"]))
    c["full"] = full
    c["ho"], c["wo"] = c.get("crop", full)
    c["m"] = c["n"] * c["ho"] * c["wo"]
    taps = c["R"] * c["S"] if prec in (P_F32, P_F16) else 1
    assert lib.seam_set_option(b"SEAM_CONV_TILE", c["force"]) == 0
    t = lib.seam_conv_tile_taps(prec, c["m"], c["k"], taps)
    assert lib.seam_set_option(b"SEAM_CONV_TILE", 0) == 0
    bm, bn = t // 1000, t % 1000
    if dual and bm == 256:
        bm = 128
    c["bm"], c["bn"] = bm, bn
    c["ntiles"] = -(-c["m"] // bm) * ((((c["k"] + 63) // 64) * 64) // bn)
    c["slots"] = 256 if bm == 256 else 512
    howo = c["ho"] * c["wo"]
    c["div_fast"] = int((howo >= 256 or lib.seam_fastdiv_exact(howo, howo + 256) == 1) and lib.seam_fastdiv_exact(c["wo"], howo) == 1)
    return c


def accepts(c):
    """The launchers' written acceptance rule (conv2d<T>() / conv2d_bx3() in csrc/seam_conv.hip and the extern "C" wrappers)."""
    fam = c["family"]
    f16 = fam in ("f16", "f16dual")
    epv, bke = (8, 64) if f16 else (4, 32)
    if c["c"] % epv or (c["c"] >= bke and c["c"] % bke) or c["n"] <= 0 or c["k"] <= 0:
        return False
    if c["full"][0] <= 0 or c["full"][1] <= 0 or c["ho"] <= 0 or c["wo"] <= 0:
        return False
    if "crop" in c and (c["crop"][0] > c["full"][0] or c["crop"][1] > c["full"][1] or c["res"] or f16 and c.get("y_f32")):
        return False
    if c["relu"] not in (0, 1, 2) or (c["relu"] == 2 and not c["res"]):
        return False
    if fam == "upres" and (c["k"] % 4 or c["rh"] <= 0 or c["rw"] <= 0 or not c["res"] or c["relu"] == 2):
        return False
    if fam in ("dual", "f16dual"):
        if (c["R"], c["S"], c["stride"], c["pad"]) != (1, 1, 1, 0) or c["c"] % bke or c["c2"] % bke or c["stride2"] < 1 or c["res"]:
            return False
        if (c["ho"] - 1) * c["stride2"] >= c["h2"] or (c["wo"] - 1) * c["stride2"] >= c["w2"]:
            return False
    if fam in ("sx6", "sx9") and c["terms"] not in (6, 9):
        return False
    if fam in ("bx3", "sx6", "sx9", "f16", "f32") and "crop" in c and fam != "f16":
        return False
    return True


def _over_slots(lib, fam, prec, b, force=0, dual=False):
    """grow the batch of an over_slots draw until the launch has more tiles than slots and a tile count that is no multiple of 8"""
    for _ in range(64):
        t = _finish(lib, fam, prec, dict(b, epi="none", relu=0, res=False, force=force), dual)
        if t["ntiles"] > t["slots"] and t["ntiles"] % 8:
            return b
        b["n"] += 1
    raise RuntimeError("no over-slots batch found")


def _generic_family(lib, fam, prec, count, rng):
    f16 = prec == P_F16
    cases = []

    def add(base, force=0, entry=None, **extra):
        epi, relu, res = _epilogue(rng)
        c = dict(base, epi=epi, relu=relu, res=res, force=force, **extra)
        if fam == "f16":            # three entries: fp16 output, fp32 output, and the cropped form (fp16 output, no residual)
            c["y_f32"] = int(rng.random() < 0.4) if entry is None else int(entry == "f32")
            if entry == "crop":
                full = (_out(c["h"], c["R"], c["stride"], c["pad"]), _out(c["w"], c["S"], c["stride"], c["pad"]))
                c["crop"] = (rng.randint(1, full[0]), rng.randint(1, full[1]))
                c["res"], c["relu"] = False, rng.choice([0, 1])
        if fam in ("sx6", "sx9"):
            c["terms"] = 6 if fam == "sx6" else 9
        cases.append(_finish(lib, fam, prec, c))

    # every tile instance, forced where the cost model would not pick it
    for bm, bn in _instances(prec):
        for _ in range(5):
            add(dict(_conv_case(rng, f16, need_slab128=(bn == 128)), kind="forced"), force=bm * 1000 + bn)
    smallrs = [(7, 7), (1, 3), (3, 1), (1, 7), (7, 1), (2, 3), (3, 3), (5, 5), (2, 2), (1, 1)]
    for i in range(20):                 # small-C tap packing: a chunk holds a fractional number of taps
        b = _conv_case(rng, f16, "small_c")
        b["c"] = SMALL_C[f16][i % len(SMALL_C[f16])]
        R, S = smallrs[i % len(smallrs)]
        pad = rng.randint(0, 3)
        b.update(R=R, S=S, pad=pad, h=_dim(rng, R - 2 * pad, 24), w=_dim(rng, S - 2 * pad, 24))
        add(dict(_renew_n(rng, b), kind="small_c"))
    for _ in range(10):
        add(dict(_conv_case(rng, f16, "many_images"), kind="many_images"))
    for _ in range(10):
        add(dict(_conv_case(rng, f16, "tiny", k_choices=[1, 3, 4, 15, 60, 63, 64, 65, 100, 128]), kind="tiny"))
    for _ in range(6):                  # more tiles than block slots, and a tile count that is no multiple of 8
        add(dict(_over_slots(lib, fam, prec, _conv_case(rng, f16, "over_slots")), kind="over_slots"))
    if prec in (P_F32, P_F16):          # ... and the persistent loop of the wide tiles (conv_igemm alone walks tiles): K = 128
        for bm, bn in ((256, 128), (128, 128), (64, 128)):
            force = bm * 1000 + bn
            add(dict(_over_slots(lib, fam, prec, _conv_case(rng, f16, "over_slots", k_choices=[128]), force), kind="over_slots"), force=force)
    if prec in (P_F32, P_F16):          # split_row() without the multiply-high: conv_igemm only (the split kernels always divide)
        ho, wo = DIVFAST_GRID
        c0 = C_F16[0] if f16 else C_F32[0]
        add(dict(n=1, h=ho, w=wo, c=c0, k=4, R=3, S=3, stride=1, pad=1, kind="div_fast0"))
        add(dict(n=1, h=2 * ho - 1, w=2 * wo - 1, c=c0, k=4, R=3, S=3, stride=2, pad=1, kind="div_fast0"))
    # the directed corners the random draw reaches too rarely to count on
    for _ in range(6):
        b = _conv_case(rng, f16)
        b["stride"] = 3
        add(dict(_renew_n(rng, b), kind="rand"))
    for _ in range(6):
        b = _conv_case(rng, f16)
        R, S = rng.choice([(1, 1), (2, 2), (1, 3), (3, 1), (2, 3), (3, 3)])
        b.update(R=R, S=S, pad=3, h=_dim(rng, 1, 24), w=_dim(rng, 1, 24))
        add(dict(_renew_n(rng, b), kind="rand"))
    while len(cases) < count:
        b = _conv_case(rng, f16)
        force = 0
        if rng.random() < 0.5:
            bm, bn = rng.choice([t for t in _instances(prec) if t[1] <= _slab(b["k"])])
            force = bm * 1000 + bn
        add(dict(b, kind="rand"), force=force, entry=("crop", "f32", "f16")[len(cases) % 3])
    return cases


def _upres_family(lib, fam, prec, count, rng):
    cases = []
    k4 = [k for k in K_ALL if k % 4 == 0]

    def coarse(size, how):
        if how == "one":
            return 1
        if how == "same":
            return size
        if how == "integer":
            divs = [d for d in (2, 3, 4, 5) if size % d == 0]
            return size // rng.choice(divs) if divs else size
        return {25: 13, 7: 3, 40: 17}.get(size, max(1, (size * 10 + 18) // 19))       # a non-integer ratio

    def add(b, how_h, how_w, force=0, kind="rand"):
        ho, wo = _out(b["h"], b["R"], b["stride"], b["pad"]), _out(b["w"], b["S"], b["stride"], b["pad"])
        epi = rng.choice(["none", "bias", "bn"])
        c = dict(b, epi=epi, relu=rng.choice([0, 1]), res=True, rh=coarse(ho, how_h), rw=coarse(wo, how_w), force=force, kind=kind)
        cases.append(_finish(lib, fam, prec, c))

    hows = ["integer", "fraction", "same", "one"]
    for i, (bm, bn) in enumerate(_instances(prec, dual=True) * 3):
        add(_conv_case(rng, False, k_choices=k4, need_slab128=(bn == 128)), hows[i % 4], hows[(i // 4) % 4], force=bm * 1000 + bn, kind="forced")
    for i in range(10):       # N large, Ho*Wo small: a tile spans many coarse images (up_first)
        add(_conv_case(rng, False, "many_images", k_choices=k4), rng.choice(hows), rng.choice(hows), kind="many_images")
    for size in (25, 7, 40, 25, 7, 40):       # the non-integer ratios by name: 25 from 13, 7 from 3, 40 from 17 (pointwise and 3x3 / pad 1)
        b = _conv_case(rng, False, k_choices=k4)
        R = rng.choice([1, 3])
        b.update(R=R, S=R, stride=1, pad=R // 2, h=size, w=rng.choice([25, 7, 40]))
        add(_renew_n(rng, b), "fraction", "fraction")
    for size in (8, 12, 20, 30, 9, 40, 6, 10):        # integer ratios 2 ... 5
        b = _conv_case(rng, False, k_choices=k4)
        R = rng.choice([1, 3])
        b.update(R=R, S=R, stride=1, pad=R // 2, h=size, w=rng.choice([8, 12, 9, 30]))
        add(_renew_n(rng, b), "integer", "integer")
    for _ in range(6):
        add(_conv_case(rng, False, "tiny", k_choices=[4, 60, 64, 100, 128]), rng.choice(hows), rng.choice(hows), kind="tiny")
    for how in ("fraction", "integer"):       # the persistent loop: every tile of a block rebases the coarse map anew
        add(_over_slots(lib, fam, prec, _conv_case(rng, False, "over_slots", k_choices=[4, 60, 64])), how, "fraction", kind="over_slots")
    while len(cases) < count:
        add(_conv_case(rng, False, k_choices=k4), rng.choice(hows), rng.choice(hows))
    return cases


def _crop_family(lib, fam, prec, count, rng):
    cases = []
    ends = [("full", "full"), ("one", "one"), ("one", "full"), ("full", "one")] * 2
    while len(cases) < count:
        i = len(cases)
        b = _conv_case(rng, False, "tiny" if 8 <= i < 14 else "rand")
        full = (_out(b["h"], b["R"], b["stride"], b["pad"]), _out(b["w"], b["S"], b["stride"], b["pad"]))
        pick = lambda f, how: f if how == "full" else 1 if how == "one" else rng.randint(1, f)
        how = ends[i] if i < len(ends) else ("any", "any")
        crop = (pick(full[0], how[0]), pick(full[1], how[1]))
        force = 0
        if rng.random() < 0.5:
            bm, bn = rng.choice([t for t in _instances(prec) if t[1] <= _slab(b["k"])])
            force = bm * 1000 + bn
        c = dict(b, epi=rng.choice(["none", "bias", "bn"]), relu=rng.choice([0, 1]), res=False, crop=crop, force=force, kind="rand")
        cases.append(_finish(lib, fam, prec, c))
    return cases


def _dual_family(lib, fam, prec, count, rng):
    f16 = prec == P_F16
    cs = [64, 128, 192] if f16 else [32, 64, 96, 128, 160]
    cases = []
    inst = _instances(prec, dual=True) * 5
    while len(cases) < count:
        i = len(cases)
        c1 = rng.choice(cs)
        c2 = rng.choice([v for v in cs if v != c1])
        bn = inst[i][1] if i < len(inst) else 0
        k = rng.choice([kk for kk in K_ALL if bn != 128 or _slab(kk) == 128])
        many = len(inst) <= i < len(inst) + 8
        over = len(inst) + 8 <= i < len(inst) + 10          # the persistent loop: more tiles than block slots
        ho, wo = (rng.choice([1, 2]), rng.choice([1, 2, 3])) if many else (_dim(rng, 1, 30), _dim(rng, 1, 30))
        stride2 = (i % 3) + 1
        if over:
            ho = wo = rng.choice([31, 33, 35, 37, 39])
            c1, c2, k, stride2 = cs[0], cs[1], rng.choice([60, 64]), 1
        h2 = (ho - 1) * stride2 + 1 + rng.randint(0, 3)
        w2 = (wo - 1) * stride2 + 1 + rng.randint(0, 3)
        per = max(ho * wo * max(c1, k), h2 * w2 * c2)
        n = rng.randint(100, max(100, min(1500, BUDGET // per))) if many else _pick_n(rng, per)
        if over:
            n = -(-66000 // (ho * wo))
        c = dict(n=n, h=ho, w=wo, c=c1, k=k, R=1, S=1, stride=1, pad=0, c2=c2, h2=h2, w2=w2, stride2=stride2,
                 epi=rng.choice(["none", "bias", "bn"]), relu=rng.choice([0, 1]), res=False,
                 force=inst[i][0] * 1000 + inst[i][1] if i < len(inst) else 0,
                 kind="many_images" if many else "over_slots" if over else "rand")
        if over:
            _over_slots(lib, fam, prec, c, dual=True)
        cases.append(_finish(lib, fam, prec, c, dual=True))
    return cases


def _pack_family(lib, fam, prec, count, rng):
    """Weight pack modes 1 (ConvTranspose2d 2x2 / stride 2 as a 1x1 conv onto 4*Cout sub-pixel channels) and 2 (the rotated,
    channel-swapped weights of a stride-1 convolution's input gradient), both run by seam_conv2d_f32.  ``cin`` is the weight's
    own reduction width; the activations carry ``c`` >= cin channels (the store width the launcher accepts) and the pack must
    leave the difference, like the rows past K, zero."""
    store = lambda cin: ((cin + 3) // 4) * 4 if cin < 32 else ((cin + 31) // 32) * 32
    cases = []
    while len(cases) < count:
        i = len(cases)
        epi, relu, res = _epilogue(rng)
        if i % 2 == 0:
            cin, cout = rng.choice([3, 6, 10, 16, 30, 32, 50, 64, 100]), rng.choice([1, 3, 16, 25, 32, 64])
            h, w = _dim(rng, 1, 20), _dim(rng, 1, 20)
            c = dict(mode=1, cin=cin, c=store(cin), k=4 * cout, R=1, S=1, stride=1, pad=0, h=h, w=w)
        else:
            cout, cin_f = rng.choice([5, 12, 30, 32, 64, 96]), rng.choice([3, 16, 60, 64, 65, 100, 128])
            R = rng.choice([1, 2, 3, 5])
            pad_fwd = rng.randint(0, R - 1)
            hin = _dim(rng, max(1, R - 2 * pad_fwd), 20), _dim(rng, max(1, R - 2 * pad_fwd), 20)      # the forward input = this case's output
            h, w = hin[0] + 2 * pad_fwd - R + 1, hin[1] + 2 * pad_fwd - R + 1
            c = dict(mode=2, cin=cout, c=store(cout), k=cin_f, R=R, S=R, stride=1, pad=R - 1 - pad_fwd, h=h, w=w, pad_fwd=pad_fwd)
        c["n"] = _pick_n(rng, c["h"] * c["w"] * max(c["c"], c["k"]) * 4, BUDGET)
        cases.append(_finish(lib, fam, prec, dict(c, epi=epi, relu=relu, res=res, kind="rand")))
    return cases


def generate(family, lib, seed=SEED):
    """The seeded cases of one family: the same list on every machine (the tile choice is the library's host function)."""
    prec, count = FAMILIES[family]
    rng = random.Random(seed * 7919 + sorted(FAMILIES).index(family))
    if family in ("f32", "f16", "bx3", "sx6", "sx9"):
        cases = _generic_family(lib, family, prec, count, rng)
    elif family == "upres":
        cases = _upres_family(lib, family, prec, count, rng)
    elif family == "crop":
        cases = _crop_family(lib, family, prec, count, rng)
    elif family in ("dual", "f16dual"):
        cases = _dual_family(lib, family, prec, count, rng)
    else:
        cases = _pack_family(lib, family, prec, count, rng)
    for i, c in enumerate(cases):
        c["tseed"] = seed * 100003 + i
    return cases


def corner_counts(cases):
    """How often the cases of one family reach each corner of the launchers and kernels (REQUIRED gives the minima)."""
    n = {}

    def hit(key, cond=True):
        n[key] = n.get(key, 0) + int(bool(cond))

    for c in cases:
        f16 = c["family"] in ("f16", "f16dual")
        hit(f"tile_{c['bm']}x{c['bn']}")
        hit("over_slots_ragged", c["ntiles"] > c["slots"] and c["ntiles"] % 8 != 0)
        hit("over_slots_wide", c["ntiles"] > c["slots"] and c["ntiles"] % 8 != 0 and c["bn"] == 128)
        hit("ntiles_lt8", c["ntiles"] < 8)
        small = c["c"] in SMALL_C[f16] and c["family"] not in ("dual", "f16dual")
        hit("small_c", small)
        hit("small_c_7x7", small and (c["R"], c["S"]) == (7, 7))
        hit("small_c_r_ne_s", small and c["R"] != c["S"])
        hit("many_images", 100 <= c["n"] <= 3000 and 1 <= c["ho"] * c["wo"] <= 7)
        hit("r_ne_s", c["R"] != c["S"])
        hit("stride3", c["stride"] == 3)
        hit("pad_ge_r", c["pad"] >= c["R"])
        hit("relu2", c["relu"] == 2)
        hit("div_fast0", c["div_fast"] == 0)
        hit("k_not_64", c["k"] % 64 != 0)
        if c["family"] == "f16":
            hit("y_f32", c.get("y_f32") == 1)
            hit("y_f16", c.get("y_f32") == 0)
            hit("crop_entry", "crop" in c)
        if c["family"] == "upres":
            rh, ho = c["rh"], c["ho"]
            hit("ratio_one", rh == ho and ho > 1)
            hit("coarse_one", rh == 1 and ho > 1)
            hit("ratio_integer", 1 < rh < ho and ho % rh == 0)
            hit("ratio_fraction", 1 < rh < ho and ho % rh != 0)
        if "crop" in c:
            hit("crop_full", c["crop"] == c["full"])
            hit("crop_one", c["crop"] == (1, 1))
            hit("crop_inside", c["crop"][0] < c["full"][0] or c["crop"][1] < c["full"][1])
        if "stride2" in c:
            hit(f"stride2_{c['stride2']}")
            hit("x2_larger", c["h2"] > (c["ho"] - 1) * c["stride2"] + 1 or c["w2"] > (c["wo"] - 1) * c["stride2"] + 1)
        if "mode" in c:
            hit(f"mode{c['mode']}")
            hit("cin_padded", c["c"] > c["cin"])
            hit("k_padded", c["k"] % 64 != 0)
    return n


def describe(c):
    d = (f"n={c['n']} {c['h']}x{c['w']} c={c['c']} k={c['k']} {c['R']}x{c['S']} s={c['stride']} p={c['pad']} out={c['ho']}x{c['wo']} "
         f"epi={c['epi']} relu={c['relu']} res={int(c['res'])} tile={c['bm']}x{c['bn']} forced={int(c['force'] != 0)} ntiles={c['ntiles']} "
         f"div_fast={c['div_fast']}")
    for key in ("y_f32", "crop", "rh", "rw", "c2", "h2", "w2", "stride2", "terms", "mode", "cin"):
        if key in c:
            d += f" {key}={c[key]}"
    return d


# ------------------------------------------------------------------------------------------------ the child: launches and checks
def child_main(argv):
    sys.path.insert(0, ROOT)
    import torch
    import conv_refs as CR
    import seam_match_rcnn_amd.ops as ops
    from seam_match_rcnn_amd import _native

    seed = int(argv[0])
    only = argv[1:]
    dev = torch.device("cuda:0")
    lib = _native.lib()
    Buf, P, fails, say, st = stress_kit.Buf, stress_kit.P, stress_kit.fails, stress_kit.say, stress_kit.st
    bufs = []

    def poisoned(shape, dtype, which):
        bufs.append(Buf(shape, dtype, which))
        return bufs[-1].t

    def guards_intact():
        ok = all(b.guard_ok() for b in bufs)
        bufs.clear()
        return ok

    def errors(got, ref):
        """max|got - ref| / max|ref| and ||got - ref|| / ||ref|| against the float64 reference"""
        d = got.double() - ref
        sc = max(float(ref.abs().max()), 1e-20)
        nr = float(ref.norm())
        return float(d.abs().max()) / sc, (float(d.norm()) / nr if nr > 0 else float(d.norm()))

    def tensors(c, f16):
        g = torch.Generator(device=dev)
        g.manual_seed(c["tseed"])
        rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
        k = c["k"]
        scale = shift = None
        if c["epi"] != "none":
            shift = rnd(k) * 0.2
        if c["epi"] == "bn":
            scale = torch.rand(k, device=dev, generator=g) + 0.5
        x = rnd(c["n"], c["h"], c["w"], c["c"])
        return g, rnd, x.half() if f16 else x, scale, shift

    def pack(c, wt, prec, cin=None, mode=0, kk=None):
        """the weights of a case in the precision's packed form"""
        k, cs, R, S = (c["k"] if kk is None else kk), c["c"] + c.get("c2", 0), c["R"], c["S"]
        cin = cs if cin is None else cin
        rows = lib.seam_conv_rows_padded(k)
        if prec == P_F16:
            wp = torch.empty((rows, lib.seam_conv_kred_f16(cs, R, S)), dtype=torch.float16, device=dev)
            rc = lib.seam_pack_conv_weight_f16(P(wt), P(wp), k, cin, R, S, cs, mode, st())
        else:
            kred = lib.seam_conv_kred(cs, R, S)
            wp = torch.empty((rows, kred), dtype=torch.float32, device=dev)
            if prec == P_F32:
                rc = lib.seam_pack_conv_weight_f32(P(wt), P(wp), k, cin, R, S, cs, mode, st())
            else:
                tmp = torch.empty((rows, kred), dtype=torch.float32, device=dev)
                if prec == P_SX:
                    wp = torch.empty((rows, kred * 3), dtype=torch.bfloat16, device=dev)
                    rc = lib.seam_pack_conv_weight_sx(P(wt), P(wp), P(tmp), k, cin, R, S, cs, mode, st())
                else:
                    rc = lib.seam_pack_conv_weight_bx3(P(wt), P(wp), P(tmp), k, cin, R, S, cs, mode, st())
        assert rc == 0, ("pack", describe(c), rc)
        return wp

    def twice(c, shape, dtype, launch):
        """two launches onto differently poisoned outputs, under the case's forced tile"""
        outs = []
        assert lib.seam_set_option(b"SEAM_CONV_TILE", c["force"]) == 0
        try:
            for rep in range(2):
                y = poisoned(shape, dtype, rep)
                rc = launch(y)
                assert rc == 0, (describe(c), rc)
                outs.append(y)
        finally:
            lib.seam_set_option(b"SEAM_CONV_TILE", 0)
        return outs

    def judge(fam, c, outs, ref, tol, tol_l2=None, extra=None):
        why = ""
        e = el2 = float("nan")
        if not guards_intact():
            why = "bytes BEHIND the output tensor were overwritten"
        elif not torch.equal(outs[0].view(torch.uint8), outs[1].view(torch.uint8)):
            why = "two launches differ"
        elif not bool(torch.isfinite(outs[0].float()).all()):
            why = "poison / non-finite values left in the output"
        else:
            e, el2 = errors(outs[0], ref)
            if not e <= tol:
                why = f"{e:.3e} of scale from the float64 reference (tolerance {tol:.0e})"
            elif tol_l2 is not None and not el2 <= tol_l2:
                why = f"L2 error {el2:.3e} (tolerance {tol_l2:.0e})"
            elif extra is not None:
                why = extra(e)
        if why:
            fails.append((fam, describe(c), why))
            say("FAIL", fam, describe(c), why)
        return e, el2

    def run_generic(fam, c):
        prec = FAMILIES[fam][0]
        f16 = prec == P_F16
        g, rnd, x, scale, shift = tensors(c, f16)
        k, R, S = c["k"], c["R"], c["S"]
        wt = rnd(k, c["c"], R, S) / math.sqrt(R * S * c["c"])
        if f16:
            wt = wt.half().float()
        res = rnd(c["n"], c["ho"], c["wo"], k) if c["res"] else None
        if f16 and res is not None:
            res = res.half()
        wp = pack(c, wt, prec)
        geo = (c["n"], c["h"], c["w"], c["c"], k, R, S, c["stride"], c["pad"])
        shape = (c["n"], c["ho"], c["wo"], k)
        crop = c.get("crop")
        acc = CR.conv_nhwc_f64(x, wt, R, S, c["stride"], c["pad"], *(crop or (None, None)))
        ref = CR.epilogue_f64(acc, scale, shift, res, c["relu"])
        if prec == P_F32:
            if crop:
                outs = twice(c, shape, torch.float32, lambda y: lib.seam_conv2d_crop_f32(P(x), P(wp), P(scale), P(shift), P(y), *geo, *crop, c["relu"], st()))
            else:
                outs = twice(c, shape, torch.float32, lambda y: lib.seam_conv2d_f32(P(x), P(wp), P(scale), P(shift), P(res), P(y), *geo, c["relu"], st()))
            return judge(fam, c, outs, ref, TOL_F32)
        if prec == P_F16:
            if crop:
                outs = twice(c, shape, torch.float16, lambda y: lib.seam_conv2d_crop_f16(P(x), P(wp), P(scale), P(shift), P(y), *geo, *crop, c["relu"], st()))
                return judge(fam, c, outs, ref, TOL_F16)
            yf = c["y_f32"]
            outs = twice(c, shape, torch.float32 if yf else torch.float16,
                         lambda y: lib.seam_conv2d_f16(P(x), P(wp), P(scale), P(shift), P(res), P(y), *geo, c["relu"], yf, st()))
            return judge(fam, c, outs, ref, TOL_F32 if yf else TOL_F16)
        if prec == P_BX3:
            outs = twice(c, shape, torch.float32, lambda y: lib.seam_conv2d_bx3(P(x), P(wp), P(scale), P(shift), P(res), P(y), *geo, c["relu"], st()))
            return judge(fam, c, outs, ref, TOL_BX3, TOL_BX3_L2)
        outs = twice(c, shape, torch.float32, lambda y: lib.seam_conv2d_sx(P(x), P(wp), P(scale), P(shift), P(res), P(y), *geo, c["relu"], c["terms"], st()))
        # the project's gate: the split may be twice as far from float64 as the exact fp32 kernel on the same case
        w32 = pack(c, wt, P_F32)
        y32 = torch.empty(shape, dtype=torch.float32, device=dev)
        assert lib.seam_conv2d_f32(P(x), P(w32), P(scale), P(shift), P(res), P(y32), *geo, c["relu"], st()) == 0
        e32, _ = errors(y32, ref)
        gate = lambda e: "" if e <= 2 * e32 + 1e-7 else f"e_sx {e:.3e} > 2 * e_f32 {e32:.3e} + 1e-7"
        e, el2 = judge(fam, c, outs, ref, TOL_F32, extra=gate)
        return e, el2, e32

    def run_upres(fam, c):
        g, rnd, x, scale, shift = tensors(c, False)
        k, R, S = c["k"], c["R"], c["S"]
        wt = rnd(k, c["c"], R, S) / math.sqrt(R * S * c["c"])
        top = rnd(c["n"], c["rh"], c["rw"], k)
        wp = pack(c, wt, P_F32)
        geo = (c["n"], c["h"], c["w"], c["c"], k, R, S, c["stride"], c["pad"])
        outs = twice(c, (c["n"], c["ho"], c["wo"], k), torch.float32,
                     lambda y: lib.seam_conv2d_upres_f32(P(x), P(wp), P(scale), P(shift), P(top), P(y), *geo, c["rh"], c["rw"], c["relu"], st()))
        ref = CR.epilogue_f64(CR.conv_nhwc_f64(x, wt, R, S, c["stride"], c["pad"]), scale, shift, CR.nearest_up_f64(top, c["ho"], c["wo"]), c["relu"])
        return judge(fam, c, outs, ref, TOL_F32)

    def run_dual(fam, c):
        f16 = fam == "f16dual"
        g, rnd, x1, scale, shift = tensors(c, f16)
        k, c1, c2 = c["k"], c["c"], c["c2"]
        x2 = rnd(c["n"], c["h2"], c["w2"], c2)
        wt = rnd(k, c1 + c2) / math.sqrt(c1 + c2)
        if f16:
            x2, wt = x2.half(), wt.half().float()
        wp = pack(c, wt, P_F16 if f16 else P_F32)
        fn = lib.seam_conv2d_dual_f16 if f16 else lib.seam_conv2d_dual_f32
        outs = twice(c, (c["n"], c["ho"], c["wo"], k), torch.float16 if f16 else torch.float32,
                     lambda y: fn(P(x1), P(x2), P(wp), P(scale), P(shift), P(y), c["n"], c["ho"], c["wo"], c1, c["h2"], c["w2"], c2, c["stride2"], k, c["relu"], st()))
        ref = CR.epilogue_f64(CR.dual_f64(x1, x2, wt, c["stride2"]), scale, shift, None, c["relu"])
        return judge(fam, c, outs, ref, TOL_F16 if f16 else TOL_F32)

    def run_pack(fam, c):
        g, rnd, x, scale, shift = tensors(c, False)       # x carries c >= cin channels: the pack's zero columns meet random data
        k, R, cin = c["k"], c["R"], c["cin"]
        res = rnd(c["n"], c["ho"], c["wo"], k) if c["res"] else None
        if c["mode"] == 1:
            wt = rnd(cin, k // 4, 2, 2) / math.sqrt(cin)
            acc = CR.conv_transpose2x2_subpixel_f64(x[..., :cin], wt)
        else:
            wt = rnd(cin, k, R, R) / math.sqrt(R * R * cin)          # the forward weight [Cout, Cin, R, R]; this launch computes dX from dY = x
            acc = CR.dgrad_f64(x[..., :cin], wt, c["pad_fwd"])
        wp = pack(c, wt, P_F32, cin=cin, mode=c["mode"])
        geo = (c["n"], c["h"], c["w"], c["c"], k, R, R, 1, c["pad"])
        outs = twice(c, (c["n"], c["ho"], c["wo"], k), torch.float32,
                     lambda y: lib.seam_conv2d_f32(P(x), P(wp), P(scale), P(shift), P(res), P(y), *geo, c["relu"], st()))
        return judge(fam, c, outs, CR.epilogue_f64(acc, scale, shift, res, c["relu"]), TOL_F32)

    def refusals():
        """Shapes outside the launchers' rule: a non-zero return and no launch (the dummy buffer is never dereferenced)."""
        t0 = time.time()
        d = torch.zeros(1 << 16, device=dev)
        p = P(d)
        s = st()
        bad = []

        tried = [0]

        def refused(what, rc):
            tried[0] += 1
            if rc == 0:
                bad.append(what)

        say("START refusals -")
        for cc in (6, 36):
            refused(f"fp32 C={cc}", lib.seam_conv2d_f32(p, p, None, None, None, p, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, s))
            refused(f"bx3 C={cc}", lib.seam_conv2d_bx3(p, p, None, None, None, p, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, s))
            refused(f"sx C={cc}", lib.seam_conv2d_sx(p, p, None, None, None, p, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, 6, s))
            refused(f"fp32 pack Cstore={cc}", lib.seam_pack_conv_weight_f32(p, p, 64, cc, 3, 3, cc, 0, s))
        for cc in (4, 72):
            refused(f"fp16 C={cc}", lib.seam_conv2d_f16(p, p, None, None, None, p, 1, 8, 8, cc, 64, 3, 3, 1, 1, 0, 0, s))
            refused(f"fp16 pack Cstore={cc}", lib.seam_pack_conv_weight_f16(p, p, 64, cc, 3, 3, cc, 0, s))
        refused("fp32 K=0", lib.seam_conv2d_f32(p, p, None, None, None, p, 1, 8, 8, 32, 0, 3, 3, 1, 1, 0, s))
        refused("fp16 K=0", lib.seam_conv2d_f16(p, p, None, None, None, p, 1, 8, 8, 64, 0, 3, 3, 1, 1, 0, 0, s))
        refused("bx3 K=0", lib.seam_conv2d_bx3(p, p, None, None, None, p, 1, 8, 8, 32, 0, 3, 3, 1, 1, 0, s))
        refused("sx K=0", lib.seam_conv2d_sx(p, p, None, None, None, p, 1, 8, 8, 32, 0, 3, 3, 1, 1, 0, 9, s))
        refused("fp32 Ho<=0", lib.seam_conv2d_f32(p, p, None, None, None, p, 1, 2, 8, 32, 64, 5, 5, 1, 1, 0, s))
        # ... also under a stride, where a division that truncates towards zero would make one output row of the negative extent
        refused("fp32 H+2*pad<R, stride 2", lib.seam_conv2d_f32(p, p, None, None, None, p, 1, 2, 8, 32, 64, 5, 5, 2, 1, 0, s))
        refused("fp32 W+2*pad<S, stride 3", lib.seam_conv2d_f32(p, p, None, None, None, p, 1, 8, 1, 32, 64, 5, 5, 3, 1, 0, s))
        refused("fp16 H+2*pad<R, stride 2", lib.seam_conv2d_f16(p, p, None, None, None, p, 1, 2, 8, 64, 64, 5, 5, 2, 1, 0, 0, s))
        refused("bx3 H+2*pad<R, stride 2", lib.seam_conv2d_bx3(p, p, None, None, None, p, 1, 2, 8, 32, 64, 5, 5, 2, 1, 0, s))
        refused("sx W+2*pad<S, stride 3", lib.seam_conv2d_sx(p, p, None, None, None, p, 1, 8, 1, 32, 64, 5, 5, 3, 1, 0, 9, s))
        refused("crop f32 H+2*pad<R, stride 2", lib.seam_conv2d_crop_f32(p, p, None, None, p, 1, 2, 8, 32, 64, 5, 5, 2, 1, 1, 1, 0, s))
        refused("fp32 Wo<=0", lib.seam_conv2d_f32(p, p, None, None, None, p, 1, 8, 2, 32, 64, 5, 5, 1, 1, 0, s))
        refused("fp16 Ho<=0", lib.seam_conv2d_f16(p, p, None, None, None, p, 1, 2, 8, 64, 64, 5, 5, 1, 1, 0, 0, s))
        refused("bx3 Ho<=0", lib.seam_conv2d_bx3(p, p, None, None, None, p, 1, 2, 8, 32, 64, 5, 5, 1, 1, 0, s))
        refused("sx Ho<=0", lib.seam_conv2d_sx(p, p, None, None, None, p, 1, 2, 8, 32, 64, 5, 5, 1, 1, 0, 6, s))
        refused("crop f32 taller than the grid", lib.seam_conv2d_crop_f32(p, p, None, None, p, 1, 8, 8, 32, 64, 3, 3, 1, 1, 9, 8, 0, s))
        refused("crop f32 wider than the grid", lib.seam_conv2d_crop_f32(p, p, None, None, p, 1, 8, 8, 32, 64, 3, 3, 2, 1, 4, 5, 0, s))
        refused("crop f16 larger than the grid", lib.seam_conv2d_crop_f16(p, p, None, None, p, 1, 8, 8, 64, 64, 3, 3, 1, 1, 8, 9, 0, s))
        refused("upres K=6", lib.seam_conv2d_upres_f32(p, p, None, None, p, p, 1, 8, 8, 32, 6, 1, 1, 1, 0, 4, 4, 0, s))
        refused("upres relu=2", lib.seam_conv2d_upres_f32(p, p, None, None, p, p, 1, 8, 8, 32, 64, 1, 1, 1, 0, 4, 4, 2, s))
        refused("upres without a residual", lib.seam_conv2d_upres_f32(p, p, None, None, None, p, 1, 8, 8, 32, 64, 1, 1, 1, 0, 4, 4, 0, s))
        refused("upres Ht=0", lib.seam_conv2d_upres_f32(p, p, None, None, p, p, 1, 8, 8, 32, 64, 1, 1, 1, 0, 0, 4, 0, s))
        refused("dual f32 (Ho-1)*stride2 == H2", lib.seam_conv2d_dual_f32(p, p, p, None, None, p, 1, 5, 5, 32, 8, 9, 64, 2, 64, 0, s))
        refused("dual f32 (Wo-1)*stride2 == W2", lib.seam_conv2d_dual_f32(p, p, p, None, None, p, 1, 5, 5, 32, 9, 8, 64, 2, 64, 0, s))
        refused("dual f32 C2=48", lib.seam_conv2d_dual_f32(p, p, p, None, None, p, 1, 5, 5, 32, 9, 9, 48, 2, 64, 0, s))
        refused("dual f32 C1=16", lib.seam_conv2d_dual_f32(p, p, p, None, None, p, 1, 5, 5, 16, 9, 9, 64, 2, 64, 0, s))
        refused("dual f16 (Ho-1)*stride2 == H2", lib.seam_conv2d_dual_f16(p, p, p, None, None, p, 1, 5, 5, 64, 8, 9, 64, 2, 64, 0, s))
        refused("dual f16 C2=48", lib.seam_conv2d_dual_f16(p, p, p, None, None, p, 1, 5, 5, 64, 9, 9, 48, 2, 64, 0, s))
        refused("dual f16 C2=96", lib.seam_conv2d_dual_f16(p, p, p, None, None, p, 1, 5, 5, 64, 9, 9, 96, 2, 64, 0, s))
        # the C entry of the dual form has no R argument: a 3x3 pack is turned away by ops.conv2d_dual before any launch
        pc3 = ops.pack_conv(torch.zeros(64, 64, 3, 3, device=dev), wino=False)
        tried[0] += 1
        try:
            ops.conv2d_dual(torch.zeros(1, 5, 5, 32, device=dev), torch.zeros(1, 5, 5, 32, device=dev), pc3)
            bad.append("dual with R=3")
        except ValueError:
            pass
        refused("sx terms=5", lib.seam_conv2d_sx(p, p, None, None, None, p, 1, 8, 8, 32, 64, 3, 3, 1, 1, 0, 5, s))
        torch.cuda.synchronize()
        for what in bad:
            fails.append(("refusals", what, "was not refused"))
            say("FAIL refusals", what, "was not refused")
        say(f"SUMMARY refusals cases {tried[0]} accepted {len(bad)} seconds {time.time() - t0:.1f}")

    runners = {"upres": run_upres, "crop": run_generic, "dual": run_dual, "f16dual": run_dual, "pack": run_pack}
    for fam in FAMILIES:
        if only and fam not in only:
            continue
        before = len(fails)
        t0 = time.time()
        cases = generate(fam, lib, seed)
        emax = el2max = e32max = 0.0
        emax16 = 0.0
        for c in cases:
            assert accepts(c), describe(c)
            say("START", fam, describe(c))
            r = runners.get(fam, run_generic)(fam, c)
            half_out = fam == "f16dual" or (fam == "f16" and not c.get("y_f32"))
            if r[0] == r[0]:
                if half_out:
                    emax16 = max(emax16, r[0])
                else:
                    emax = max(emax, r[0])
                el2max = max(el2max, r[1])
            if len(r) > 2 and r[2] == r[2]:
                e32max = max(e32max, r[2])
        torch.cuda.synchronize()
        counts = corner_counts(cases)
        line = f"SUMMARY {fam} cases {len(cases)} " + " ".join(f"{k} {v}" for k, v in sorted(counts.items()))
        if fam in ("f16", "f16dual"):
            line += f" max_err_f16out {emax16:.3e}"
        if fam != "f16dual":
            line += f" max_err {emax:.3e}"
        if fam == "bx3":
            line += f" max_err_l2 {el2max:.3e}"
        if fam in ("sx6", "sx9"):
            line += f" max_err_f32_kernel {e32max:.3e}"
        say(line + f" seconds {time.time() - t0:.1f}")
        say("KERNEL", fam, "failures", len(fails) - before)
    if not only or "refusals" in only:
        before = len(fails)
        refusals()
        say("KERNEL refusals failures", len(fails) - before)
    say("DONE failures", len(fails))
    for f in fails[:40]:
        say("FAILED", *f)
    return 1 if fails else 0


# ------------------------------------------------------------------------------------------------ the tests: read the child's output
@pytest.fixture(scope="module")
def sweep():
    """One child process runs every family (one ``import torch``); its stdout is what the tests below read."""
    return stress_kit.run_child([sys.executable, os.path.abspath(__file__), str(SEED)], WALL_S, ROOT)


def _family_ok(sweep, name):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    if name in FAMILIES:
        assert int(f["cases"]) >= FAMILIES[name][1], f
        for key, need in REQUIRED[name].items():
            assert int(f.get(key, 0)) >= need, (key, need, f)
        if "div_fast0" in REQUIRED[name]:
            assert int(f["div_fast0"]) == REQUIRED[name]["div_fast0"], f
    return f


def test_stress_igemm_f32(sweep):
    assert float(_family_ok(sweep, "f32")["max_err"]) <= TOL_F32


def test_stress_igemm_upres_f32(sweep):
    assert float(_family_ok(sweep, "upres")["max_err"]) <= TOL_F32


def test_stress_igemm_crop_f32(sweep):
    assert float(_family_ok(sweep, "crop")["max_err"]) <= TOL_F32


def test_stress_igemm_dual_f32(sweep):
    assert float(_family_ok(sweep, "dual")["max_err"]) <= TOL_F32


def test_stress_igemm_f16(sweep):
    f = _family_ok(sweep, "f16")
    assert float(f["max_err"]) <= TOL_F32 and float(f["max_err_f16out"]) <= TOL_F16


def test_stress_igemm_dual_f16(sweep):
    assert float(_family_ok(sweep, "f16dual")["max_err_f16out"]) <= TOL_F16


def test_stress_igemm_bx3(sweep):
    f = _family_ok(sweep, "bx3")
    assert float(f["max_err"]) <= TOL_BX3 and float(f["max_err_l2"]) <= TOL_BX3_L2


def test_stress_igemm_sx6(sweep):
    assert float(_family_ok(sweep, "sx6")["max_err"]) <= TOL_F32


def test_stress_igemm_sx9(sweep):
    assert float(_family_ok(sweep, "sx9")["max_err"]) <= TOL_F32


def test_stress_igemm_pack_modes(sweep):
    assert float(_family_ok(sweep, "pack")["max_err"]) <= TOL_F32


def test_stress_igemm_refusals(sweep):
    assert _family_ok(sweep, "refusals")["accepted"] == "0"


def test_stress_igemm_sweep_is_fast(sweep):
    """<= 90 s of sweep, measured inside the child family by family (process start-up and ``import torch`` excluded)."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    assert len(secs) == len(FAMILIES) + 1 and sum(secs) <= 90.0, secs


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
