"""The seeded case generator of the split-bf16 1x1 sweep (tests/stress_child_sxpc.py, tests/test_gpu_stress_sxpc.py): the seven
launch entries of ``sxpc_body`` (csrc/seam_pwsx.hip).  Pure Python: no torch, no device, nothing launched.

``cases(family, ncase, seed)`` is a pure function of its arguments.  Every case is served by construction -- nothing is drawn and
skipped against the library; tests/test_sxpc_stress_cases_host.py asks the library's predicates about every case of the list.

A case is steered, not hoped for.  Case ``i`` takes one entry of each of these schedules (their lengths are pairwise coprime, so a
hundred cases cross them):

  SIZES (11)  what the row count M = N Ho Wo is aimed at: 1, below a tile, a multiple of the tile, one row past / short of a
              multiple, at most eight tiles, fewer tiles than CUs with ragged XCD ranges, anything.  16 MiB of output are 256
              tiles, one per CU, so two cases in 33 take the larger budget on the smallest channel counts: a LONG WALK (more
              than three tiles per CU, the last round ragged) and a two-tile walk (between one and two tiles per CU);
  GEOS (7)    (second-source families) the output grid of one image: Ho Wo = 1, 2 .. 42 (a tile over more than three images),
              43 .. 127, >= 128 and no multiple of 128, Wo = 1, Ho = 1, one image -- the three image-lookup rules of ``sxpc_pixel``;
  channel counts by rotation (5, or 4 for sxpc64), ``stride2`` by rotation (3) and x2's slack by the next digit (3), the coarse
  map's ratio by rotation (5) with a fall-back where the grid cannot have it (an exact 2x ratio of a one-column grid).

Within a class the integers are drawn from ``random.Random`` seeded by (family, seed).  The rows N are solved for, not searched:
``_pick_n`` knows the set of N that meets a size target for a given Ho Wo and draws from it.

Sizes: no operand or output above 16 MiB and M <= 60 000; the six walks of a hundred cases (``long``) stay under 64 MiB.  The 64-output-channel entries
(``sxpc64``, ``stem_sxpc``) have one tile per 128 rows, so a walk of more than 3 x 256 tiles needs M > 98 304: their three long walks
have M <= 100 000 (still under 64 MiB), every other case of them M <= 60 000.

``classify(family, case, cus)`` names the classes a case belongs to; the child recounts with the device's CU count.  ``REQUIRED``
holds the least count of each class in a list of 100."""
import math
import random

BM = 128                    # rows per tile
CK = 64                     # channels per chunk
CUS, XCDS = 256, 8          # the host-side grid constants (MI355X); the child recounts with the device's
BUDGET = 16 << 20           # bytes of any operand or output
LONG_BUDGET = 64 << 20      # ... of a long walk
M_MAX = 60_000
M_MAX_LONG64 = 100_000      # long walks of the 64-output-channel entries: see the header

FAMILIES = ("sxpc", "sxpc_short", "sxpc_dual", "sxpc_dual_short", "sxpc_up", "sxpc64", "stem_sxpc")
SECOND = ("sxpc_dual", "sxpc_dual_short", "sxpc_up", "stem_sxpc")       # families with a second source under an [N, Ho, Wo] grid
RESIDUAL = ("sxpc", "sxpc_short", "sxpc64")                             # entries that take a residual
C_LONG = (256, 320, 384, 512, 1024)
K_LONG = (128, 256, 384, 512)
C_64 = (128, 192, 256, 512)

SIZES = ("m1", "lt128", "mult", "pm1", "le8", "sub", "free", "free", "mult", "pm1", "sub")
GEOS = ("h1", "small", "mid", "big", "wo1", "ho1", "n1")
LONG_EVERY, LONG_AT, WALK_AT = 33, 32, 16   # cases 32, 65, 98 of a hundred are long walks, cases 16, 49, 82 two-tile walks
LONG_GEOS = ("small", "mid", "big")
RATIOS = ("ratio2", "frac", "ratio1", "coarse", "one")
RANGES = {"h1": (1, 1), "small": (2, 42), "mid": (43, 127), "big": (128, 1200)}

T_ROWS = ("M<128", "M%128==0", "M%128in{1,127}", "M==1")
T_GRID = ("tiles<=8", "tiles<CUs&tiles%8!=0", "tiles>3CUs&tiles%CUs!=0")
T_SECOND = ("HoWo==1", "2<=HoWo<=42", "43<=HoWo<128", "HoWo>=128&HoWo%128!=0", "Wo==1", "Ho==1", "N==1")
T_EPI = ("epi-none", "epi-shift", "epi-scale+shift", "relu0", "relu1")


def tiles_of(case):
    return -(-case["M"] // BM) * max(case["K"] // 128, 1)


def classify(family, case, cus=CUS):
    """-> tuple of class tags of ``case``; ``cus``: the CU count the grid classes are counted with"""
    m, tiles, nch = case["M"], tiles_of(case), case["nchunks"]
    t = []
    if m < BM:
        t.append("M<128")
    if m % BM == 0:
        t.append("M%128==0")
    if m % BM in (1, BM - 1):
        t.append("M%128in{1,127}")
    if m == 1:
        t.append("M==1")
    if tiles <= XCDS:
        t.append("tiles<=8")
    if tiles < cus and tiles % XCDS != 0:
        t.append("tiles<CUs&tiles%8!=0")
    if tiles > 3 * cus and tiles % cus != 0:
        t.append("tiles>3CUs&tiles%CUs!=0")
    if cus < tiles < 2 * cus:
        t.append("CUs<tiles<2CUs")
    t.append("nchunks-odd" if nch % 2 else "nchunks-even")
    if nch in (2, 3):
        t.append(f"nchunks=={nch}")
    if family in SECOND:
        n, ho, wo = case["N"], case["Ho"], case["Wo"]
        hw = ho * wo
        if hw == 1:
            t.append("HoWo==1")
        elif hw <= 42:
            t.append("2<=HoWo<=42")
        elif hw < BM:
            t.append("43<=HoWo<128")
        elif hw % BM != 0:
            t.append("HoWo>=128&HoWo%128!=0")
        if wo == 1:
            t.append("Wo==1")
        if ho == 1:
            t.append("Ho==1")
        if n == 1:
            t.append("N==1")
    if family in ("sxpc_dual", "sxpc_dual_short"):
        s, h2, w2 = case["stride2"], case["H2"], case["W2"]
        t.append(f"stride2=={s}")
        hmin, wmin = (case["Ho"] - 1) * s + 1, (case["Wo"] - 1) * s + 1
        if h2 == hmin and w2 == wmin:
            t.append("x2-min")
        if h2 > hmin and w2 > wmin:
            t.append("x2-slack")
    if family == "sxpc_up":
        ho, wo, rh, rw = case["Ho"], case["Wo"], case["rH"], case["rW"]
        if ho == 2 * rh and wo == 2 * rw:
            t.append("ratio2")
        if rh < ho and rw < wo and ho % rh and wo % rw:
            t.append("ratio-frac")
        if rh == ho and rw == wo:
            t.append("ratio1")
        if rh > ho and rw > wo:
            t.append("coarse>out")
        if rh == 1 or rw == 1:
            t.append("rH==1|rW==1")
    t.append("epi-scale+shift" if case["scale"] else "epi-shift" if case["shift"] else "epi-none")
    if case["res"]:
        t.append("res")
    t.append(f"relu{case['relu']}")
    return tuple(t)


def _required(family):
    """the least count of each class among 100 cases.  Set by the issue: three long walks, ten of each of the four Ho Wo classes.
    The others are what the schedules give with room to spare: a class aimed at by one entry in eleven (or one in seven, five,
    three) of a hundred cases is met at least 5 times after the fall-backs; the epilogue draws are independent with p >= 1/3."""
    r = {"M<128": 8, "M%128==0": 8, "M%128in{1,127}": 8, "M==1": 3, "tiles<=8": 8, "tiles<CUs&tiles%8!=0": 8, "tiles>3CUs&tiles%CUs!=0": 3,
         "CUs<tiles<2CUs": 3,
         "epi-none": 10, "epi-shift": 10, "epi-scale+shift": 10, "relu0": 20, "relu1": 20}
    if family in ("sxpc", "sxpc_dual", "sxpc_up"):
        r.update({"nchunks-odd": 10, "nchunks-even": 10})
    if family in ("sxpc_short", "sxpc_dual_short", "sxpc64"):
        r["nchunks==2"] = 100 if family != "sxpc64" else 10
    if family == "stem_sxpc":
        r["nchunks==3"] = 100
    if family in RESIDUAL:
        r["res"] = 15
    if family in SECOND:
        r.update({"HoWo==1": 10, "2<=HoWo<=42": 10, "43<=HoWo<128": 10, "HoWo>=128&HoWo%128!=0": 10, "Wo==1": 10, "Ho==1": 10, "N==1": 10})
    if family == "sxpc_dual":
        r.update({"stride2==1": 20, "stride2==2": 20, "stride2==3": 20, "x2-min": 15, "x2-slack": 15})
    if family == "sxpc_dual_short":
        r.update({"stride2==1": 100, "x2-min": 15, "x2-slack": 15})
    if family == "sxpc_up":
        r.update({"ratio2": 5, "ratio-frac": 5, "ratio1": 5, "coarse>out": 5, "rH==1|rW==1": 5})
    return r


REQUIRED = {f: _required(f) for f in FAMILIES}


# ------------------------------------------------------------------------------------------------ solving for the rows
def _n_for_mtiles(rng, hw, mt, cap):
    """an N with ceil(N hw / 128) == mt and N <= cap, or None"""
    lo, hi = (BM * (mt - 1)) // hw + 1, min(cap, (BM * mt) // hw)
    return rng.randint(lo, hi) if lo <= hi else None


def _pick_n(rng, target, hw, cap, tn, one_image):
    """an N in [1, cap] (``one_image``: 1) whose M = N hw meets ``target``, drawn from the set of those that do; None: there is none"""
    if cap < 1:
        return None
    if one_image:
        cap = 1
    if target == "m1":
        return 1 if hw == 1 else None
    if target == "lt128":
        hi = min(cap, (BM - 1) // hw)
        return rng.randint(1, hi) if hi >= 1 else None
    if target == "mult":
        q = BM // math.gcd(hw, BM)
        hi = min(cap // q, 40)
        return q * rng.randint(1, hi) if hi >= 1 else None
    if target == "pm1":
        if hw % 2 == 0:
            return None
        inv = pow(hw, -1, BM)
        firsts = [r for r in (inv % BM, (BM - inv) % BM) if 1 <= r <= cap]
        if not firsts:
            return None
        r = rng.choice(firsts)
        return r + BM * rng.randint(0, min((cap - r) // BM, 20))
    if target == "le8":
        hi = min(cap, BM * (XCDS // tn) // hw)
        return rng.randint(1, hi) if hi >= 1 else None
    if target in ("sub", "walk", "long"):
        if target == "sub":
            mts = [mt for mt in range(1, (CUS - 1) // tn + 1) if (mt * tn) % XCDS != 0]
        elif target == "walk":              # some blocks walk two tiles, the others one
            mts = list(range(CUS // tn + 1, 2 * CUS // tn))
        else:
            first = 3 * CUS // tn + 1
            mts = [mt for mt in range(first, first + 24) if (mt * tn) % CUS != 0]
        rng.shuffle(mts)
        for mt in mts:
            n = _n_for_mtiles(rng, hw, mt, cap)
            if n is not None:
                return n
        return None
    assert target == "free", target
    return rng.randint(1, min(cap, max(1, 4096 // hw))) if rng.random() < 0.5 else rng.randint(1, cap)


def _draw_range(rng, lo, hi):
    """(Ho, Wo) with lo <= Ho Wo <= hi, either axis the long one"""
    wo = rng.randint(1, min(hi, 48))
    ho = rng.randint(-(-lo // wo), max(hi // wo, -(-lo // wo)))
    if ho * wo > hi:                        # (cannot happen for the ranges of RANGES; kept as the rule)
        ho = hi // wo
    return (ho, wo) if rng.random() < 0.5 else (wo, ho)


def _draw_grid(rng, geo):
    """one image's output grid of class ``geo`` -> (Ho, Wo, one_image)"""
    if geo in ("wo1", "ho1"):
        lo, hi = RANGES[rng.choice(("small", "mid", "big", "big"))]
        length = rng.randint(lo, min(hi, 700))
        if lo == BM and length % BM == 0:
            length += 1
        return (length, 1, False) if geo == "wo1" else (1, length, False)
    cls = rng.choice(("h1", "small", "mid", "big")) if geo == "n1" else geo
    ho, wo = _draw_range(rng, *RANGES[cls])
    if cls == "big" and (ho * wo) % BM == 0:
        ho += 1
    return ho, wo, geo == "n1"


# ------------------------------------------------------------------------------------------------ per family: channels, extras, bytes
def _channels(family, rng, i, long):
    """-> dict of the channel integers of case i"""
    if family in ("sxpc", "sxpc_up"):
        c = 256 if long else C_LONG[i % 5]
        return {"C": c, "K": rng.choice((256, 512)) if long else rng.choice(K_LONG)}
    if family == "sxpc_short":
        return {"C": 128, "K": rng.choice((256, 512)) if long else rng.choice(K_LONG)}
    if family == "sxpc_dual":
        c = 256 if long else C_LONG[i % 5]
        n1 = rng.randint(1, c // CK - 1)
        return {"C": c, "C1": n1 * CK, "C2": c - n1 * CK, "K": rng.choice((256, 512)) if long else rng.choice(K_LONG)}
    if family == "sxpc_dual_short":
        return {"C": 128, "C1": 64, "C2": 64, "K": rng.choice((256, 512)) if long else rng.choice(K_LONG)}
    if family == "sxpc64":
        return {"C": 128 if long else C_64[i % 4], "K": 64}
    return {"C": 192, "K": 64}             # stem_sxpc


def _extras(family, rng, i, ho, wo, ratio, long):
    """the second source's own integers for the grid (Ho, Wo), or None where the grid cannot have what case i asks for"""
    if family == "sxpc_dual" or family == "sxpc_dual_short":
        s = 1 + i % 3 if family == "sxpc_dual" and not long else 1         # (a long walk: x2 no larger than it must be)
        mode = 2 if long else (i // 3) % 3  # both minimal | both with slack | drawn per axis
        slack = [0, 0] if mode == 0 else [rng.randint(1, 3), rng.randint(1, 3)] if mode == 1 else [rng.randint(0, 2), rng.randint(0, 2)]
        return {"stride2": s, "H2": (ho - 1) * s + 1 + slack[0], "W2": (wo - 1) * s + 1 + slack[1]}
    if family == "sxpc_up":
        if ratio == "ratio2":
            return {"rH": ho // 2, "rW": wo // 2} if ho % 2 == 0 and wo % 2 == 0 else None
        if ratio == "frac":
            hs = [r for r in range(2, ho) if ho % r]
            ws = [r for r in range(2, wo) if wo % r]
            return {"rH": rng.choice(hs), "rW": rng.choice(ws)} if hs and ws else None
        if ratio == "ratio1":
            return {"rH": ho, "rW": wo}
        if ratio == "coarse":
            return {"rH": ho + rng.randint(1, 5), "rW": wo + rng.randint(1, 5)}
        rh, rw = rng.randint(1, ho), rng.randint(1, wo)       # "one": a coarse map of one row or one column
        return {"rH": 1, "rW": rw} if rng.random() < 0.5 else {"rH": rh, "rW": 1}
    return {}


def _n_cap(family, ch, ex, ho, wo, budget, m_max):
    """the largest N for which every operand and the output of (ch, ex, Ho, Wo) stay within ``budget`` bytes and M within m_max"""
    hw = ho * wo
    per_image = [4 * hw * ch["K"]]                                         # y (and the residual)
    if family in ("sxpc", "sxpc_short", "sxpc64", "sxpc_up"):
        per_image.append(4 * hw * ch["C"])
    if family in ("sxpc_dual", "sxpc_dual_short"):
        per_image += [4 * hw * ch["C1"], 4 * ex["H2"] * ex["W2"] * ch["C2"]]
    if family == "sxpc_up":
        per_image.append(4 * ex["rH"] * ex["rW"] * ch["K"])
    if family == "stem_sxpc":
        per_image.append(48 * (ho + 3) * (wo + 3))
    return min(budget // max(per_image), m_max // hw)


def operand_bytes(family, case):
    """{name: bytes} of every operand and the output of ``case`` (what the budgets are about)"""
    m, c, k = case["M"], case["C"], case["K"]
    b = {"y": 4 * m * k}
    if case["res"]:
        b["res"] = 4 * m * k
    if family in ("sxpc", "sxpc_short", "sxpc64", "sxpc_up"):
        b["x"] = 4 * m * c
    if family in ("sxpc_dual", "sxpc_dual_short"):
        b["x1"] = 4 * m * case["C1"]
        b["x2"] = 4 * case["N"] * case["H2"] * case["W2"] * case["C2"]
    if family == "sxpc_up":
        b["top"] = 4 * case["N"] * case["rH"] * case["rW"] * k
    if family == "stem_sxpc":
        b["xp"] = 48 * case["N"] * (case["Ho"] + 3) * (case["Wo"] + 3)
    return b


def m_limit(family, case):
    return M_MAX_LONG64 if case["long"] and case["index"] % LONG_EVERY == LONG_AT and family in ("sxpc64", "stem_sxpc") else M_MAX


# ------------------------------------------------------------------------------------------------ the generator
def _geometry(family, rng, i, ch, long):
    """-> (N, Ho, Wo, extras) of case i: its size target met where the grid class allows, relaxed to "free" where not"""
    tn = max(ch["K"] // 128, 1)
    target = ("long" if i % LONG_EVERY == LONG_AT else "walk") if long else SIZES[i % len(SIZES)]
    budget = LONG_BUDGET if long else BUDGET
    m_max = M_MAX_LONG64 if target == "long" and family in ("sxpc64", "stem_sxpc") else M_MAX
    if family not in SECOND:
        for tg in (target, "free"):
            n = _pick_n(rng, tg, 1, _n_cap(family, ch, {}, 1, 1, budget, m_max), tn, False)
            if n is not None:
                return n, 1, 1, {}
    geo = LONG_GEOS[(i // LONG_EVERY + (i % LONG_EVERY == WALK_AT)) % 3] if long else GEOS[i % len(GEOS)]
    ratios = [RATIOS[(i + j) % len(RATIOS)] for j in range(len(RATIOS))] if family == "sxpc_up" else [None]
    for tg in (target,) if long else (target, "free"):
        for ratio in ratios:                # (sxpc_up: the case's own ratio first, then the next one the grid can have)
            for _ in range(200):
                if tg == "m1" and geo in ("h1", "wo1", "ho1", "n1"):
                    ho, wo, one = 1, 1, geo == "n1"     # one row: the 1 x 1 grid of these classes
                else:
                    ho, wo, one = _draw_grid(rng, geo)
                ex = _extras(family, rng, i, ho, wo, ratio, long)
                if ex is None:
                    continue
                n = _pick_n(rng, tg, ho * wo, _n_cap(family, ch, ex, ho, wo, budget, m_max), tn, one)
                if n is not None:
                    return n, ho, wo, ex
    raise AssertionError((family, i, target, geo))


def cases(family, ncase, seed):
    """-> list of ``ncase`` dicts: the entry's integers, the epilogue choice, a data seed, ``long`` and the class tags"""
    assert family in FAMILIES, family
    rng = random.Random(f"sxpc-stress {family} {seed}")
    out = []
    for i in range(ncase):
        long = i % LONG_EVERY in (LONG_AT, WALK_AT)        # the larger budget, the smallest channel counts
        ch = _channels(family, rng, i, long)
        n, ho, wo, ex = _geometry(family, rng, i, ch, long)
        mode = rng.choice(("none", "shift", "scale+shift"))
        case = {"family": family, "index": i, "M": n * ho * wo, "nchunks": ch["C"] // CK, "long": long,
                "scale": mode == "scale+shift", "shift": mode != "none", "res": family in RESIDUAL and rng.random() < 0.4,
                "relu": rng.randint(0, 1), "data_seed": rng.randrange(1 << 30)}
        case.update(ch)
        if family in SECOND:
            case.update({"N": n, "Ho": ho, "Wo": wo})
            case.update(ex)
        case["tags"] = classify(family, case)
        out.append(case)
    return out


def describe(case):
    keys = ("M", "N", "Ho", "Wo", "C", "C1", "C2", "K", "H2", "W2", "stride2", "rH", "rW")
    epi = ("scale+shift" if case["scale"] else "shift" if case["shift"] else "none") + ("+res" if case["res"] else "")
    return f"#{case['index']} " + " ".join(f"{k}={case[k]}" for k in keys if k in case) + f" epi={epi} relu={case['relu']}"


def count_tags(tag_lists):
    counts = {}
    for tags in tag_lists:
        for t in tags:
            counts[t] = counts.get(t, 0) + 1
    return counts
