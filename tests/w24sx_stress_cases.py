"""The seeded case generator of the split-bf16 Winograd sweep (tests/stress_child_w24sx.py, tests/test_gpu_stress_w24sx.py):
``conv3x3_wino24sx`` (csrc/seam_wino24sx.hip) and, on the same operands, the fp32 F(2x4) kernels.  Pure Python: no torch, no
device, nothing launched.

``cases(ncase, seed, layout)`` is a pure function of its arguments; ``layout(n, h, w, c, k, pad) -> dict | None`` is
``w24_layout_cases.query`` bound to the library (``seam_wino24_layout`` is host code).  A case is steered, not drawn and skipped:

  * ``scan(layout)`` asks the library for the layout of every tile grid with tiles_x <= 40, tiles_y <= 60 at N = 1 and N = 8
    (4 800 host queries, a fifth of a second) and files each grid under its layout class and the HS class of its first region.
  * Case ``i`` takes one entry of each of these schedules, whose lengths are pairwise coprime (28, 11, 9, 13, 5, 19, 17, 23):
      LAYOUTS x HS (7 x 4)  one region | main + right | main + bottom | main + right + bottom | stacked G = 1 | G >= 2 | G >= 4,
                            with HS = 9, 5, 3, run-time by rotation inside the class.  A pair the scan shows empty is named in
                            UNREACHABLE and replaced by ``_reachable``: the next HS of its class; the stacked G = 1 class, empty
                            in every HS, by the ROI heads' form -- stacked G >= 4 at HS 3, a map of one or two tiles -- aimed
                            at N >= 512, since only such maps hold 512 images of 512 channels within the budget;
      SIZES (11)            the grid patch_blocks x K / 64: one block (K is then 64), <= 8 blocks, fewer blocks than CUs with
                            blocks % 8 != 0 (K >= 512 makes every grid a multiple of 8: then fewer blocks than CUs), N >= 64,
                            N >= 512, free; cases 16, 49, 82 of a hundred walk between one and two blocks per CU and cases 32,
                            65, 98 more than three (LONG WALKS, no multiple of the CU count);
      C (9), K (13)         C from (64 .. 512), K from (64 .. 1024) by rotation; C = 1024 is left out (no 3x3 layer has it);
      PADS (5), EDGES (19)  pad 0 | 1; Wo % 4 and the parity of Ho;
      EPILOGUES (17)        none, shift, scale + shift, + residual, + ReLU, residual + ReLU, mask (relu = 2);
      PACKS (23)            mode 0 with Cin == Cstore; three slots Cin = Cstore - 8 j; two slots mode 2 (rotated taps, swapped
                            channels: the reference is the transposed convolution).
  * N is solved for: from the blocks per image of the scan the generator knows which N meet the size target, and asks the
    library about those only -- the layout of every candidate is checked (a larger batch can turn a region layout into a stacked
    one), and the first that has the case's layout pair and meets the target is taken.  A target a pair cannot have (one block
    with three regions, N >= 512 with a 100-pixel-wide map) relaxes along FALLBACK; the layout pair never does.

Budgets: x, the residual and y at most 16 MiB each (the six walks: 64 MiB, at C <= 128) and N <= 4096.  The weights are what the
channel rotation makes them (18 MiB of fp32 at 512 -> 1024).

``classify(case, lay, cus)`` names the classes of a case from the layout the library reports; the child recounts with the
device's CU count.  ``REQUIRED`` holds the least count of each class in a list of 100: conditions, not measurements."""
import random

import w24_layout_cases as T

CUS, XCDS = 256, 8          # the host-side grid constants (MI355X); the child recounts with the device's
BUDGET = 16 << 20           # bytes of x, of the residual and of y
LONG_BUDGET = 64 << 20      # ... of the six walks
N_MAX = 4096
SCAN = dict(tiles_x=40, tiles_y=60, images=(1, 8))

HS_CLASSES = (9, 5, 3, T.RT)
LAYOUTS = ("one", "mainR", "mainB", "mainRB", "stackG1", "stackG2", "stackG4")
# Pairs no grid of the scan has.  stackG1: a stacked block that never spans two images has TY | tiles_y, and then the uniform region
# layout with the same patch needs no more blocks -- choose_layout takes the stacked form only where it saves one.  stackG4 / 9: four
# images in 32 tile slots leave a map 7 tiles wide one tile row per image, and one row of 7 or 8 tiles is a region of its own at
# equal cost.  mainR / 3: a main region of one or two tile columns leaves a right strip no block cheaper than the uniform layout.
UNREACHABLE = {("stackG1", 9), ("stackG1", 5), ("stackG1", 3), ("stackG1", T.RT), ("stackG4", 9), ("mainR", 3)}

SIZES = ("one", "le8", "sub", "n512", "sub", "n64", "free", "n512", "sub", "n512", "n64")
FALLBACK = {"one": "le8", "le8": "sub", "sub": "lt", "lt": "free", "n512": "n64", "n64": "free", "free": None, "walk": None, "long": None}
LONG_EVERY, LONG_AT, WALK_AT = 33, 32, 16
CS = (64, 128, 192, 256, 320, 384, 512, 256, 512)
KS = (64, 128, 192, 256, 512, 1024, 64, 128, 192, 256, 512, 1024, 1024)
PADS = (0, 1, 0, 1, 1)
EDGES = tuple((r, odd) for r in (0, 1, 2, 3) for odd in (0, 1)) * 2 + ((1, 1), (3, 0), (2, 1))       # (Wo % 4, Ho odd)
EPILOGUES = ("none", "shift", "scale_shift", "residual", "relu", "residual_relu", "mask")
EPI_SCHEDULE = EPILOGUES * 2 + ("mask", "residual_relu", "residual")
EPI_FLAGS = {  # (scale, shift, residual operand, relu)
    "none": (0, 0, 0, 0), "shift": (0, 1, 0, 0), "scale_shift": (1, 1, 0, 0), "residual": (1, 1, 1, 0), "relu": (1, 1, 0, 1),
    "residual_relu": (1, 1, 1, 1), "mask": (1, 1, 1, 2)}
PACKS = 23
PACK_SHORT, PACK_MODE2 = (0, 7, 14), (3, 13)         # slots of the 23: Cin < Cstore | mode 2


def layout_pair(lay, n, h, w, pad):
    """(layout class, HS class of the first region) of a layout the library reported"""
    sig = T.signature(lay, n, h, w, pad)
    if sig["stack"]:
        cls = "stackG1" if sig["G"] == 1 else "stackG2" if sig["G"] < 4 else "stackG4"
    else:
        cls = {"": "one", "R": "mainR", "B": "mainB", "RB": "mainRB"}[sig["strips"]]
    return cls, sig["hs"][0]


def scan(layout):
    """{(layout class, HS class): [(tiles_x, tiles_y, scan N, patch blocks), ...]} over every tile grid of SCAN"""
    pool = {}
    for n in SCAN["images"]:
        for ty in range(1, SCAN["tiles_y"] + 1):
            for tx in range(1, SCAN["tiles_x"] + 1):
                lay = layout(n, 2 * ty, 4 * tx, 64, 64, 1)
                pool.setdefault(layout_pair(lay, n, 2 * ty, 4 * tx, 1), []).append((tx, ty, n, lay["patch_blocks"]))
    return pool


def _reachable(cls, hs, i):
    """the pair case i runs: its own, or the stand-in of an UNREACHABLE one"""
    if cls == "stackG1":                    # the ROI heads' form, a few tile slots per image; a walk needs a larger map
        return ("stackG2", hs if hs != 3 else 5) if i % LONG_EVERY in (LONG_AT, WALK_AT) else ("stackG4", 3)
    at = HS_CLASSES.index(hs)
    for j in range(4):
        if (cls, HS_CLASSES[(at + j) % 4]) not in UNREACHABLE:
            return cls, HS_CLASSES[(at + j) % 4]
    raise AssertionError(cls)


def grid_blocks(lay, k):
    """blocks of the rule's launch: patch blocks x n-tiles of 64 channels"""
    return lay["patch_blocks"] * (k // 64)


def _meets(target, n, blocks):
    if target == "one":
        return blocks == 1
    if target == "le8":
        return blocks <= XCDS
    if target == "sub":
        return blocks < CUS and blocks % XCDS != 0
    if target == "lt":
        return blocks < CUS
    if target == "walk":
        return CUS < blocks < 2 * CUS
    if target == "long":
        return blocks > 3 * CUS and blocks % CUS != 0
    if target == "n64":
        return n >= 64
    if target == "n512":
        return n >= 512
    return True


def _block_range(target):
    return {"one": (1, 1), "le8": (1, XCDS), "sub": (1, CUS - 1), "lt": (1, CUS - 1), "walk": (CUS + 1, 2 * CUS - 1), "long": (3 * CUS + 1, 3 * CUS + 64)}[target]


def _candidates(rng, target, entry, tn, cap):
    """the N worth asking the library about: those that meet ``target`` by the scan's blocks per image, at most 24 of them"""
    _, _, n_scan, pb = entry
    if n_scan == 1:
        return [1]
    if cap < 2:
        return []
    if target in ("n64", "n512", "free"):
        lo = {"n64": 64, "n512": 512, "free": 2}[target]
        if lo > cap:
            return []
        out = {min(cap, int(lo * (cap / lo) ** rng.random())) for _ in range(6)}       # log-uniform: small batches as likely as large
        return sorted(out, key=lambda v: rng.random())
    lo, hi = _block_range(target)
    per_image = pb / n_scan
    nlo, nhi = max(2, int(lo / tn / per_image) - 1), min(cap, int(hi / tn / per_image) + 2)
    if nlo > nhi:
        return []
    span = list(range(nlo, nhi + 1))
    rng.shuffle(span)
    return span[:24]


def _solve(layout, rng, pool, pair, target, geo, budget):
    """-> (n, h, w) whose layout is ``pair`` and which meets ``target``, or None"""
    c, k, pad, (wo_mod, ho_odd) = geo
    entries = list(pool.get(pair, ()))
    rng.shuffle(entries)
    if target in ("n64", "n512"):                       # the smallest maps hold the largest batches
        entries.sort(key=lambda e: e[0] * e[1])
        entries = [e for e in entries if e[2] > 1][:24]
        rng.shuffle(entries)
    for entry in entries[:48]:
        tx, ty = entry[:2]
        wo, ho = 4 * (tx - 1) + (wo_mod or 4), 2 * ty - ho_odd
        h, w = ho + 2 - 2 * pad, wo + 2 - 2 * pad
        cap = min(N_MAX, budget // max(4 * h * w * c, 4 * ho * wo * k))
        for n in _candidates(rng, target, entry, k // 64, cap):
            if n > cap:
                continue
            lay = layout(n, h, w, c, k, pad)
            if lay is not None and layout_pair(lay, n, h, w, pad) == pair and _meets(target, n, grid_blocks(lay, k)):
                return n, h, w
    return None


def cases(ncase, seed, layout):
    """-> list of ``ncase`` dicts: the launch's integers, the pack form, the epilogue, a data seed, the layout pair and the tags"""
    rng = random.Random(f"w24sx-stress {seed}")
    pool = scan(layout)
    out = []
    for i in range(ncase):
        pair = _reachable(LAYOUTS[i % 7], HS_CLASSES[(i // 7) % 4], i)
        long = i % LONG_EVERY in (LONG_AT, WALK_AT)
        target = ("long" if i % LONG_EVERY == LONG_AT else "walk") if long else SIZES[i % len(SIZES)]
        if LAYOUTS[i % 7] == "stackG1" and not long:
            target = "n512"                 # the stand-ins of the empty class are the cases that can hold the largest batches
        k = KS[i % len(KS)]
        c = (128 if k >= 256 else 64) if long else CS[i % len(CS)]            # a walk: x no larger than y
        pad, edge = PADS[i % len(PADS)], EDGES[i % len(EDGES)]
        found = None
        while found is None:
            kk = 64 if target == "one" else k
            found = _solve(layout, rng, pool, pair, target, (c, kk, pad, edge), LONG_BUDGET if long else BUDGET)
            if found is None:
                assert FALLBACK[target] is not None, (i, pair, target, c, k)
                target = FALLBACK[target]
        n, h, w = found
        epi = EPI_SCHEDULE[i % len(EPI_SCHEDULE)]
        slot = i % PACKS
        case = {"index": i, "n": n, "h": h, "w": w, "c": c, "k": kk, "pad": pad, "epilogue": epi, "long": long, "target": target,
                "cin": c - 8 * rng.randint(1, 7) if slot in PACK_SHORT else c, "mode": 2 if slot in PACK_MODE2 else 0,
                "pair": pair, "data_seed": rng.randrange(1 << 30)}
        case["tags"] = classify(case, layout(n, h, w, c, kk, pad))
        out.append(case)
    return out


def operand_bytes(case):
    """{name: bytes} of the activations of ``case`` (what the budgets are about)"""
    ho, wo = case["h"] + 2 * case["pad"] - 2, case["w"] + 2 * case["pad"] - 2
    b = {"x": 4 * case["n"] * case["h"] * case["w"] * case["c"], "y": 4 * case["n"] * ho * wo * case["k"]}
    if EPI_FLAGS[case["epilogue"]][2]:
        b["res"] = b["y"]
    return b


def pair_tag(pair):
    return f"lay:{pair[0]}/hs{'rt' if pair[1] == T.RT else pair[1]}"


def classify(case, lay, cus=CUS):
    """-> tuple of class tags of ``case`` laid out as ``lay``; ``cus``: the CU count the grid classes are counted with"""
    n, h, w, c, k, pad = (case[key] for key in ("n", "h", "w", "c", "k", "pad"))
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    blocks = grid_blocks(lay, k)
    t = [pair_tag(layout_pair(lay, n, h, w, pad)), f"C={c}", f"K={k}", f"pad{pad}", f"Wo%4={wo % 4}", "Ho-odd" if ho % 2 else "Ho-even",
         f"epi:{case['epilogue']}"]
    if c >= 256:
        t.append("C>=256")
    if k >= 512:
        t.append("K>=512")
    if n >= 64:
        t.append("N>=64")
    if n >= 512:
        t.append("N>=512")
    if lay["stack"] and lay["patch_blocks"] >= 8:
        t.append("stacked&patch-blocks>=8")
    if blocks == 1:
        t.append("blocks==1")
    if blocks <= XCDS:
        t.append("blocks<=8")
    if blocks % XCDS != 0:
        t.append("blocks%8!=0")
    if blocks < cus:
        t.append("blocks<CUs")
    if cus < blocks < 2 * cus:
        t.append("CUs<blocks<2CUs")
    if blocks > 3 * cus and blocks % cus != 0:
        t.append("long-walk")
    if case["epilogue"] == "mask":
        t.append("mask")
    if case["cin"] < c:
        t.append("Cin<Cstore")
    if case["mode"] == 2:
        t.append("mode2")
    return tuple(t)


def _required():
    """The issue's floors.  The pairs: 7 x 4 nominal pairs over 100 cases are met 3 or 4 times each, a stand-in adds to its own."""
    r = {pair_tag((cls, hs)): 3 for cls in LAYOUTS for hs in HS_CLASSES if (cls, hs) not in UNREACHABLE}
    r.update({f"C={c}": 10 for c in set(CS)})
    r.update({f"K={k}": 10 for k in set(KS)})
    r.update({f"epi:{e}": 8 for e in EPILOGUES})
    r.update({"C>=256": 40, "K>=512": 25, "N>=64": 20, "N>=512": 8, "stacked&patch-blocks>=8": 8, "blocks%8!=0": 20, "blocks<CUs": 20,
              "long-walk": 3, "mask": 8, "Cin<Cstore": 10, "mode2": 6, "pad0": 30, "pad1": 30})
    # not in the issue's table, from the schedules: three two-block walks; 19 edge slots over 100 cases give every Wo % 4 four
    # slots (>= 20 cases) and either parity of Ho nine (>= 45)
    r.update({"CUs<blocks<2CUs": 3, "Wo%4=0": 20, "Wo%4=1": 20, "Wo%4=2": 20, "Wo%4=3": 20, "Ho-odd": 45, "Ho-even": 45})
    return r


REQUIRED = _required()


def describe(case):
    keys = ("n", "h", "w", "c", "k", "pad", "cin", "mode")
    return f"#{case['index']} " + " ".join(f"{key}={case[key]}" for key in keys) + f" epi={case['epilogue']} {pair_tag(case['pair'])}"


def count_tags(tag_lists):
    counts = {}
    for tags in tag_lists:
        for t in tags:
            counts[t] = counts.get(t, 0) + 1
    return counts
