"""The child of ``test_gpu_stress_w24sx.py``: ``python stress_child_w24sx.py NCASE SEED [family ...]`` runs the seeded cases of
``w24sx_stress_cases.py`` through ``seam_conv3x3_wino24sx_f32`` (family ``w24sx``) and, on the same operands,
``seam_conv3x3_wino24_f32`` in whatever form its rule picks (family ``w24f32``), and prints the lines ``stress_kit.family_ok``
reads.  Importing it launches nothing; ``normal``, ``reference64`` and ``check`` are plain functions on tensors of any device
(tests/test_w24sx_stress_cases_host.py runs them on the CPU).

Per case:
  * inputs N(0, 1) on the case's data seed: ``normal`` is ``synth.normal`` in torch integers, so that a hundred cases of up to
    16 M values are drawn on the device (the host test holds it against ``synth.normal`` bit for bit); weights scaled by
    1 / sqrt(9 C).  x, the residual or mask, scale and shift each lie between two runs of NAN_AROUND bytes of NaN, the second
    directly behind the last element: a load one pixel outside an image at either end of the batch shows as a non-finite output, and
    a load from a neighbouring image that leaks into a result fails the image check below;
  * Cin < Cstore: the channels of x beyond Cin hold PAD_FILL = 3e4 and the pack zero-fills their weights.  (Not NaN: the kernels
    multiply what they load, and 0 x NaN is NaN in every IEEE product -- the contract of include/seam_hip.h is "pad channels
    zero-weighted", not "not read".  A finite value that large shows any weight that is not exactly zero as a gross error.)
  * every launch goes through ``stress_kit.twice``: two launches onto NaN and 3e4 poison between guards, bit-identical;
  * one image j = data_seed % N launched alone equals image j of the batch bit for bit (where the batch is stacked the lone image
    has another layout, asserted from the query);
  * the float64 reference is ``reference64`` on the device: nine shifted float64 matmuls (no per-shape MIOpen search) and the
    epilogue in float64; mode 2 is the transposed convolution, ``relu = 2`` the mask;
  * ``w24f32``: e_w24 <= 3e-5 (TOL_W24 of tests/test_gpu_w24sx_layouts.py, set for reductions up to 4608 = 9 x 512);
  * ``w24sx``: the two gates of ``test_gpu_w24sx.gates`` -- e_new <= 3 e_w24 + 1e-7 and |y_new - y_exact| <= 2e-5 scale against
    ``seam_conv2d_f32`` with the same pack form and epilogue;
  * every case with K >= 256 whose index is a multiple of 5 runs again under forced n-tile splits 2, 4 and 8 (the split that runs
    is read back from the query; the forced value is restored in a ``finally``): the bytes of the rule's launch.
One block of refusals per family.  The child stops launching at the first exception (a HIP error is a RuntimeError of torch); a
non-zero return code or a touched guard is a FAIL and the child goes on."""
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

import w24_layout_cases as T
import w24sx_stress_cases as SC
from stress_kit import Buf, P, fail, fails, refused, say, st, twice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_AROUND = 1 << 16            # bytes of NaN before and directly behind every input tensor (a multiple of 16: 16-byte loads)
PAD_FILL = 3.0e4                # the channels of x beyond Cin
TOL_W24 = 3e-5                  # tests/test_gpu_w24sx_layouts.py
FORCED = (2, 4, 8)
_M64 = (1 << 64) - 1
_GOLD = 0x9E3779B97F4A7C15


# ------------------------------------------------------------------------------------------------ synth.normal in torch integers
def _i64(v):
    v &= _M64
    return v - (1 << 64) if v >> 63 else v


def _shr(z, s):
    """logical right shift of the 64 bits of an int64 tensor"""
    return (z >> s) & ((1 << (64 - s)) - 1)


def _mix64(z):
    z = z ^ _shr(z, 30)
    z = z * _i64(0xBF58476D1CE4E5B9)
    z = z ^ _shr(z, 27)
    z = z * _i64(0x94D049BB133111EB)
    return z ^ _shr(z, 31)


def _mix64_int(z):
    z &= _M64
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & _M64
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & _M64
    return z ^ (z >> 31)


def normal(stream, shape, device):
    """``synth.normal(stream, shape)`` (Irwin-Hall(12) - 6 over splitmix64 streams) as an fp32 tensor on ``device``, bit for bit"""
    n = math.prod(shape)
    out = torch.empty(n, dtype=torch.float32, device=device)
    step = 1 << 22
    for s in range(0, n, step):
        e = min(n, s + step)
        idx1 = (torch.arange(s, e, dtype=torch.int64, device=device) + 1) * _i64(_GOLD)
        acc = torch.zeros(e - s, dtype=torch.int64, device=device)
        for j in range(12):
            sj = (stream ^ (0x5851F42D4C957F2D * (j + 1) & _M64)) & _M64
            base = _mix64_int(sj * _GOLD + 0x632BE59BD9B4E019)
            acc += _shr(_mix64(idx1 ^ _i64(base)), 40)
        out[s:e] = (acc.double() / 16777216.0 - 6.0).float()
    return out.view(shape)


def between_nans(t):
    """a contiguous copy of fp32 ``t`` with NAN_AROUND bytes of NaN before its first and directly behind its last element"""
    pad, n = NAN_AROUND // 4, t.numel()
    raw = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float32, device=t.device)
    raw[pad:pad + n].copy_(t.reshape(-1))
    return raw[pad:pad + n].view(t.shape)


# ------------------------------------------------------------------------------------------------ the reference and the checks
def reference64(x, w, pad, mode=0, scale=None, shift=None, res=None, relu=0):
    """The float64 3x3 / stride-1 convolution of NHWC ``x`` [N, H, W, Cstore] as nine shifted matmuls, and the epilogue in float64.
    mode 0: ``w`` is OIHW [K, Cin, 3, 3]; mode 2: ``w`` is [Cin, K, 3, 3] and the result is the transposed convolution
    (F.conv_transpose2d with padding 2 - pad): taps rotated by 180 degrees, channels swapped.  Only the first Cin channels of x count.
    relu 0 | 1, or 2: ``res`` is not added, the result is zero where res <= 0.  -> [N, Ho, Wo, K] float64"""
    n, h, wd, _ = x.shape
    cin, k = (w.shape[1], w.shape[0]) if mode == 0 else (w.shape[0], w.shape[1])
    ho, wo = h + 2 * pad - 2, wd + 2 * pad - 2
    xp = F.pad(x[..., :cin].double(), (0, 0, pad, pad, pad, pad))
    w64 = w.double()
    acc = torch.zeros((n * ho * wo, k), dtype=torch.float64, device=x.device)
    for r in range(3):
        for s in range(3):
            tap = w64[:, :, r, s].t() if mode == 0 else w64[:, :, 2 - r, 2 - s]         # [Cin, K]
            acc += xp[:, r:r + ho, s:s + wo, :].reshape(-1, cin) @ tap
    y = acc.view(n, ho, wo, k)
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if relu == 2:
        return torch.where(res > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu == 1 else y


def figures(y, y64, y24, yex):
    """-> dict e_new, e_w24 (max error over max|y64|), d_ex = max|y - y_exact| over the same scale"""
    scale = max(float(y64.abs().max()), 1e-30)
    return {"e_new": float((y.double() - y64).abs().max()) / scale, "e_w24": float((y24.double() - y64).abs().max()) / scale,
            "d_ex": float((y - yex).abs().max()) / scale}


def check(desc, y, y64, y24, yex):
    """The gates of family ``w24sx`` on a result ``y`` -> (list of reasons it fails, empty where it passes; its figures)"""
    import test_gpu_w24sx as W
    why = []
    if not bool(torch.isfinite(y).all()):
        why.append("poison or non-finite values left in the output")
    try:
        W.gates(desc, y, y64, y24, yex)
    except AssertionError as e:
        why.append(str(e))
    return why, figures(y, y64, y24, yex)


def check_f32(y24, y64):
    """The gate of family ``w24f32``"""
    why = []
    if not bool(torch.isfinite(y24).all()):
        why.append("poison or non-finite values left in the output")
    e = float((y24.double() - y64).abs().max()) / max(float(y64.abs().max()), 1e-30)
    if not e <= TOL_W24:
        why.append(f"e_w24 {e:.3e} > {TOL_W24:.0e}")
    return why


# ------------------------------------------------------------------------------------------------ one case
def operands(c, device):
    """the tensors of case ``c`` on ``device`` -> dict x, w, scale, shift, res (None where the epilogue has none), relu"""
    import seam_match_rcnn_amd.synth as synth
    seed = c["data_seed"]
    n, h, w, cc, k, pad, cin = (c[key] for key in ("n", "h", "w", "c", "k", "pad", "cin"))
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    x = normal(synth.stream_id(seed, "x"), (n, h, w, cc), device)
    if cin < cc:
        x[..., cin:] = PAD_FILL
    wshape = (k, cin, 3, 3) if c["mode"] == 0 else (cin, k, 3, 3)
    wt = normal(synth.stream_id(seed, "w"), wshape, device) * (1.0 / math.sqrt(9 * cc))
    has_scale, has_shift, has_res, relu = SC.EPI_FLAGS[c["epilogue"]]
    o = {"x": between_nans(x), "w": wt, "scale": None, "shift": None, "res": None, "relu": relu}
    if has_scale:
        o["scale"] = between_nans(torch.from_numpy(synth.uniform(synth.stream_id(seed, "sc"), (k,), 0.5, 1.5)).to(device))
    if has_shift:
        o["shift"] = between_nans(normal(synth.stream_id(seed, "sh"), (k,), device) * 0.1)
    if has_res:
        res = normal(synth.stream_id(seed, "res"), (n, ho, wo, k), device)
        if relu == 2:                       # the mask: mixed signs and exact zeros (a fifth of it)
            res = torch.where(res.abs() < 0.25, torch.zeros_like(res), res)
        o["res"] = between_nans(res)
    return o


def packs(o, c):
    k, cc, cin, mode = c["k"], c["c"], c["cin"], c["mode"]
    u = torch.empty((int(lib.seam_wino24sx_weight_bytes(k, cc)),), dtype=torch.uint8, device=dev)
    assert lib.seam_pack_conv_weight_wino24_sx(P(o["w"]), P(u), k, cin, cc, mode, st()) == 0
    u24 = torch.empty((int(lib.seam_wino24_weight_floats(k, cc)),), dtype=torch.float32, device=dev)
    assert lib.seam_pack_conv_weight_wino24_f32(P(o["w"]), P(u24), k, cin, cc, mode, st()) == 0
    wp = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred(cc, 3, 3)), dtype=torch.float32, device=dev)
    assert lib.seam_pack_conv_weight_f32(P(o["w"]), P(wp), k, cin, 3, 3, cc, mode, st()) == 0
    return u, u24, wp


def launch_sx(o, u, c, y, x=None, res=None, n=None):
    x, res = o["x"] if x is None else x, o["res"] if res is None else res
    return lib.seam_conv3x3_wino24sx_f32(P(x), P(u), P(o["scale"]), P(o["shift"]), P(res), P(y), n or c["n"], c["h"], c["w"], c["c"], c["k"],
                                         c["pad"], 1, o["relu"], st())


def launch_f32(o, u24, c, y, x=None, res=None, n=None):
    x, res = o["x"] if x is None else x, o["res"] if res is None else res
    return lib.seam_conv3x3_wino24_f32(P(x), P(u24), P(o["scale"]), P(o["shift"]), P(res), P(y), n or c["n"], c["h"], c["w"], c["c"], c["k"],
                                       c["pad"], o["relu"], st())


def run_family(family, desc, c, o, launch, shape):
    """twice + the image check -> (y or None, bit-identical)"""
    say("START", family, desc)
    out = twice(family, desc, [shape], lambda bufs: launch(bufs[0].t))
    if out is None:
        return None, False
    y = out[0]
    j = c["data_seed"] % c["n"]
    xj = between_nans(o["x"][j:j + 1])
    rj = None if o["res"] is None else between_nans(o["res"][j:j + 1])
    alone = Buf((1,) + tuple(shape[1:]), torch.float32, 0, dev)
    rc = launch(alone.t, x=xj, res=rj, n=1)
    torch.cuda.synchronize()
    if rc != 0 or not alone.guard_ok():
        fail(family, desc, f"image {j} alone: rc {rc}, guards intact {alone.guard_ok()}")
        return y, False
    same = torch.equal(alone.bits()[0], y[j].view(torch.int32))
    if not same:
        fail(family, desc, f"image {j} alone differs from image {j} in the batch")
    return y, same


def run_case(c, stats, wanted):
    n, h, w, cc, k, pad = (c[key] for key in ("n", "h", "w", "c", "k", "pad"))
    desc = SC.describe(c)
    shape = (n, h + 2 * pad - 2, w + 2 * pad - 2, k)
    t0 = time.time()
    lay = T.query(lib, n, h, w, cc, k, pad)
    if lay is None or SC.layout_pair(lay, n, h, w, pad) != c["pair"]:
        return fail("w24sx", desc, f"the library lays this case out as {lay}, not as {c['pair']}")
    if lay["stack"]:
        alone = T.query(lib, 1, h, w, cc, k, pad)
        if (alone["stack"], alone["TX"], alone["TY"]) == (lay["stack"], lay["TX"], lay["TY"]):
            fail("w24sx", desc, "one image alone has the layout of the batch: the image check proves nothing")
    for fam in wanted:
        stats[fam]["tags"].append(SC.classify(c, lay, cus))
    o = operands(c, dev)
    u, u24, wp = packs(o, c)
    y64 = reference64(o["x"], o["w"], pad, c["mode"], o["scale"], o["shift"], o["res"], o["relu"])
    if not bool(torch.isfinite(y64).all()):
        return fail("w24sx", desc, "the float64 reference is not finite: the test's own operands are wrong")
    # ---- w24f32 (and what both families need: the operands, the reference, the exact kernel)
    y24, same = run_family("w24f32", desc, c, o, lambda y, **kw: launch_f32(o, u24, c, y, **kw), shape)
    yex = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
    rc = lib.seam_conv2d_f32(P(o["x"]), P(wp), P(o["scale"]), P(o["shift"]), P(o["res"]), P(yex), n, h, w, cc, k, 3, 3, 1, pad, o["relu"], st())
    torch.cuda.synchronize()
    if rc != 0:
        fail("w24f32", desc, f"seam_conv2d_f32 returned {rc}")
    if y24 is not None:
        why = check_f32(y24, y64)
        for reason in why:
            fail("w24f32", desc, reason)
        stats["w24f32"]["identical"] += int(same)
    elif "w24sx" in wanted:          # the fp32 launch failed its own checks: the split kernel is still gated, against one more of it
        y24 = torch.full(shape, float("nan"), dtype=torch.float32, device=dev)
        if launch_f32(o, u24, c, y24) != 0:
            y24 = yex               # (refused: the exact kernel stands in, e_w24 is then e_exact)
        torch.cuda.synchronize()
    stats["w24f32"]["seconds"] += time.time() - t0
    if "w24sx" not in wanted or rc != 0:
        return
    # ---- w24sx
    t0 = time.time()
    y, same = run_family("w24sx", desc, c, o, lambda y, **kw: launch_sx(o, u, c, y, **kw), shape)
    if y is not None:
        why, f = check(desc, y, y64, y24, yex)
        for reason in why:
            fail("w24sx", desc, reason)
        ratio = f["e_new"] / max(f["e_w24"], 1e-30)
        say(f"CASE {desc} e_new {f['e_new']:.3e} e_w24 {f['e_w24']:.3e} ratio {ratio:.2f} |new-exact|/scale {f['d_ex']:.3e}")
        stats["w24sx"]["identical"] += int(same)
        stats["figures"].append((cc, f["e_new"], f["e_w24"], ratio))
        if k >= 256 and c["index"] % 5 == 0:
            forced_splits(c, desc, lay, o, u, y, shape, stats)
    stats["w24sx"]["seconds"] += time.time() - t0


def forced_splits(c, desc, lay, o, u, y, shape, stats):
    """the n-tile split over XCD groups only renumbers the blocks: the bytes of the rule's launch, padding blocks or not"""
    before = lib.seam_conv3x3_wino24sx_get_nsplit()
    try:
        for ns in FORCED:
            if lib.seam_conv3x3_wino24sx_set_nsplit(ns) != 0:
                fail("w24sx", desc, f"set_nsplit({ns}) refused")
                continue
            got = T.query(lib, c["n"], c["h"], c["w"], c["c"], c["k"], c["pad"])
            stats["forced"] += 1
            stats["ragged-partitions"] += int(lay["patch_blocks"] % (8 // got["nsplit"]) != 0)
            say("START w24sx", desc, f"forced nsplit {ns} runs as {got['nsplit']}, grid {got['grid_blocks']}")
            b = Buf(shape, torch.float32, 0, dev)
            rc = launch_sx(o, u, c, b.t)
            torch.cuda.synchronize()
            if rc != 0 or not b.guard_ok():
                fail("w24sx", desc, f"forced split {ns}: rc {rc}, guards intact {b.guard_ok()}")
            elif not torch.equal(b.bits(), y.view(torch.int32)):
                fail("w24sx", desc, f"forced split {ns} (runs as {got['nsplit']}) differs from the rule's launch")
    finally:
        lib.seam_conv3x3_wino24sx_set_nsplit(before)


# ------------------------------------------------------------------------------------------------ refusals
REFUSED_LAUNCHES = [("C=96", dict(c=96)), ("K=32", dict(k=32)), ("stride=2", dict(stride=2)), ("pad=2", dict(pad=2)), ("Ho<=0", dict(h=1, pad=0))]
# predicates only (nothing that large is allocated): one image of >= 2^31 bytes of input; >= 2^24 blocks
REFUSED_PREDICATES = [("image>=2^31-bytes", (1, 210, 210, 12224, 64, 1)), ("blocks>=2^24", (4000, 210, 210, 64, 2048, 1))]
# the fp32 entry's own contract (include/seam_hip.h): C a multiple of 8, K of 32, an output of at least one pixel, N >= 1
REFUSED_LAUNCHES_F32 = [("C=60", dict(c=60)), ("K=48", dict(k=48)), ("Ho<=0", dict(h=1, pad=0)), ("N=0", dict(n=0))]


def refusals(family):
    d = torch.zeros(1 << 20, device=dev)        # stands for every operand
    for name, change in REFUSED_LAUNCHES if family == "w24sx" else REFUSED_LAUNCHES_F32:
        a = dict(n=1, h=8, w=8, c=64, k=64, pad=1, stride=1)
        a.update(change)
        if family == "w24sx":
            fn = lambda b, a=a: lib.seam_conv3x3_wino24sx_f32(P(d), P(d), None, None, None, P(b[0].t), a["n"], a["h"], a["w"], a["c"], a["k"],
                                                              a["pad"], a["stride"], 0, st())
        else:
            fn = lambda b, a=a: lib.seam_conv3x3_wino24_f32(P(d), P(d), None, None, None, P(b[0].t), a["n"], a["h"], a["w"], a["c"], a["k"], a["pad"],
                                                            0, st())
        refused(family, name, [(1, 8, 8, 64)], fn)
    if family == "w24sx":
        for name, args in REFUSED_PREDICATES:
            say("START", family, "refuse", name)
            if lib.seam_conv3x3_wino24sx_supported(*args, 1) != 0 or T.query(lib, *args) is not None:
                fail(family, name, "not refused")


# ------------------------------------------------------------------------------------------------ the sweep
def summary(family, stats, ncases):
    s = stats[family]
    counts = SC.count_tags(s["tags"])
    classes = " ".join(f"{t} {counts[t]}" for t in sorted(counts))
    figs = stats["figures"]
    e_new, e_w24, ratio = (max([f[i] for f in figs], default=0.0) for i in (1, 2, 3))
    per_c = " ".join(f"worst-ratio-C{cc} {max(f[3] for f in figs if f[0] == cc):.2f}" for cc in sorted({f[0] for f in figs}))
    say(f"SUMMARY {family} cases {ncases} bit-identical {s['identical']} {classes} cus {cus} max_e_new {e_new:.3e} max_e_w24 {e_w24:.3e} "
        f"max_ratio {ratio:.2f} {per_c} forced-splits {stats['forced']} ragged-partitions {stats['ragged-partitions']} seconds {s['seconds']:.1f}")
    if family == "w24sx":
        for cc in sorted({f[0] for f in figs}):
            mine = [f for f in figs if f[0] == cc]
            lo, hi = (lambda i: min(f[i] for f in mine)), (lambda i: max(f[i] for f in mine))
            say(f"RANGE C {cc} cases {len(mine)} e_new {lo(1):.3e} {hi(1):.3e} e_w24 {lo(2):.3e} {hi(2):.3e} ratio {lo(3):.2f} {hi(3):.2f}")


def sweep(wanted):
    stats = {f: {"tags": [], "identical": 0, "seconds": 0.0} for f in FAMILY_NAMES}
    stats.update({"figures": [], "forced": 0, "ragged-partitions": 0})
    cs = SC.cases(NCASE, SEED, lambda *a: T.query(lib, *a))
    done = 0
    try:
        for c in cs:
            run_case(c, stats, wanted)
            done += 1
        for family in wanted:
            t0 = time.time()
            refusals(family)
            stats[family]["seconds"] += time.time() - t0
        torch.cuda.synchronize()
    except Exception as e:          # a HIP error surfaces as a RuntimeError of torch: nothing more is launched
        text = str(e).splitlines()[0] if str(e) else ""
        say("STOP", type(e).__name__, text)
        for family in wanted:
            fail(family, "-", f"stopped after {done} cases: {type(e).__name__} {text}".replace("\n", " "))
        return
    if "w24sx" in wanted and NCASE >= 100 and not stats["ragged-partitions"]:
        fail("w24sx", "-", "no forced split whose partition count does not divide the patch blocks")
    for family in wanted:
        if stats[family]["identical"] != len(cs):
            fail(family, "-", f"only {stats[family]['identical']} of {len(cs)} cases bit-identical (twice, and one image alone)")
        summary(family, stats, done)


FAMILY_NAMES = ("w24f32", "w24sx")
# both families run in one pass over the case list (they share operands, reference and exact kernel); asked for alone, ``w24sx``
# still needs the fp32 results its gate is relative to
FAMILIES = [(name, (lambda f: lambda: sweep(("w24f32", "w24sx") if f == "w24sx" else (f,)))(name)) for name in FAMILY_NAMES]


def main(argv):
    global NCASE, SEED, cus, dev, lib
    sys.path.insert(0, ROOT)
    from seam_match_rcnn_amd import _native
    NCASE, SEED = int(argv[0]), int(argv[1])
    dev = torch.device("cuda:0")
    lib = _native.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    asked = [name for name in FAMILY_NAMES if len(argv) <= 2 or name in argv[2:]]
    sweep(tuple(FAMILY_NAMES) if "w24sx" in asked else tuple(asked))
    for name in asked:
        say("KERNEL", name, "failures", sum(1 for f in fails if f[0] == name))
    say("DONE failures", len(fails))
    for f in fails[:40]:
        say("FAILED", *f)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
