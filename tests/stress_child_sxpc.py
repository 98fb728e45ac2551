"""The child of ``test_gpu_stress_sxpc.py``: ``python stress_child_sxpc.py NCASE SEED [family ...]`` runs the seeded cases of
``sxpc_stress_cases.py`` through the seven launch entries of ``sxpc_body`` (csrc/seam_pwsx.hip) and prints the lines
``stress_kit.family_ok`` reads.  Importing it launches nothing.

Per case:
  * inputs N(0, 1), weights N(0, 1) / sqrt(C).  Every input tensor lies between two runs of NAN_AROUND bytes of NaN, the second
    directly behind its last element; x2 is NaN wherever the stride does not sample it, ``top`` wherever ATen's nearest rule does
    not reach (the stem's frame keeps its zero cells: the window needs them).  A load one row past M, past a sampled pixel or
    from a wrong image shows as a non-finite output;
  * the launch goes through ``stress_kit.twice``: two launches onto differently poisoned, guarded outputs, bit-identical;
  * (a) a float64 reference in plain torch on the device, from the entry's own inputs and the unpacked fp32 weight -- no project
    kernel in it -- under the project's gate e <= 2 e_exact + 1e-7, e = max|y - y64| / max|y64|, e_exact the same measure of the
    exact fp32 kernel on the same operands (``seam_conv2d_f32`` on the materialised rows; the stem: the exact stem launch);
  * (b) the bits of ``seam_conv2d_sx(terms=6)`` on the materialised rows (the kernel header's claim).
Per family (c) the nearest unserved neighbours of served shapes are refused on the host and write nothing, and (d) the SUMMARY line
repeats the class counts of the generator, recounted with the device's CU count."""
import math
import os
import sys
import time

import torch
import torch.nn.functional as F

import sxpc_stress_cases as SC
from stress_kit import P, fail, fails, refused, say, st, twice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN_AROUND = 1 << 16            # bytes of NaN before and directly behind every input tensor (a multiple of 16: the kernels load 16-byte vectors)


def between_nans(t):
    """a contiguous copy of fp32 ``t`` with NAN_AROUND bytes of NaN before its first and directly behind its last element"""
    pad, n = NAN_AROUND // 4, t.numel()
    raw = torch.full((n + 2 * pad,), float("nan"), dtype=torch.float32, device=t.device)
    raw[pad:pad + n].copy_(t.reshape(-1))
    return raw[pad:pad + n].view(t.shape)


def randn(g, *shape):
    return torch.randn(shape, device=dev, generator=g)


def epilogue64(acc, scale, shift, res, relu):
    y = acc
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if relu else y


def nearest_index(ho, wo, rh, rw):
    """[Ho Wo] long: the coarse pixel rW hs + ws of every output pixel, by ATen's own nearest rule (an index map through
    ``F.interpolate``; the indices are exact in fp32)"""
    idx = torch.arange(rh * rw, dtype=torch.float32, device=dev).view(1, 1, rh, rw)
    return F.interpolate(idx, size=(ho, wo), mode="nearest").view(ho * wo).long()


def stem_rows(xp):
    """[N, Hs + 3, Ws + 3, 12] -> [N Hs Ws, 192]: per output pixel its 4 x 4 cells in (r, s, c) order"""
    n, hp, wp, _ = xp.shape
    win = xp.unfold(1, 4, 1).unfold(2, 4, 1)                 # [N, Hs, Ws, 12, r, s]
    return win.permute(0, 1, 2, 4, 5, 3).reshape(n * (hp - 3) * (wp - 3), 192).contiguous()


# ------------------------------------------------------------------------------------------------ the packs (through the C ABI)
def pack_sx(wt):
    """the pack of ``seam_conv2d_sx`` for the 1x1 layer wt [K, C]"""
    k, c = wt.shape
    rows, kred = lib.seam_conv_rows_padded(k), lib.seam_conv_kred(c, 1, 1)
    wp = torch.empty((rows, kred * 3), dtype=torch.bfloat16, device=dev)
    tmp = torch.empty((rows, kred), dtype=torch.float32, device=dev)
    assert lib.seam_pack_conv_weight_sx(P(wt), P(wp), P(tmp), k, c, 1, 1, c, 0, st()) == 0
    return wp


def pack_f32(w4, cs):
    """the exact implicit GEMM's pack of the OIHW weight w4"""
    k, c, r, s = w4.shape
    wp = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred(cs, r, s)), dtype=torch.float32, device=dev)
    assert lib.seam_pack_conv_weight_f32(P(w4), P(wp), k, c, r, s, cs, 0, st()) == 0
    return wp


def pack_sxpc(wt, entry):
    k, c = wt.shape
    wq = torch.empty((int(lib.seam_conv1x1_sxpc_weight_bytes(k, c)),), dtype=torch.uint8, device=dev)
    assert getattr(lib, entry)(P(wt), P(wq), k, c, st()) == 0, entry
    return wq


PACK_ENTRY = {"sxpc": "seam_pack_conv1x1_weight_sxpc", "sxpc_dual": "seam_pack_conv1x1_weight_sxpc", "sxpc_up": "seam_pack_conv1x1_weight_sxpc",
              "sxpc_short": "seam_pack_conv1x1_weight_sxpc_short", "sxpc_dual_short": "seam_pack_conv1x1_weight_sxpc_short",
              "sxpc64": "seam_pack_conv1x1_weight_sxpc64", "stem_sxpc": "seam_pack_conv1x1_weight_sxpc64"}


# ------------------------------------------------------------------------------------------------ one case
def build(family, c, g):
    """the operands of case ``c`` -> dict: ``launch(y)`` -> rc, ``rows`` [M, C] (the materialised reduction rows, exact copies of the
    inputs), ``wt`` [K, C], ``add`` [M, K] or None (the residual / the gathered coarse pixels), ``y64`` before the epilogue, and for
    the stem ``exact(y)``"""
    m, cc, k, relu = c["M"], c["C"], c["K"], c["relu"]
    o = {}
    if family == "stem_sxpc":
        n, hs, ws = c["N"], c["Ho"], c["Wo"]
        xu = randn(g, n, hs, ws, 12)
        w4 = randn(g, 64, 12, 4, 4) / math.sqrt(cc)             # OIHW of the 4x4 / stride-1 form; the pack takes its (r, s, c) rows
        wt = w4.permute(0, 2, 3, 1).reshape(64, 192).contiguous()
    else:
        wt = randn(g, k, cc) / math.sqrt(cc)
    scale = (torch.rand(k, device=dev, generator=g) + 0.5) if c["scale"] else None
    shift = randn(g, k) if c["shift"] else None
    res = between_nans(randn(g, m, k)) if c["res"] else None
    wq = pack_sxpc(wt, PACK_ENTRY[family])
    add = res
    if family in ("sxpc", "sxpc_short", "sxpc64"):
        x = between_nans(randn(g, m, cc))
        entry = {"sxpc": lib.seam_conv1x1_sxpc, "sxpc_short": lib.seam_conv1x1_sxpc_short, "sxpc64": lib.seam_conv1x1_sxpc64}[family]
        o["launch"] = lambda y: entry(P(x), P(wq), P(scale), P(shift), P(res), P(y), m, cc, k, relu, st())
        rows = x
    elif family in ("sxpc_dual", "sxpc_dual_short"):
        n, ho, wo, c1, c2, h2, w2, s = c["N"], c["Ho"], c["Wo"], c["C1"], c["C2"], c["H2"], c["W2"], c["stride2"]
        x1 = between_nans(randn(g, n, ho, wo, c1))
        full = torch.full((n, h2, w2, c2), float("nan"), dtype=torch.float32, device=dev)
        hi, wi = torch.arange(ho, device=dev) * s, torch.arange(wo, device=dev) * s
        full[:, hi[:, None], wi[None, :]] = randn(g, n, ho, wo, c2)
        x2 = between_nans(full)
        del full
        if family == "sxpc_dual":
            o["launch"] = lambda y: lib.seam_conv1x1_sxpc_dual(P(x1), P(x2), P(wq), P(scale), P(shift), P(y), n, ho, wo, c1, h2, w2, c2, s, k, relu, st())
        else:
            o["launch"] = lambda y: lib.seam_conv1x1_sxpc_dual_short(P(x1), P(x2), P(wq), P(scale), P(shift), P(y), n, ho, wo, c1, h2, w2, c2, k, relu, st())
        rows = torch.cat([x1, x2[:, ::s, ::s][:, :ho, :wo]], -1).reshape(m, cc).contiguous()
    elif family == "sxpc_up":
        n, ho, wo, rh, rw = c["N"], c["Ho"], c["Wo"], c["rH"], c["rW"]
        x = between_nans(randn(g, n, ho, wo, cc))
        idx = nearest_index(ho, wo, rh, rw)
        full = torch.full((n, rh * rw, k), float("nan"), dtype=torch.float32, device=dev)
        reached = torch.unique(idx)
        full[:, reached] = randn(g, n, reached.numel(), k)
        top = between_nans(full.view(n, rh, rw, k))
        del full
        o["launch"] = lambda y: lib.seam_conv1x1_sxpc_up(P(x), P(wq), P(scale), P(shift), P(top), P(y), n, ho, wo, cc, k, rh, rw, relu, st())
        rows = x.view(m, cc)
        add = top.view(n, rh * rw, k)[:, idx].reshape(m, k).contiguous()
    else:
        xp = between_nans(F.pad(xu, (0, 0, 2, 1, 2, 1)))
        o["launch"] = lambda y: lib.seam_stem_sxpc(P(xp), P(wq), P(scale), P(shift), P(y), n, hs, ws, relu, st())
        rows = stem_rows(xp)
        o["acc64"] = F.conv2d(xp.permute(0, 3, 1, 2).double(), w4.double()).permute(0, 2, 3, 1).reshape(m, 64)
        we = pack_f32(w4, 12)
        # the exact stem launch of tests/test_gpu_stem_sxpc.py: the implicit GEMM over the unpadded frame, pad 2, cropped to its grid
        o["exact"] = lambda y: lib.seam_conv2d_crop_f32(P(xu), P(we), P(scale), P(shift), P(y), n, hs, ws, 12, 64, 4, 4, 1, 2, hs, ws, relu, st())
    if "acc64" not in o:
        o["acc64"] = rows.double() @ wt.double().t()
    o.update(rows=rows, wt=wt, scale=scale, shift=shift, add=add, up=family == "sxpc_up")
    return o


def run_case(family, c, stats):
    m, cc, k, relu = c["M"], c["C"], c["K"], c["relu"]
    desc = SC.describe(c)
    say("START", family, desc)
    g = torch.Generator(device=dev)
    g.manual_seed(c["data_seed"])
    o = build(family, c, g)
    rows, scale, shift, add = o["rows"], o["scale"], o["shift"], o["add"]
    shape = (m, k)
    out = twice(family, desc, [shape], lambda bufs: o["launch"](bufs[0].t))
    if out is None:
        return
    y = out[0]
    if not bool(torch.isfinite(y).all()):
        bad = torch.nonzero(~torch.isfinite(y).all(1)).flatten()
        return fail(family, desc, f"non-finite output in {bad.numel()} rows, first {int(bad[0])}: a load outside the sampled input")
    # (a) float64, no project kernel
    y64 = epilogue64(o["acc64"], scale, shift, add, relu)
    if not bool(torch.isfinite(y64).all()):
        return fail(family, desc, "the float64 reference is not finite: the test's own operands are wrong")
    ye = torch.empty(shape, dtype=torch.float32, device=dev)
    if "exact" in o:
        rc = o["exact"](ye)
    else:
        we = pack_f32(o["wt"].view(k, cc, 1, 1), cc)
        rc = lib.seam_conv2d_f32(P(rows), P(we), P(scale), P(shift), P(add), P(ye), 1, 1, m, cc, k, 1, 1, 1, 0, relu, st())
    if rc != 0:
        return fail(family, desc, f"the exact kernel returned {rc}")
    top = max(float(y64.abs().max()), 1e-30)
    e = float((y.double() - y64).abs().max()) / top
    e_exact = float((ye.double() - y64).abs().max()) / top
    ratio = e / (2 * e_exact + 1e-7)
    stats["worst"] = max(stats["worst"], ratio)
    if not e <= 2 * e_exact + 1e-7:
        fail(family, desc, f"gate: e {e:.3e} > 2 * e_exact {e_exact:.3e} + 1e-7")
    # (b) the bits of seam_conv2d_sx(terms = 6) on the materialised rows
    ws = pack_sx(o["wt"])
    yb = torch.empty(shape, dtype=torch.float32, device=dev)
    if o["up"]:        # (scale, shift), then ONE fp32 add of the gathered coarse pixel, then ReLU -- in torch
        rc = lib.seam_conv2d_sx(P(rows), P(ws), P(scale), P(shift), None, P(yb), 1, m, 1, cc, k, 1, 1, 1, 0, 0, 6, st())
        yb = yb + add
        yb = torch.relu(yb) if relu else yb
    else:
        rc = lib.seam_conv2d_sx(P(rows), P(ws), P(scale), P(shift), P(add), P(yb), 1, m, 1, cc, k, 1, 1, 1, 0, relu, 6, st())
    if rc != 0:
        return fail(family, desc, f"seam_conv2d_sx returned {rc}")
    if torch.equal(y.view(torch.int32), yb.view(torch.int32)):
        stats["identical"] += 1
    else:
        diff = y.view(torch.int32) != yb.view(torch.int32)
        fail(family, desc, f"bits differ from seam_conv2d_sx(terms=6) in {int(diff.sum())} elements, first row {int(torch.nonzero(diff.any(1))[0])}")


# ------------------------------------------------------------------------------------------------ (c) refusals: host side only
def refusals(family):
    d = torch.zeros(1 << 20, device=dev)   # stands for every operand: larger than any of them at these shapes
    n, ho, wo = 2, 4, 8                    # M = 64

    def plain(entry):
        return lambda c, k, relu: (lambda b: entry(P(d), P(d), None, None, None, P(b[0].t), 64, c, k, relu, st()))
    if family in ("sxpc", "sxpc_short", "sxpc64"):
        entry = plain({"sxpc": lib.seam_conv1x1_sxpc, "sxpc_short": lib.seam_conv1x1_sxpc_short, "sxpc64": lib.seam_conv1x1_sxpc64}[family])
        ok = {"sxpc": (256, 128), "sxpc_short": (128, 128), "sxpc64": (128, 64)}[family]
        near = {"sxpc": [("C=288", 288, 128, 0), ("C=192", 192, 128, 0), ("K=192", 256, 192, 0), ("K=64", 256, 64, 0)],
                "sxpc_short": [("C=160", 160, 128, 0), ("C=64", 64, 128, 0), ("C=192", 192, 128, 0), ("K=192", 128, 192, 0), ("K=64", 128, 64, 0)],
                "sxpc64": [("C=160", 160, 64, 0), ("C=64", 64, 64, 0), ("K=128", 128, 128, 0), ("K=32", 128, 32, 0)]}[family]
        for name, c, k, relu in near + [("relu=2", ok[0], ok[1], 2)]:
            refused(family, name, [(64, max(k, 64))], entry(c, k, relu))
    elif family in ("sxpc_dual", "sxpc_dual_short"):
        def entry(c1, c2, k, relu, h2=ho, w2=wo, s=1):
            if family == "sxpc_dual":
                return lambda b: lib.seam_conv1x1_sxpc_dual(P(d), P(d), P(d), None, None, P(b[0].t), n, ho, wo, c1, h2, w2, c2, s, k, relu, st())
            return lambda b: lib.seam_conv1x1_sxpc_dual_short(P(d), P(d), P(d), None, None, P(b[0].t), n, ho, wo, c1, h2, w2, c2, k, relu, st())
        a, b_ = (64, 192) if family == "sxpc_dual" else (64, 64)
        near = [("C1=96", entry(96, 160, 128, 0)), ("C2=32", entry(a, 32, 128, 0)), ("K=192", entry(a, b_, 192, 0)), ("relu=2", entry(a, b_, 128, 2))]
        if family == "sxpc_dual":
            near += [("C1+C2=192", entry(64, 128, 128, 0)), ("(Ho-1)*s==H2", entry(a, b_, 128, 0, h2=(ho - 1) * 2, w2=2 * wo, s=2)),
                     ("(Wo-1)*s==W2", entry(a, b_, 128, 0, h2=2 * ho, w2=(wo - 1) * 2, s=2))]
        else:
            near += [("C2=128", entry(64, 128, 128, 0)), ("C1=128", entry(128, 64, 128, 0)), ("(Ho-1)*s==H2", entry(a, b_, 128, 0, h2=ho - 1))]
        for name, fn in near:
            refused(family, name, [(64, 192)], fn)
    elif family == "sxpc_up":
        def entry(c, k, rh, rw, relu):
            return lambda b: lib.seam_conv1x1_sxpc_up(P(d), P(d), None, None, P(d), P(b[0].t), n, ho, wo, c, k, rh, rw, relu, st())
        for name, fn in [("C=288", entry(288, 128, 2, 4, 0)), ("C=192", entry(192, 128, 2, 4, 0)), ("K=192", entry(256, 192, 2, 4, 0)),
                         ("relu=2", entry(256, 128, 2, 4, 2)), ("rH=0", entry(256, 128, 0, 4, 0)), ("rW=0", entry(256, 128, 2, 0, 0))]:
            refused(family, name, [(64, 192)], fn)
    else:                                   # the stem has no channel arguments: its geometry and the ReLU flag
        def entry(n_, hs, ws, relu):
            return lambda b: lib.seam_stem_sxpc(P(d), P(d), None, None, P(b[0].t), n_, hs, ws, relu, st())
        for name, fn in [("relu=2", entry(n, ho, wo, 2)), ("N=0", entry(0, ho, wo, 0)), ("Hs=0", entry(n, 0, wo, 0)), ("Ws=0", entry(n, ho, 0, 0))]:
            refused(family, name, [(64, 64)], fn)


def stress(family):
    t0 = time.time()
    stats = {"identical": 0, "worst": 0.0}
    cs = SC.cases(family, NCASE, SEED)
    for c in cs:
        run_case(family, c, stats)
    refusals(family)
    counts = SC.count_tags(SC.classify(family, c, cus) for c in cs)
    classes = " ".join(f"{t} {counts[t]}" for t in sorted(counts))
    say(f"SUMMARY {family} cases {len(cs)} bit-identical {stats['identical']} {classes} cus {cus} worst-gate-ratio {stats['worst']:.4f} "
        f"seconds {time.time() - t0:.1f}")
    if stats["identical"] != len(cs):
        fail(family, "-", f"only {stats['identical']} of {len(cs)} results bit-identical to seam_conv2d_sx(terms=6)")


FAMILIES = [(name, (lambda f: lambda: stress(f))(name)) for name in SC.FAMILIES]


def main(argv):
    global NCASE, SEED, cus, dev, lib
    sys.path.insert(0, ROOT)
    from seam_match_rcnn_amd import _native
    NCASE, SEED = int(argv[0]), int(argv[1])
    dev = torch.device("cuda:0")
    lib = _native.lib()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    for name, fn in FAMILIES:
        if len(argv) > 2 and name not in argv[2:]:
            continue
        before = len(fails)
        fn()
        torch.cuda.synchronize()
        say("KERNEL", name, "failures", len(fails) - before)
    say("DONE failures", len(fails))
    for f in fails[:40]:
        say("FAILED", *f)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
