#!/usr/bin/env python3
"""stem_sxpc and conv1x1_sxpc64 (csrc/seam_pwsx.hip) against the kernels they replace, at the shapes of a step: an interleaved
same-process A/B (GPU box).

  stem      the exact implicit GEMM over the unpadded space-to-depth frame (``conv2d(..., out_hw=)``, today's stem) against
            ``stem_s2d_sx`` over the padded frame; the outputs differ (six-term split products), the largest difference is printed
            against the output's scale
  c1 64     layer1's 256 -> 64 reduction: conv_igemm_sx against conv1x1_sxpc64 on the same SX6 pack (the same bits)
  c3 short  layer2's 128 -> 512 expansion with its residual: the exact conv1x1_sw against conv1x1_sxpc on two chunks
  c3ds short  layer1.0's conv3 + projection shortcut, 64 + 64 -> 256: the exact two-source conv1x1_sw against conv1x1_sxpc_dual

Each of ROUNDS rounds times every variant once (REPS launches between two events), variants in turn inside the round.  Reported per
shape: the median over the rounds and the spread (max - min) / median of either kernel, and the ratio of the medians.
`--abl name=lib.so ...` adds timing-only builds of the stem kernel (tools/sxpc_abl_build.sh: SEAM_SXPC_ABL bits).
usage: sxpc64_ab.py [--abl name=path ...] [frames ...]      (default: 80 40)"""
import ctypes as C
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from seam_match_rcnn_amd import _native, ops

ROUNDS, REPS = 5, 10
args = sys.argv[1:]
abl = []
while args and args[0] == "--abl":
    name, path = args[1].split("=", 1)
    lib = C.CDLL(os.path.abspath(path))
    lib.seam_stem_sxpc.restype = C.c_int
    lib.seam_stem_sxpc.argtypes = _native.SIGNATURES["seam_stem_sxpc"][1]
    abl.append((name, lib))
    args = args[2:]
frames = [int(a) for a in args] or [80, 40]
dev = torch.device("cuda:0")
ops.SXPC_RULE = False


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / REPS


def med_spread(v):
    m = statistics.median(v)
    return m, (max(v) - min(v)) / m


def report(label, shape, flops, ta, tb, note, extra=()):
    (ma, sa), (mb, sb) = med_spread(ta), med_spread(tb)
    wins = ma - mb > max(sa * ma, sb * mb)
    print(f"{label:>10} {shape:>20} {ma:9.1f} {sa:6.3f} {mb:9.1f} {sb:6.3f} {flops / mb / 1e6:6.1f} {ma / mb:5.2f} {'yes' if wins else 'no':>5} {note}"
          + "".join(f" {statistics.median(v):10.1f}" for v in extra), flush=True)


print(f"{'layer':>10} {'shape':>20} {'old us':>9} {'spread':>6} {'new us':>9} {'spread':>6} {'TF/s':>6} {'x':>5} {'wins':>5} note"
      + "".join(f" {n + ' us':>10}" for n, _ in abl))
g = torch.Generator(device=dev)
g.manual_seed(1)
bn = lambda k: (torch.rand(k, device=dev, generator=g) + 0.5, torch.randn(k, device=dev, generator=g) * 0.1,
                torch.randn(k, device=dev, generator=g) * 0.1, torch.rand(k, device=dev, generator=g) + 0.5)
for n in frames:
    # ---- the stem: 800 x 800 frames, space-to-depth 400 x 400 x 12
    hs = ws = 400
    x = torch.randn(n, hs, ws, 12, device=dev, generator=g)
    xp = torch.nn.functional.pad(x, (0, 0, 2, 1, 2, 1)).contiguous()
    w4 = torch.randn(64, 12, 4, 4, device=dev, generator=g) / 147 ** 0.5
    b = bn(64)
    exact = ops.pack_conv(w4, None, b, stride=1, pad=2, cstore=12, wino=False)
    twin = ops.pack_conv(w4.permute(0, 2, 3, 1).reshape(64, 192, 1, 1).contiguous(), None, b, dtype=ops.SX6)
    ya = ops.conv2d(x, exact, relu=True, out_hw=(hs, ws))
    yb = ops.stem_s2d_sx(xp, twin, relu=True, padded=True)
    yc = torch.empty_like(yb)
    torch.cuda.synchronize()
    err = float((ya - yb).abs().max()) / float(ya.abs().max())
    del ya, yb

    def run_abl(lib):
        lib.seam_stem_sxpc(ops._ptr(xp), ops._ptr(twin.wx64), ops._ptr(twin.scale), ops._ptr(twin.shift), ops._ptr(yc), n, hs, ws, 1, ops._stream())

    ta, tb, tx = [], [], [[] for _ in abl]
    for _ in range(ROUNDS):
        ta.append(timed(lambda: ops.conv2d(x, exact, relu=True, out_hw=(hs, ws))))
        tb.append(timed(lambda: ops.stem_s2d_sx(xp, twin, relu=True, padded=True)))
        for i, (_, lib) in enumerate(abl):
            tx[i].append(timed(lambda: run_abl(lib)))
    report("stem", f"{n},{hs},{ws},12->64 4x4", 2.0 * n * hs * ws * 192 * 64, ta, tb, f"max diff / scale {err:.1e}", tx)
    del x, xp, yc
    # ---- layer1's 256 -> 64 reduction at 200 x 200
    x = torch.relu(torch.randn(n, 200, 200, 256, device=dev, generator=g))
    pc = ops.pack_conv(torch.randn(64, 256, 1, 1, device=dev, generator=g) / 16, None, bn(64), dtype=ops.SX6)
    ya, yb = torch.empty((n, 200, 200, 64), device=dev), torch.empty((n, 200, 200, 64), device=dev)

    def run(on, y):
        ops.SXPC64 = on
        ops.conv2d(x, pc, True, out=y)

    ops.CONV_TRACE = []
    run(False, ya); run(True, yb)
    names = [t[0] for t in ops.CONV_TRACE]
    ops.CONV_TRACE = None
    assert names[0].startswith("conv_igemm_sx") and names[1] == "conv1x1_sxpc64", names
    torch.cuda.synchronize()
    same = torch.equal(ya, yb)
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(lambda: run(False, ya)))
        tb.append(timed(lambda: run(True, yb)))
    report("c1 64", f"{n},200,200,256->64", 2.0 * n * 200 * 200 * 256 * 64, ta, tb, f"same bits {same}")
    del x, ya, yb
    # ---- layer2's 128 -> 512 expansion with its residual at 100 x 100: the exact conv1x1_sw against conv1x1_sxpc on two chunks
    x = torch.relu(torch.randn(n, 100, 100, 128, device=dev, generator=g))
    r = torch.relu(torch.randn(n, 100, 100, 512, device=dev, generator=g))
    wt, b = torch.randn(512, 128, 1, 1, device=dev, generator=g) / 128 ** 0.5, bn(512)
    exact, twin = ops.pack_conv(wt, None, b), ops.pack_conv(wt, None, b, dtype=ops.SX6)
    ya, yb = torch.empty((n, 100, 100, 512), device=dev), torch.empty((n, 100, 100, 512), device=dev)
    ops.CONV_TRACE = []
    ops.conv2d(x, exact, True, r, out=ya); ops.conv2d(x, twin, True, r, out=yb)
    names = [t[0] for t in ops.CONV_TRACE]
    ops.CONV_TRACE = None
    assert names[0].startswith("conv1x1_sw") and names[1] == "conv1x1_sxpc_short", names
    torch.cuda.synchronize()
    err = float((ya - yb).abs().max()) / float(ya.abs().max())
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(lambda: ops.conv2d(x, exact, True, r, out=ya)))
        tb.append(timed(lambda: ops.conv2d(x, twin, True, r, out=yb)))
    report("c3 short", f"{n},100,100,128->512+r", 2.0 * n * 100 * 100 * 128 * 512, ta, tb, f"max diff / scale {err:.1e}")
    del x, r, ya, yb
    # ---- layer1.0's conv3 + projection shortcut at 200 x 200: the exact two-source conv1x1_sw against conv1x1_sxpc_dual on two chunks
    x1 = torch.relu(torch.randn(n, 200, 200, 64, device=dev, generator=g))
    x2 = torch.relu(torch.randn(n, 200, 200, 64, device=dev, generator=g))
    w1, w2 = (torch.randn(256, 64, 1, 1, device=dev, generator=g) / 8 for _ in range(2))
    exact, twin = ops.pack_conv_dual(w1, bn(256), w2, bn(256), dtype=(ops.F32, ops.SX6))
    ops.CONV_TRACE = []
    ya, yb = ops.conv2d_dual(x1, x2, exact, 1, relu=True), ops.conv2d_dual(x1, x2, twin, 1, relu=True)
    names = [t[0] for t in ops.CONV_TRACE]
    ops.CONV_TRACE = None
    assert names[0].startswith("conv1x1_sw") and names[1] == "conv1x1_sxpc_dual_short", names
    torch.cuda.synchronize()
    err = float((ya - yb).abs().max()) / float(ya.abs().max())
    del ya, yb
    ta, tb = [], []
    for _ in range(ROUNDS):
        ta.append(timed(lambda: ops.conv2d_dual(x1, x2, exact, 1, relu=True)))
        tb.append(timed(lambda: ops.conv2d_dual(x1, x2, twin, 1, relu=True)))
    report("c3ds short", f"{n},200,200,64+64->256", 2.0 * n * 200 * 200 * 128 * 256, ta, tb, f"max diff / scale {err:.1e}")
    del x1, x2
