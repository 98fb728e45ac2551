#!/usr/bin/env python3
"""conv1x1_sxpc_dual (csrc/seam_pwsx.hip) against the exact two-source GEMM conv_igemm<float, .., DUAL> (seam_conv2d_dual_f32) on the
three projection-shortcut blocks of the fp32 path -- layer2.0 / layer3.0 / layer4.0 of an 800 x 800 frame -- at 40 frames (the stream
slice of a step), 80, 5 and one: an interleaved same-process A/B (GPU box), in the form of tools/sxpc_ab.py.

Each of ROUNDS rounds times every variant once (REPS launches between two events), variants in turn inside the round.  Reported per
shape: the median over the rounds and the spread (max - min) / median of either kernel, the ratio of the medians, the new kernel's
algorithmic TFLOP/s, whether it gives the bits of the fallback (gather + concatenate + conv_igemm_sx on the same pack) and its
largest difference from the exact kernel relative to the output's scale.  `--abl name=lib.so ...` adds timing-only builds of the
new kernel (tools/sxpc_abl_build.sh: SEAM_SXPC_ABL bits), run on the shapes named by --abl-on (default: layer3.0 at 40 frames).
usage: sxpc_dual_ab.py [--abl name=path ...] [N,Ho,Wo,C1,H2,W2,C2,stride2,K ...]"""
import ctypes as C
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from seam_match_rcnn_amd import _native, ops

LAYERS = [("layer2.0", "{n},100,100,128,200,200,256,2,512"), ("layer3.0", "{n},50,50,256,100,100,512,2,1024"),
          ("layer4.0", "{n},25,25,512,50,50,1024,2,2048")]
DEFAULT = [(f"{name} x{n}", s.format(n=n)) for n in (40, 80, 5, 1) for name, s in LAYERS]
ABL_ON = "layer3.0 x40"
ROUNDS, REPS = 5, 10
args = sys.argv[1:]
abl = []
while args and args[0] == "--abl":
    name, path = args[1].split("=", 1)
    lib = C.CDLL(os.path.abspath(path))
    lib.seam_conv1x1_sxpc_dual.restype = C.c_int
    lib.seam_conv1x1_sxpc_dual.argtypes = _native.SIGNATURES["seam_conv1x1_sxpc_dual"][1]
    abl.append((name, lib))
    args = args[2:]
shapes = [("", a) for a in args] or DEFAULT
dev = torch.device("cuda:0")


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


hdr = (f"{'layer':>13} {'N,Ho,Wo,C1,H2,W2,C2,s,K':>34} {'exact us':>9} {'spread':>6} {'dual us':>8} {'spread':>6} {'TF/s':>6} {'x':>5} "
       f"{'wins':>5} {'same bits':>9} {'vs exact':>9}")
print(hdr + "".join(f" {n + ' us':>16}" for n, _ in abl))
for label, s in shapes:
    n, ho, wo, c1, h2, w2, c2, st, k = map(int, s.split(","))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x1 = torch.relu(torch.randn(n, ho, wo, c1, device=dev, generator=g))          # post-ReLU operands, as the blocks see them
    x2 = torch.relu(torch.randn(n, h2, w2, c2, device=dev, generator=g))
    bn = lambda: (torch.rand(k, device=dev, generator=g) + 0.5, torch.randn(k, device=dev, generator=g) * 0.1,
                  torch.randn(k, device=dev, generator=g) * 0.1, torch.rand(k, device=dev, generator=g) + 0.5)
    w1 = torch.randn(k, c1, 1, 1, device=dev, generator=g) / (c1 + c2) ** 0.5
    w2_ = torch.randn(k, c2, 1, 1, device=dev, generator=g) / (c1 + c2) ** 0.5
    exact, split = ops.pack_conv_dual(w1, bn(), w2_, bn(), dtype=(torch.float32, ops.SX6))
    assert split.wx is not None
    yc = torch.empty((n, ho, wo, k), device=dev)

    def run_a():
        return ops.conv2d_dual(x1, x2, exact, st, relu=True)

    def run_b():
        return ops.conv2d_dual(x1, x2, split, st, relu=True)

    def run_abl(lib):
        lib.seam_conv1x1_sxpc_dual(ops._ptr(x1), ops._ptr(x2), ops._ptr(split.wx), ops._ptr(split.scale), ops._ptr(split.shift), ops._ptr(yc),
                                   n, ho, wo, c1, h2, w2, c2, st, k, 1, ops._stream())

    ops.CONV_TRACE = []
    ya, yb = run_a(), run_b()
    names = [t[0] for t in ops.CONV_TRACE]
    ops.CONV_TRACE = None
    assert names[0].startswith("conv_igemm<float") and names[1] == "conv1x1_sxpc_dual", names
    ops.SXPC = False
    yf = run_b()                        # the fallback: the same pack on conv_igemm_sx over the materialised rows
    ops.SXPC = True
    torch.cuda.synchronize()
    same = torch.equal(yb, yf)
    rel = float((yb - ya).abs().max()) / float(ya.abs().max())
    del yf
    use_abl = abl if label == ABL_ON or not label else []
    for _, lib in use_abl:
        run_abl(lib)
    ta, tb, tx = [], [], [[] for _ in use_abl]
    for _ in range(ROUNDS):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        for i, (_, lib) in enumerate(use_abl):
            tx[i].append(timed(lambda: run_abl(lib)))
    ma, sa = med_spread(ta)
    mb, sb = med_spread(tb)
    fl = 2.0 * n * ho * wo * (c1 + c2) * k
    wins = ma / mb > 1 + max(sa, sb)    # by more than both kernels' spreads
    print(f"{label:>13} {s:>34} {ma:9.1f} {sa:6.3f} {mb:8.1f} {sb:6.3f} {fl / mb / 1e6:6.1f} {ma / mb:5.2f} {str(wins):>5} {str(same):>9} {rel:9.2e}"
          + "".join(f" {statistics.median(v):16.1f}" for v in tx), flush=True)
    del x1, x2, ya, yb, yc
