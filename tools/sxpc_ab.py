#!/usr/bin/env python3
"""conv1x1_sxpc (csrc/seam_pwsx.hip) against conv_igemm_sx<.., 6> on the 1x1 layers the split classes of the fp32 path run in a
step (40 frames per stream slice) plus the top FPN lateral: an interleaved same-process A/B (GPU box).

Each of ROUNDS rounds times every variant once (REPS launches between two events), variants in turn inside the round, so that a
drifting clock moves all of them alike.  Reported per shape: the median over the rounds and the spread (max - min) / median of
either kernel, the ratio of the medians, and whether the two outputs are the same bits.  `--abl name=lib.so ...` adds timing-only
builds of the new kernel (tools/sxpc_abl_build.sh: SEAM_SXPC_ABL bits) -- their outputs are wrong by construction and are not
compared.
usage: sxpc_ab.py [--abl name=path ...] [N,H,W,C,K,res,relu ...]"""
import ctypes as C
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from seam_match_rcnn_amd import _native, ops

# the 23 launches of a step by shape (x count), 40 frames of 800 x 800: c1 = bottleneck reductions (ReLU), c3 = plain expansions
# with their residual (ReLU); then the C5 lateral of the FPN (80 frames, bias only)
DEFAULT = [("c1 layer1 x2", "40,200,200,256,64,0,1"), ("c1 layer2.0", "40,200,200,256,128,0,1"), ("c1 layer2 x3", "40,100,100,512,128,0,1"),
           ("c1 layer3.0", "40,100,100,512,256,0,1"), ("c1 layer3 x5", "40,50,50,1024,256,0,1"), ("c1 layer4.0", "40,50,50,1024,512,0,1"),
           ("c1 layer4 x2", "40,25,25,2048,512,0,1"), ("c3 layer3 x5", "40,50,50,256,1024,1,1"), ("c3 layer4 x2", "40,25,25,512,2048,1,1"),
           ("C5 lateral", "80,25,25,2048,256,0,0")]
ROUNDS, REPS = 5, 10
args = sys.argv[1:]
abl = []
while args and args[0] == "--abl":
    name, path = args[1].split("=", 1)
    lib = C.CDLL(os.path.abspath(path))
    lib.seam_conv1x1_sxpc.restype = C.c_int
    lib.seam_conv1x1_sxpc.argtypes = _native.SIGNATURES["seam_conv1x1_sxpc"][1]
    abl.append((name, lib))
    args = args[2:]
shapes = [("", a) for a in args] or DEFAULT
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


hdr = f"{'layer':>13} {'N,H,W,C,K,res,relu':>24} {'igemm_sx us':>11} {'spread':>6} {'sxpc us':>8} {'spread':>6} {'TF/s':>6} {'x':>5} {'same bits':>9}"
print(hdr + "".join(f" {n + ' us':>12} {'spread':>6}" for n, _ in abl))
for label, s in shapes:
    n, h, w, c, k, res, relu = map(int, s.split(","))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.relu(torch.randn(n, h, w, c, device=dev, generator=g))            # post-ReLU operands, as the layers see them
    wt = torch.randn(k, c, 1, 1, device=dev, generator=g) / c ** 0.5
    bn = (torch.rand(k, device=dev, generator=g) + 0.5, torch.randn(k, device=dev, generator=g) * 0.1,
          torch.randn(k, device=dev, generator=g) * 0.1, torch.rand(k, device=dev, generator=g) + 0.5)
    r = torch.randn(n, h, w, k, device=dev, generator=g) if res else None
    pc = ops.pack_conv(wt, None, bn, dtype=ops.SX6)
    if pc.wx is None:
        ops.SXPC = False
        y = ops.conv2d(x, pc, bool(relu), r)
        t = [timed(lambda: ops.conv2d(x, pc, bool(relu), r, out=y)) for _ in range(ROUNDS)]
        ops.SXPC = True
        m, sp = med_spread(t)
        print(f"{label:>13} {s:>24} {m:11.1f} {sp:6.3f} {'not served':>8}")
        continue
    ya = torch.empty((n, h, w, k), device=dev)
    yb = torch.empty_like(ya)
    yc = torch.empty_like(ya)

    def run_a():
        ops.SXPC = False
        ops.conv2d(x, pc, bool(relu), r, out=ya)

    def run_b():
        ops.SXPC = True
        ops.conv2d(x, pc, bool(relu), r, out=yb)

    def run_abl(lib):
        lib.seam_conv1x1_sxpc(ops._ptr(x), ops._ptr(pc.wx), ops._ptr(pc.scale), ops._ptr(pc.shift), ops._ptr(r), ops._ptr(yc), n * h * w, c, k,
                              relu, ops._stream())

    ops.CONV_TRACE = []
    run_a(); run_b()
    names = [t[0] for t in ops.CONV_TRACE]
    ops.CONV_TRACE = None
    assert names[0].startswith("conv_igemm_sx") and names[1] == "conv1x1_sxpc", names
    for _, lib in abl:
        run_abl(lib)
    torch.cuda.synchronize()
    same = torch.equal(ya, yb)
    ta, tb, tx = [], [], [[] for _ in abl]
    for _ in range(ROUNDS):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        for i, (_, lib) in enumerate(abl):
            tx[i].append(timed(lambda: run_abl(lib)))
    ma, sa = med_spread(ta)
    mb, sb = med_spread(tb)
    fl = 2.0 * n * h * w * c * k
    print(f"{label:>13} {s:>24} {ma:11.1f} {sa:6.3f} {mb:8.1f} {sb:6.3f} {fl / mb / 1e6:6.1f} {ma / mb:5.2f} {str(same):>9}"
          + "".join(f" {med_spread(v)[0]:12.1f} {med_spread(v)[1]:6.3f}" for v in tx), flush=True)
