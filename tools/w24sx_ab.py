#!/usr/bin/env python3
"""conv3x3_wino24sx (csrc/seam_wino24sx.hip) against seam_conv3x3_wino24_f32 (conv3x3_wino24pc on these shapes) on the ten stride-1
3x3 shapes a step runs on that kernel: an interleaved same-process A/B through the C ABI (GPU box).

Each of ROUNDS rounds times every variant once (REPS launches between two events), variants in turn inside the round, so that a
drifting clock moves all of them alike.  Reported per shape: the median over the rounds and the spread (max - min) / median of
either kernel, the ratio of the medians, and the largest difference of the two outputs over the output's largest value.
`--abl name=lib.so ...` adds timing-only builds of the new kernel (tools/w24sx_abl_build.sh: SEAM_W24SX_ABL bits) -- their
outputs are wrong by construction and are not compared.  `--frames F` scales the batches (80 frames / 2560 ROIs) to F frames.
`--nsplit 1,2,4` adds the tree's kernel with seam_conv3x3_wino24sx_set_nsplit forcing each value, in the same rounds: median, spread,
and whether its output is the `w24sx` column's bit for bit (that column runs under 0, the launcher's rule, unless W24SX_NSPLIT in
the environment names a forced value for the whole run).
usage: w24sx_ab.py [--frames F] [--nsplit a,b,..] [--abl name=path ...] [N,H,W,C,K,pad ...]"""
import ctypes as C
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from seam_match_rcnn_amd import _native, ops

# the launches of a step on conv3x3_wino24pc by shape (profiles/r06_breakdown_f32.txt), 80 frames / 2560 ROIs
DEFAULT = [("fpn/rpn 200^2", "80,200,200,256,256,1"), ("mask 14^2", "2560,14,14,256,256,1"), ("fpn/rpn 100^2", "80,100,100,256,256,1"),
           ("layer3/fpn 50^2", "80,50,50,256,256,1"), ("layer1 200^2", "80,200,200,64,64,1"), ("layer2 100^2", "80,100,100,128,128,1"),
           ("trunk 14->12", "2560,14,14,256,256,0"), ("layer4 25^2", "80,25,25,512,512,1"), ("trunk 12->10", "2560,12,12,256,256,0"),
           ("fpn/rpn 25^2", "80,25,25,256,256,1")]
ROUNDS, REPS = 5, 5
args = sys.argv[1:]
frames = 80
abl = []
forced = []
while args and args[0] in ("--abl", "--frames", "--nsplit"):
    if args[0] == "--frames":
        frames = int(args[1])
    elif args[0] == "--nsplit":
        forced = [int(v) for v in args[1].split(",")]
    else:
        name, path = args[1].split("=", 1)
        lib = C.CDLL(os.path.abspath(path))
        lib.seam_conv3x3_wino24sx_f32.restype = C.c_int
        lib.seam_conv3x3_wino24sx_f32.argtypes = _native.SIGNATURES["seam_conv3x3_wino24sx_f32"][1]
        abl.append((name, lib))
    args = args[2:]
shapes = [("", a) for a in args] or DEFAULT
dev = torch.device("cuda:0")
lib0 = _native.lib()
BASE_NSPLIT = int(os.environ.get("W24SX_NSPLIT", "0"))          # for a counter pass over one forced value (tools/pmc_w24.sh)
if BASE_NSPLIT:
    _native.check(lib0.seam_conv3x3_wino24sx_set_nsplit(BASE_NSPLIT), "set_nsplit")
P = ops._ptr


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


print(f"{'layer':>16} {'N,H,W,C,K,pad':>22} {'wino24 us':>10} {'spread':>6} {'w24sx us':>9} {'spread':>6} {'TF/s':>6} {'x':>5} {'max diff':>9}"
      + "".join(f" {'ns=%d us' % v:>9} {'spread':>6} {'bits':>4}" for v in forced) + "".join(f" {n + ' us':>14} {'spread':>6}" for n, _ in abl))
for label, s in shapes:
    n, h, w, c, k, pad = map(int, s.split(","))
    n = max(1, n * frames // 80)
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.relu(torch.randn(n, h, w, c, device=dev, generator=g))            # post-ReLU operands, as the layers see them
    wt = torch.randn(k, c, 3, 3, device=dev, generator=g) / (9 * c) ** 0.5
    sh = torch.randn(k, device=dev, generator=g) * 0.1
    u24 = torch.empty((int(lib0.seam_wino24_weight_floats(k, c)),), device=dev)
    _native.check(lib0.seam_pack_conv_weight_wino24_f32(P(wt), P(u24), k, c, c, 0, ops._stream()), "pack wino24")
    ux = torch.empty((int(lib0.seam_wino24sx_weight_bytes(k, c)),), dtype=torch.uint8, device=dev)
    _native.check(lib0.seam_pack_conv_weight_wino24_sx(P(wt), P(ux), k, c, c, 0, ops._stream()), "pack wino24sx")
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    ya = torch.empty((n, ho, wo, k), device=dev)
    yb = torch.empty_like(ya)
    yc = torch.empty_like(ya)

    def run_a():
        _native.check(lib0.seam_conv3x3_wino24_f32(P(x), P(u24), None, P(sh), None, P(ya), n, h, w, c, k, pad, 1, ops._stream()), "wino24")

    def run_b(lib=lib0, y=yb):
        _native.check(lib.seam_conv3x3_wino24sx_f32(P(x), P(ux), None, P(sh), None, P(y), n, h, w, c, k, pad, 1, 1, ops._stream()), "wino24sx")

    def run_ns(v, y=yc):
        _native.check(lib0.seam_conv3x3_wino24sx_set_nsplit(v), "set_nsplit")
        try:
            run_b(lib0, y)
        finally:
            lib0.seam_conv3x3_wino24sx_set_nsplit(BASE_NSPLIT)

    run_a(); run_b()
    same = []
    for v in forced:
        yc.fill_(float("nan"))
        run_ns(v)
        same.append(bool(torch.equal(yb.view(torch.int32), yc.view(torch.int32))))
    for _, lib in abl:
        run_b(lib, yc)
    torch.cuda.synchronize()
    diff = float((ya - yb).abs().max()) / float(ya.abs().max())
    ta, tb, tx, tn = [], [], [[] for _ in abl], [[] for _ in forced]
    for _ in range(ROUNDS):
        ta.append(timed(run_a))
        tb.append(timed(run_b))
        for i, v in enumerate(forced):
            tn[i].append(timed(lambda: run_ns(v)))
        for i, (_, lib) in enumerate(abl):
            tx[i].append(timed(lambda: run_b(lib, yc)))
    ma, sa = med_spread(ta)
    mb, sb = med_spread(tb)
    fl = 2.0 * n * ho * wo * c * k * 9
    print(f"{label:>16} {n:>6},{h},{w},{c},{k},{pad:<2} {ma:10.1f} {sa:6.3f} {mb:9.1f} {sb:6.3f} {fl / mb / 1e6:6.1f} {ma / mb:5.2f} {diff:9.2e}"
          + "".join(f" {med_spread(v)[0]:9.1f} {med_spread(v)[1]:6.3f} {'same' if ok else 'DIFF':>4}" for v, ok in zip(tn, same))
          + "".join(f" {med_spread(v)[0]:14.1f} {med_spread(v)[1]:6.3f}" for v in tx), flush=True)
    del x, ya, yb, yc
