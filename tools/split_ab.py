#!/usr/bin/env python3
"""Same-process interleaved A/B of the three-plane split kernels (ops.SX6 / ops.SX9) against the exact-fp32 kernel that serves
each layer today, at the shapes of the flagship step (800 x 800 frames, 40 per stream slice).  Per shape: ROUNDS rounds, each
timing REPS launches of every variant in turn; prints the median and the min..max spread of the per-round means.
usage: split_ab.py [N,H,W,C,K,R,stride,pad,res ...]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from seam_match_rcnn_amd import ops

DEFAULT = [  # class c1: bottleneck reductions
           "40,200,200,256,64,1,1,0,0", "40,100,100,512,128,1,1,0,0", "40,50,50,1024,256,1,1,0,0", "40,25,25,2048,512,1,1,0,0",
           # class c3: expansions + residual
           "40,200,200,64,256,1,1,0,1", "40,100,100,128,512,1,1,0,1", "40,50,50,256,1024,1,1,0,1", "40,25,25,512,2048,1,1,0,1",
           # class c2s2: the stride-2 3x3s
           "40,200,200,128,128,3,2,1,0", "40,100,100,256,256,3,2,1,0", "40,50,50,512,512,3,2,1,0",
           # FPN lateral C5, mask deconv (as its 1x1 GEMM)
           "80,25,25,2048,256,1,1,0,0", "320,14,14,256,1024,1,1,0,0"]
ROUNDS, REPS = 5, 8
shapes = [a for a in sys.argv[1:] if not a.startswith("--")] or DEFAULT
dev = torch.device("cuda:0")
print(f"{'N,H,W,C,K,R,s,p,res':>28} {'exact us':>9} {'spread':>13} {'six us':>8} {'spread':>13} {'nine us':>8} {'spread':>13} {'x six':>6} {'x nine':>6}  TF/s six")
for s in shapes:
    n, h, w, c, k, r, st, pad, res = map(int, s.split(","))
    x = torch.randn(n, h, w, c, device=dev)
    wt = torch.randn(k, c, r, r, device=dev) * 0.05
    bnp = (torch.rand(k, device=dev) + 0.5, torch.randn(k, device=dev), torch.randn(k, device=dev), torch.rand(k, device=dev) + 0.5)
    packs = [ops.pack_conv(wt, None, bnp, stride=st, pad=pad, dtype=d) for d in (torch.float32, ops.SX6, ops.SX9)]
    ho, wo = (h + 2 * pad - r) // st + 1, (w + 2 * pad - r) // st + 1
    resid = torch.randn(n, ho, wo, k, device=dev) if res else None
    y = torch.empty(n, ho, wo, k, device=dev)
    for pc in packs:
        ops.conv2d(x, pc, True, resid, out=y)
    torch.cuda.synchronize()
    t = [[], [], []]
    for _ in range(ROUNDS):
        for i, pc in enumerate(packs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                ops.conv2d(x, pc, True, resid, out=y)
            e1.record()
            torch.cuda.synchronize()
            t[i].append(e0.elapsed_time(e1) * 1e3 / REPS)
    med = [sorted(v)[len(v) // 2] for v in t]
    sp = [f"{min(v):.0f}..{max(v):.0f}" for v in t]
    fl = 2.0 * n * ho * wo * k * r * r * c
    print(f"{s:>28} {med[0]:9.1f} {sp[0]:>13} {med[1]:8.1f} {sp[1]:>13} {med[2]:8.1f} {sp[2]:>13} {med[0] / med[1]:6.2f} {med[0] / med[2]:6.2f}  {fl / med[1] / 1e6:7.1f}",
          flush=True)
