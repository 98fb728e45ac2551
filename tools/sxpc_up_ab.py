#!/usr/bin/env python3
"""The split classes ``lat`` and ``mdeconv`` against the exact kernels they replace: the FPN's three merging laterals
(conv1x1_sxpc_up against pw_sw_kernel<..,2> / seam_conv2d_upres_f32), the C5 lateral and the mask head's deconvolution GEMM
(conv1x1_sxpc against conv_igemm<float> / pw_sw_kernel) on the maps of an 800 x 800 frame at 80 frames (a step), 40, 5 and one -- the
deconvolution at 32 ROIs per frame: an interleaved same-process A/B (GPU box), in the form of tools/sxpc_dual_ab.py.

Each of ROUNDS rounds times every variant once (REPS launches between two events), variants in turn inside the round.  Reported per
shape: the median over the rounds and the spread (max - min) / median of either kernel, the ratio of the medians, the split kernel's
algorithmic TFLOP/s, whether it gives the bits of its un-fused fallback (conv_igemm_sx on the same pack, then upsample_add_) and its
largest difference from the exact kernel relative to the output's scale.  The tile rule is off (ops.SXPC_RULE = False): the table
shows what the rule should say.  `--abl name=lib.so ...` adds timing-only builds of the new kernel (tools/sxpc_abl_build.sh:
SEAM_SXPC_ABL bits), run on the lateral named by ABL_ON.
usage: sxpc_up_ab.py [--abl name=path ...] [N,Ho,Wo,C,K,rH,rW,relu ...]      (rH = 0: no coarse map, the plain kernel)"""
import ctypes as C
import os
import statistics
import sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from seam_match_rcnn_amd import _native, ops

LAYERS = [("P2 lateral", "{n},200,200,256,256,100,100,0"), ("P3 lateral", "{n},100,100,512,256,50,50,0"),
          ("P4 lateral", "{n},50,50,1024,256,25,25,0"), ("C5 lateral", "{n},25,25,2048,256,0,0,0"), ("mask deconv", "{r},14,14,256,1024,0,0,1")]
DEFAULT = [(f"{name} x{n}", s.format(n=n, r=32 * n)) for n in (80, 40, 5, 1) for name, s in LAYERS]
ABL_ON = "P3 lateral x80"
ROUNDS, REPS = 5, 10
args = sys.argv[1:]
abl = []
while args and args[0] == "--abl":
    name, path = args[1].split("=", 1)
    lib = C.CDLL(os.path.abspath(path))
    lib.seam_conv1x1_sxpc_up.restype = C.c_int
    lib.seam_conv1x1_sxpc_up.argtypes = _native.SIGNATURES["seam_conv1x1_sxpc_up"][1]
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


hdr = (f"{'layer':>16} {'N,Ho,Wo,C,K,rH,rW,relu':>30} {'exact kernel':>26} {'exact us':>9} {'spread':>6} {'split us':>8} {'spread':>6} {'TF/s':>6} "
       f"{'x':>5} {'wins':>5} {'same bits':>9} {'vs exact':>9}")
print(hdr + "".join(f" {n + ' us':>16}" for n, _ in abl))
for label, s in shapes:
    n, ho, wo, c, k, rh, rw, relu = map(int, s.split(","))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    x = torch.relu(torch.randn(n, ho, wo, c, device=dev, generator=g))          # post-ReLU operands, as the layers see them
    top = torch.randn(n, rh, rw, k, device=dev, generator=g) if rh else None
    w = torch.randn(k, c, 1, 1, device=dev, generator=g) / c ** 0.5
    bias = torch.randn(k, device=dev, generator=g) * 0.1
    exact, split = ops.pack_conv(w, bias, dtype=(torch.float32, ops.SX6))
    assert split.wx is not None
    yc = torch.empty((n, ho, wo, k), device=dev)

    def run(pc):
        return ops.conv2d_topdown(x, pc, top) if rh else ops.conv2d(x, pc, relu=bool(relu))

    def run_abl(lib):
        lib.seam_conv1x1_sxpc_up(ops._ptr(x), ops._ptr(split.wx), ops._ptr(split.scale), ops._ptr(split.shift), ops._ptr(top), ops._ptr(yc),
                                 n, ho, wo, c, k, rh, rw, relu, ops._stream())

    ops.CONV_TRACE = []
    ya, yb = run(exact), run(split)
    names = [t[0] for t in ops.CONV_TRACE]
    ops.CONV_TRACE = None
    assert names[1] == ("conv1x1_sxpc_up" if rh else "conv1x1_sxpc"), names
    ops.SXPC = False
    yf = run(split)                     # the fallback: the same pack on conv_igemm_sx (+ upsample_add_)
    ops.SXPC = True
    torch.cuda.synchronize()
    same = torch.equal(yb, yf)
    rel = float((yb - ya).abs().max()) / float(ya.abs().max())
    del yf
    use_abl = abl if rh and (label == ABL_ON or not label) else []
    for _, lib in use_abl:
        run_abl(lib)
    ta, tb, tx = [], [], [[] for _ in use_abl]
    for _ in range(ROUNDS):
        ta.append(timed(lambda: run(exact)))
        tb.append(timed(lambda: run(split)))
        for i, (_, lib) in enumerate(use_abl):
            tx[i].append(timed(lambda: run_abl(lib)))
    ma, sa = med_spread(ta)
    mb, sb = med_spread(tb)
    fl = 2.0 * n * ho * wo * c * k
    wins = ma / mb > 1 + max(sa, sb)    # by more than both kernels' spreads
    print(f"{label:>16} {s:>30} {names[0]:>26} {ma:9.1f} {sa:6.3f} {mb:8.1f} {sb:6.3f} {fl / mb / 1e6:6.1f} {ma / mb:5.2f} {str(wins):>5} "
          f"{str(same):>9} {rel:9.2e}" + "".join(f" {statistics.median(v):16.1f}" for v in tx), flush=True)
    del x, top, ya, yb, yc
