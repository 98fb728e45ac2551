#!/usr/bin/env python3
"""CPU emulation of conv3x3_wino24sx's arithmetic (csrc/seam_wino24sx.hip), the figure its test tolerance rests on: F(2x4,3x3) with
fp32 transforms, U from float64 rounded once, the position GEMMs as bf16-plane products (three truncation planes per operand)
accumulated in fp32 per 16-channel k-step in the kernel's term order -- six terms and all nine -- against the fp32 F(2x4,3x3) form
(fp32 products, summed per 8-channel chunk), the exact fp32 convolution and float64.  Prints e = max|y - y64| / max|y64| of each
and the ratio e_six / e_f32wino.  The emulation sums a k-step's 16 products in fp32 one after the other; the MFMA's internal
summation is wider, so the GPU's ratios come out lower.  torch only; no GPU.
usage: w24sx_noise_probe.py [N,H,W,C,K,pad ...]"""
import sys
import torch

DEFAULT = ["1,8,8,64,64,1", "2,9,11,64,64,1", "3,14,14,128,64,1", "1,20,28,64,128,1", "1,10,10,192,64,0", "1,25,25,512,64,1"]

G2 = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float64)
B2T = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float64)
A2T = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float64)
G4 = torch.tensor([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
                  dtype=torch.float64)
B4T = torch.tensor([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0],
                    [0, 4, 0, -5, 0, 1]], dtype=torch.float64)
A4T = torch.tensor([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=torch.float64)


def planes(x):
    """the three truncation planes of fp32 x (each a bf16 value held in fp32); they sum to x exactly"""
    top = lambda t: (t.view(torch.int32) & -65536).view(torch.float32)
    p0 = top(x)
    r = x - p0
    p1 = top(r)
    return p0, p1, r - p1


def tiles(x, pad):
    """x [N,C,H,W] -> d [N,C,ty,tx,4,6] (fp32), the 4 x 6 input tiles of the 2 x 4 output tiles"""
    n, c, h, w = x.shape
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    ty, tx = (ho + 1) // 2, (wo + 3) // 4
    xp = torch.zeros((n, c, 2 * ty + 2, 4 * tx + 2), dtype=x.dtype)
    xp[:, :, pad:pad + h, pad:pad + w] = x
    return xp.unfold(2, 4, 2).unfold(3, 6, 4), ho, wo


def run(x, wt, pad, mode):
    n, c, h, w = x.shape
    k = wt.shape[0]
    d, ho, wo = tiles(x, pad)
    # fp32 transforms (the multipliers are small integers: the fp32 matmul of a 4- or 6-term row is the kernel's fma chain up to order)
    v = torch.einsum("ij,nctsjl,ml->nctsim", B2T.float(), d, B4T.float())                      # [N,C,ty,tx,4,6]
    u = torch.einsum("ij,kcjl,ml->kcim", G2, wt.double(), G4).float()                          # fp64, one rounding
    nn_, _, ty, tx = v.shape[:4]
    vm = v.permute(4, 5, 0, 2, 3, 1).reshape(24, -1, c)                                        # [p, tile, c]
    um = u.permute(2, 3, 0, 1).reshape(24, k, c)                                               # [p, k, c]
    step = 8 if mode == "f32" else 16
    acc = torch.zeros((24, vm.shape[1], k), dtype=torch.float32)
    if mode != "f32":
        vp, up = planes(vm), planes(um)
        terms = [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)] if mode == "six" else \
                [(2, 2), (2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]
    for s in range(0, c, step):
        if mode == "f32":
            for cc in range(s, s + step):                                                      # one fma per channel
                acc = torch.addcmul(acc, vm[:, :, cc:cc + 1], um[:, None, :, cc])
        else:
            for i, j in terms:                                                                 # bf16 x bf16 is exact in fp32
                for cc in range(s, s + step):
                    acc = acc + vp[i][:, :, cc:cc + 1] * up[j][:, None, :, cc]
    m = acc.reshape(4, 6, nn_, ty, tx, k)
    y = torch.einsum("ai,ijntsk,bj->nktasb", A2T.float(), m, A4T.float()).reshape(nn_, k, 2 * ty, 4 * tx)
    return y[:, :, :ho, :wo]


def main(argv):
    print(f"{'N,H,W,C,K,pad':>18} {'e_exact':>9} {'e_f32wino':>9} {'e_six':>9} {'e_nine':>9} {'six/f32wino':>11}")
    for s in argv or DEFAULT:
        n, h, w, c, k, pad = map(int, s.split(","))
        g = torch.Generator().manual_seed(1)
        x = torch.relu(torch.randn((n, c, h, w), generator=g))
        wt = torch.randn((k, c, 3, 3), generator=g) / (9 * c) ** 0.5
        y64 = torch.nn.functional.conv2d(x.double(), wt.double(), None, 1, pad)
        e = lambda y: float((y.double() - y64).abs().max() / y64.abs().max())
        e_ex = e(torch.nn.functional.conv2d(x, wt, None, 1, pad))
        e_f, e_6, e_9 = (e(run(x, wt, pad, mode)) for mode in ("f32", "six", "nine"))
        print(f"{s:>18} {e_ex:9.2e} {e_f:9.2e} {e_6:9.2e} {e_9:9.2e} {e_6 / e_f:11.2f}", flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
