"""Float64 references of the implicit-GEMM convolution family (csrc/seam_conv.hip) in plain torch.

Every helper runs on whatever device its inputs live on and never calls a convolution primitive: a convolution is a sum of
tap-wise ``matmul`` products in float64, so there is no per-shape algorithm search and no library kernel between the test and
the arithmetic.  Operands are taken as given: for the fp16 and split paths the caller rounds x and w first, so that the
reference sees exactly the values the kernel sees.

``igemm_mirror_f64`` is a host mirror of the kernels' own indexing -- the packed weight layout of ``seam_pack::igemm_value`` and
the chunk walk of ``setup()`` / ``advance_k()`` -- evaluated in float64.  tests/test_conv_refs_host.py holds it against the
tap-wise form, which pins the (r, s, c) / (r, c-chunk, s) orders on the CPU before any launch.
"""
import torch
import torch.nn.functional as F


def out_size(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


def conv_nhwc_f64(x, w, R, S, stride, pad, ho_crop=None, wo_crop=None):
    """x NHWC [N,H,W,C], w OIHW [K,C,R,S] -> NHWC float64 [N,Ho,Wo,K]; ``ho_crop, wo_crop``: the top-left part of the grid."""
    n, h, wd, c = x.shape
    k = w.shape[0]
    assert tuple(w.shape) == (k, c, R, S), (tuple(w.shape), (k, c, R, S))
    ho, wo = out_size(h, R, stride, pad), out_size(wd, S, stride, pad)
    if ho_crop is not None:
        assert 0 < ho_crop <= ho and 0 < wo_crop <= wo
        ho, wo = ho_crop, wo_crop
    assert ho > 0 and wo > 0
    xp = x.double()
    if pad:
        xp = F.pad(xp, (0, 0, pad, pad, pad, pad))
    wd64 = w.double()
    acc = torch.zeros((n * ho * wo, k), dtype=torch.float64, device=x.device)
    for r in range(R):
        for s in range(S):
            tap = xp[:, r:r + (ho - 1) * stride + 1:stride, s:s + (wo - 1) * stride + 1:stride, :]
            acc += tap.reshape(-1, c) @ wd64[:, :, r, s].t()
    return acc.view(n, ho, wo, k)


def epilogue_f64(acc, scale, shift, res, mode):
    """acc*scale + shift; mode 0 / 1: + res, then ReLU for mode 1; mode 2: times the mask ``res > 0`` (the backward of a ReLU)."""
    y = acc.double()
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if mode == 2:
        assert res is not None
        return torch.where(res > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res.double()
    return torch.relu(y) if mode == 1 else y


def nearest_index(out, inp):
    """Source index of every destination index, as seam_fpn::nearest_src computes it in float32:
    min(int(floor(float32(dst) * (float32(inp) / float32(out)))), inp - 1)."""
    scale = torch.tensor(float(inp), dtype=torch.float32) / torch.tensor(float(out), dtype=torch.float32)
    src = torch.floor(torch.arange(out, dtype=torch.float32) * scale).to(torch.int64)
    return torch.clamp(src, max=inp - 1)


def nearest_up_f64(top, Ho, Wo):
    """top NHWC [N,rH,rW,K] -> float64 [N,Ho,Wo,K], nearest neighbour."""
    _, rh, rw, _ = top.shape
    hi = nearest_index(Ho, rh).to(top.device)
    wi = nearest_index(Wo, rw).to(top.device)
    return top.double()[:, hi][:, :, wi]


def dual_f64(x1, x2, w, stride2):
    """W[:, :C1] . x1 + W[:, C1:] . x2[:, ::stride2, ::stride2][:, :Ho, :Wo]; x1 [N,Ho,Wo,C1], x2 [N,H2,W2,C2], w [K, C1+C2]."""
    n, ho, wo, c1 = x1.shape
    c2 = x2.shape[3]
    w2d = w.reshape(w.shape[0], -1).double()
    assert w2d.shape[1] == c1 + c2
    xs = x2[:, ::stride2, ::stride2][:, :ho, :wo]
    assert xs.shape[1] == ho and xs.shape[2] == wo
    acc = x1.double().reshape(-1, c1) @ w2d[:, :c1].t() + xs.double().reshape(-1, c2) @ w2d[:, c1:].t()
    return acc.view(n, ho, wo, -1)


def conv_transpose2x2_subpixel_f64(x, w):
    """ConvTranspose2d, 2x2 kernel, stride 2, in the sub-pixel layout of the mode-1 weight pack: x NHWC [N,H,W,Cin],
    w [Cin,Cout,2,2] -> [N,H,W,4*Cout] with channel (a*2 + b)*Cout + co = output pixel (2h + a, 2w + b), channel co."""
    n, h, wd, cin = x.shape
    cout = w.shape[1]
    assert tuple(w.shape) == (cin, cout, 2, 2)
    wm = w.double().permute(0, 2, 3, 1).reshape(cin, 4 * cout)
    return (x.double().reshape(-1, cin) @ wm).view(n, h, wd, 4 * cout)


def subpixel_to_nchw(y, cout):
    """[N,H,W,4*Cout] of conv_transpose2x2_subpixel_f64 -> NCHW [N,Cout,2H,2W]"""
    n, h, wd, _ = y.shape
    return y.view(n, h, wd, 2, 2, cout).permute(0, 5, 1, 3, 2, 4).reshape(n, cout, 2 * h, 2 * wd)


def dgrad_f64(dy, w, pad_fwd):
    """Input gradient of a stride-1 convolution y = conv(x, w, pad_fwd): dy NHWC [N,Ho,Wo,Cout], w OIHW [Cout,Cin,R,S]
    -> dx NHWC [N,H,W,Cin] = conv(dy, w rotated by 180 degrees with its channels swapped, pad R-1-pad_fwd) (R == S)."""
    cout, cin, R, S = w.shape
    assert R == S and 0 <= pad_fwd <= R - 1
    wr = torch.flip(w, (2, 3)).permute(1, 0, 2, 3).contiguous()
    return conv_nhwc_f64(dy, wr, R, S, 1, R - 1 - pad_fwd)


# ------------------------------------------------------------------------------------------------ the kernels' own indexing
def igemm_pack_mirror(w, K, Cin, R, S, Cstore, bke, mode=0):
    """seam_pack::igemm_value on the host: the reduction-ordered weight matrix [K, kred] (rows and slabs left out: they only
    place a row in memory).  Chunk q, column col -> (r, s, c): C >= one chunk: (r, c-chunk, s); smaller: plain (r, s, c)."""
    kred = ((R * S * Cstore + bke - 1) // bke) * bke
    out = torch.zeros((K, kred), dtype=torch.float64)
    w = w.double()
    for kk in range(kred):
        q, col = divmod(kk, bke)
        if Cstore >= bke:
            ccn = Cstore // bke
            s2 = q % S
            c = ((q // S) % ccn) * bke + col
            r = q // (S * ccn)
        else:
            pos, c = divmod(kk, Cstore)
            r, s2 = divmod(pos, S)
        if c >= Cin or r >= R:
            continue
        if mode == 0:
            out[:, kk] = w[:, c, r, s2]
        elif mode == 2:
            out[:, kk] = w[c, :, R - 1 - r, S - 1 - s2]
        else:
            cout = K // 4
            out[:, kk] = w[c].permute(1, 2, 0).reshape(4 * cout)          # row = (a*2 + b)*Cout + co
    return out


def igemm_gather_mirror(x, R, S, stride, pad, bke, epv, ho_crop=None, wo_crop=None):
    """The A operand as the kernels gather it: [M, kred] float64.  A row's chunk is eight 16-byte vectors (epv elements each);
    vector ``lcol`` starts at (kr, ks, kc) from setup() and moves on by advance_k(); a tap outside the input, or kr >= R, reads 0."""
    n, h, wd, c = x.shape
    ho, wo = out_size(h, R, stride, pad), out_size(wd, S, stride, pad)
    if ho_crop is not None:
        ho, wo = ho_crop, wo_crop
    kred = ((R * S * c + bke - 1) // bke) * bke
    nk = kred // bke
    a = torch.zeros((n, ho, wo, kred), dtype=torch.float64)
    xd = x.double()
    for lcol in range(8):
        kk = lcol * epv
        pos = kk // c
        kc = kk - pos * c
        kr = pos // S
        ks = pos - kr * S
        for q in range(nk):
            if kr < R:
                for oh in range(ho):
                    ih = oh * stride - pad + kr
                    if not 0 <= ih < h:
                        continue
                    for ow in range(wo):
                        iw = ow * stride - pad + ks
                        if 0 <= iw < wd:
                            a[:, oh, ow, q * bke + kk:q * bke + kk + epv] = xd[:, ih, iw, kc:kc + epv]
            # advance_k()
            if c >= bke:
                ks += 1
                if ks == S:
                    ks = 0
                    kc += bke
                    if kc >= c:
                        kc -= c
                        kr += 1
            else:
                kc += bke
                while kc >= c:
                    kc -= c
                    ks += 1
                    if ks == S:
                        ks = 0
                        kr += 1
    return a.view(n * ho * wo, kred), (n, ho, wo)


def igemm_mirror_f64(x, w, R, S, stride, pad, bke, epv, ho_crop=None, wo_crop=None, mode=0, K=None, Cin=None):
    """Gather times pack: what the implicit GEMM computes, from the kernels' index arithmetic alone."""
    c = x.shape[3]
    K = w.shape[0] if K is None else K
    Cin = w.shape[1] if Cin is None else Cin
    a, (n, ho, wo) = igemm_gather_mirror(x, R, S, stride, pad, bke, epv, ho_crop, wo_crop)
    b = igemm_pack_mirror(w, K, Cin, R, S, c, bke, mode)
    return (a @ b.t()).view(n, ho, wo, K)
