"""Plain float64 references of the gradient kernels of ``csrc/seam_backward.hip``, and the error bounds the GPU sweep
(``test_gpu_stress_train.py``) holds each kernel to.  Device-agnostic: every function runs on whatever device its tensors
live on, so ``test_train_references.py`` checks them against ``torch.autograd`` on the CPU at tiny shapes.

Error bounds.  A fp32 sum of products evaluated as ONE sequential chain of L roundings (fmaf, MFMA accumulate, add) obeys
``|got - exact| <= gamma_L * sum|terms|`` with ``gamma_L = L u / (1 - L u)``, ``u = 2^-24`` (Higham, Accuracy and Stability,
sec. 3.1); any fixed tree of partial sums has a chain no longer than its depth plus its longest leaf chain.  Each term that
is itself rounded k times before it enters the chain adds k to L.  ``C_ERR = 2`` covers the 1 / (1 - L u) factor (L u < 0.5
in every case of the sweep) and the final rounding of the stored result, so the checks use ``C_ERR * U * L * sum|terms|``
with L stated next to each call.  ``sum|terms|`` is the same float64 reduction over absolute values (a majorant)."""
import math

import torch
import torch.nn.functional as F

U = 2.0 ** -24
C_ERR = 2.0
F64 = torch.float64


def bound(maj, L):
    return C_ERR * U * L * maj


# ------------------------------------------------------------------------------------------------ conv weight gradient
def wgrad(x, dy, R, S, stride, pad):
    """x NHWC [N,H,W,C], dy [N,Ho,Wo,K] -> dW [K,C,R,S] (OIHW): one matmul ``dy[M,K]^T @ x_shifted[M,C]`` per tap (r,s)."""
    x, dy = x.to(F64), dy.to(F64)
    n, h, w, c = x.shape
    ho, wo, k = dy.shape[1], dy.shape[2], dy.shape[3]
    xp = F.pad(x, (0, 0, pad, pad, pad, pad))
    d = dy.reshape(-1, k)
    out = torch.empty((k, c, R, S), dtype=F64, device=x.device)
    for r in range(R):
        for s in range(S):
            xs = xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, :]
            out[:, :, r, s] = d.t() @ xs.reshape(-1, c)
    return out


def wgrad_rows(x, dy, R, S, stride, pad, ks):
    """Rows ``ks`` of ``wgrad`` only (the reference of a shape whose full dW is too slow to form in float64)."""
    return wgrad(x, dy[..., ks], R, S, stride, pad)


def conv_out(h, w, R, S, stride, pad):
    return (h + 2 * pad - R) // stride + 1, (w + 2 * pad - S) // stride + 1


# ------------------------------------------------------------------------------------------------ small reductions
def colsum(x):
    return x.to(F64).reshape(-1, x.shape[-1]).sum(0)


def avgpool_relu_bwd(dpool, y):
    """dpool [N,C], y [N,HW,C] -> dy [N,HW,C] = (y > 0) * dpool / HW."""
    hw = y.shape[1]
    return torch.where(y > 0, dpool.to(F64)[:, None, :] / hw, torch.zeros((), dtype=F64, device=y.device))


def ulp32(v):
    """Spacing of fp32 at |v| (v float64): the size of one fp32 ulp there (the subnormal spacing at 0)."""
    a = v.abs().to(torch.float32)
    return (torch.nextafter(a, torch.full_like(a, math.inf)) - a).to(F64)


# ------------------------------------------------------------------------------------------------ BatchNorm1d
def bn_train(x, gamma, beta, run_mean, run_var, momentum, eps, dy):
    """nn.BatchNorm1d in training mode, float64 autograd -> dict(y, mean, invstd, run_mean, run_var, dx, dgamma, dbeta);
    run_* None: no running buffers (both returned as None)."""
    x = x.to(F64).detach().requires_grad_(True)
    g = gamma.to(F64).detach().requires_grad_(True)
    b = beta.to(F64).detach().requires_grad_(True)
    rm = None if run_mean is None else run_mean.to(F64).clone()
    rv = None if run_var is None else run_var.to(F64).clone()
    y = F.batch_norm(x, rm, rv, g, b, True, momentum, eps)
    y.backward(dy.to(F64))
    mean = x.detach().mean(0)
    invstd = 1.0 / torch.sqrt(x.detach().var(0, unbiased=False) + eps)
    return dict(y=y.detach(), mean=mean, invstd=invstd, run_mean=rm, run_var=rv, dx=x.grad, dgamma=g.grad, dbeta=b.grad)


def bn_backward(dy, x, mean, invstd, gamma, frozen):
    """The backward of BatchNorm1d at GIVEN saved statistics -- what seam_bn1d_bwd_f32 and torch's native backward compute
    from (dy, x, save_mean, save_invstd, gamma) -- in float64: xh = (x - mean) invstd, dbeta = sum dy, dgamma = sum dy xh,
    dx = gamma invstd (dy - dbeta / M - xh dgamma / M) (batch statistics) or gamma invstd dy (frozen).  At the batch's exact
    statistics this is autograd through the module (test_train_references.py)."""
    x, dy, g = x.to(F64), dy.to(F64), gamma.to(F64)
    m0, i0 = mean.to(F64), invstd.to(F64)
    M = x.shape[0]
    xh = (x - m0) * i0
    sb, sg = dy.sum(0), (dy * xh).sum(0)
    if frozen:
        dx = g * i0 * dy
    else:
        dx = g * i0 / M * (M * dy - sb - xh * sg)
    return dx, sg, sb


# ------------------------------------------------------------------------------------------------ pairwise classifier
def pair_bwd(a, b, w, g, chunk=32):
    """Gradients of x5[i,j,c] = sum_d w[c,d] (a_i - b_j)_d^2 + bias[c] for upstream g [Q,G,2], in closed form, chunked over Q
    -> (da, db, dw, dbias) and their majorants (the same sums over absolute values)."""
    a, b, w, g = a.to(F64), b.to(F64), w.to(F64), g.to(F64)
    da, db = torch.zeros_like(a), torch.zeros_like(b)
    mda, mdb = torch.zeros_like(a), torch.zeros_like(b)
    dw, mdw = torch.zeros_like(w), torch.zeros_like(w)
    for s in range(0, a.shape[0], chunk):
        df = a[s:s + chunk, None, :] - b[None, :, :]                       # [q,G,D]
        gs = g[s:s + chunk]                                                 # [q,G,2]
        co = torch.einsum("qgc,cd->qgd", gs, w)
        mco = torch.einsum("qgc,cd->qgd", gs.abs(), w.abs())
        da[s:s + chunk] = 2 * (df * co).sum(1)
        mda[s:s + chunk] = 2 * (df.abs() * mco).sum(1)
        db -= 2 * (df * co).sum(0)
        mdb += 2 * (df.abs() * mco).sum(0)
        dw += torch.einsum("qgc,qgd->cd", gs, df * df)
        mdw += torch.einsum("qgc,qgd->cd", gs.abs(), df * df)
    dbias = g.reshape(-1, 2).sum(0)
    mdbias = g.reshape(-1, 2).abs().sum(0)
    return (da, db, dw, dbias), (mda, mdb, mdw, mdbias)


# ------------------------------------------------------------------------------------------------ weighted 2-class CE
def ce2(logits, target, weight):
    """nn.CrossEntropyLoss(weight) (mean) in float64 -> (loss, dlogits).  The loss is torch's; dlogits is its closed form
    k (p1 - y) (-1, +1) with k = w_y / sum w and p1 - y = sigmoid(x1 - x0) or -sigmoid(x0 - x1): autograd's
    softmax - onehot cancels in the target's column once the softmax saturates (1 - p0 with p0 == 1.0 in float64 is 0, not
    -p1), and the kernel is more accurate than that there."""
    x = logits.to(F64)
    w = weight.to(F64)
    loss = F.cross_entropy(x, target, weight=w)
    wi = w[target]
    k = wi / wi.sum()
    d = x[:, 1] - x[:, 0]
    g1 = k * torch.where(target != 0, -torch.sigmoid(-d), torch.sigmoid(d))
    return loss, torch.stack([-g1, g1], 1)


# ------------------------------------------------------------------------------------------------ NLB + attention pooling
NLB_NAMES = ["theta.weight", "theta.bias", "phi.weight", "phi.bias", "g.weight", "g.bias", "concat_project.0.weight",
             "W.weight", "W.bias", "attention_scorer.weight", "attention_scorer.bias"]


def nlb_params(pk):
    """The eleven parameters in the reference's layouts (prefix ``newnlb.`` as oracle/heads.py expects) from a flat pack
    dict w_proj_t [256,384], b_proj [384], w_cat [256], w_out_t [128,256], b_out [256], w_att [256], b_att [1]."""
    wp = pk["w_proj_t"].t()
    vals = [wp[:128, :, None], pk["b_proj"][:128], wp[128:256, :, None], pk["b_proj"][128:256], wp[256:, :, None],
            pk["b_proj"][256:], pk["w_cat"].reshape(1, 256, 1, 1), pk["w_out_t"].t()[:, :, None], pk["b_out"],
            pk["w_att"].reshape(1, 256), pk["b_att"].reshape(1)]
    p = {}
    for nm, v in zip(NLB_NAMES, vals):
        p[("" if nm.startswith("attention") else "newnlb.") + nm] = v.to(F64).contiguous()
    return p


def _applies(use_nlb, t):
    return use_nlb == 2 or (use_nlb == 1 and t > 1)


def nlb_bwd(seqs, p, use_nlb, dout=None, dz=None, _major=None):
    """float64 autograd through oracle/heads.py: seqs = list of [T_s,256] (T_s >= 1), p from ``nlb_params``.
    dout [S,256]: the attention-pooled path (aggregate_sequences; use_nlb 2 also runs the block on length-1 sequences);
    dz = list of [T_s,256]: the block alone (nlb_closed_form).  -> (list of dX [T_s,256], dict name -> gradient)."""
    from oracle import heads as OH
    q = {k: v.detach().clone().requires_grad_(True) for k, v in p.items()}
    xs = [s.to(F64).detach().clone().requires_grad_(True) for s in seqs]
    total = 0.0
    for i, x in enumerate(xs):
        z = OH.nlb_closed_form(x, q) if _applies(use_nlb, x.shape[0]) else x
        if dz is None:
            if _major is not None:
                e = F.linear(z, q["attention_scorer.weight"], q["attention_scorer.bias"])
                o = (_MajorSoftmax.apply(e, _major[i]) * z).sum(0)
            else:
                o, _ = OH.attention_pool(z, q)
            total = total + (o * dout[i].to(F64)).sum()
        else:
            total = total + (z * dz[i].to(F64)).sum()
    grads = {}
    if xs:
        total.backward()
    dx = [x.grad if x.grad is not None else torch.zeros_like(x) for x in xs]
    for k, v in q.items():
        grads[k] = v.grad if v.grad is not None else torch.zeros_like(v)
    return dx, grads


def nlb_ab(x, p):
    """a_i = theta(x_i) . wc[:128], b_j = phi(x_j) . wc[128:] and their majorants (the ReLU argument is a_i + b_j)."""
    x = x.to(F64)
    wc = p["newnlb.concat_project.0.weight"].reshape(-1)
    th_w, ph_w = p["newnlb.theta.weight"][:, :, 0], p["newnlb.phi.weight"][:, :, 0]
    th_b, ph_b = p["newnlb.theta.bias"], p["newnlb.phi.bias"]
    a = (x @ th_w.t() + th_b) @ wc[:128]
    b = (x @ ph_w.t() + ph_b) @ wc[128:]
    ma = (x.abs() @ th_w.abs().t() + th_b.abs()) @ wc[:128].abs()
    mb = (x.abs() @ ph_w.abs().t() + ph_b.abs()) @ wc[128:].abs()
    return a, b, ma, mb


# a and b are each 256 fmaf + 1 bias add + 1 multiply by wc + a 64-lane butterfly (6) + 1 add of two wave sums: L = 265
NLB_AB_CHAIN = 265


def _integral(t):
    return bool(torch.equal(t, torch.round(t)))


def relu_margin_hits(x, p):
    """Number of pairs (i,j) whose ReLU argument a_i + b_j lies within the fp32 error bound of a and b -- where the kernel's
    mask may legitimately differ from the float64 one.  With integer x, theta / phi parameters and concat_project and
    |a| + |b| < 2^24 every partial sum is exact in fp32, so a, b and a + b are exact on both sides: no hit (an exact zero
    gives relu(0) = 0 and a zero gradient on both)."""
    a, b, ma, mb = nlb_ab(x, p)
    ab = ["newnlb.theta.weight", "newnlb.theta.bias", "newnlb.phi.weight", "newnlb.phi.bias", "newnlb.concat_project.0.weight"]
    if _integral(x) and all(_integral(p[k]) for k in ab) and float(ma.max() + mb.max()) < 2.0 ** 24:
        return 0
    s = a[:, None] + b[None, :]
    margin = bound(ma[:, None] + mb[None, :], NLB_AB_CHAIN)
    return int(((s.abs() <= margin) & (s != 0)).sum())


class _MajorSoftmax(torch.autograd.Function):
    """The REAL softmax values s (given) whose backward is the majorant s (g + sum s g) of the true s (g - sum s g), g >= 0."""

    @staticmethod
    def forward(ctx, e, s):
        ctx.save_for_backward(s)
        return s.clone()

    @staticmethod
    def backward(ctx, g):
        (s,) = ctx.saved_tensors
        return s * (g + (s * g).sum(0, keepdim=True)), None


def nlb_majorants(seqs, p, use_nlb, dout=None, dz=None):
    """Magnitude scale of every NLB backward output: the same float64 autograd with every input, parameter and upstream
    gradient replaced by its absolute value, ReLU(a_i + b_j) then the identity (its argument is >= 0, mask all on), the
    attention weights kept at their REAL softmax values s (positive) and the softmax backward s (g - sum s g) replaced by
    s (g + sum s g).  Every output is then a sum of the absolute values of the terms the true gradient sums."""
    from oracle import heads as OH
    pa = {k: v.abs() for k, v in p.items()}
    sa = [s.to(F64).abs() for s in seqs]
    if dz is None:
        with torch.no_grad():
            real = []
            for x in seqs:
                x = x.to(F64)
                z = OH.nlb_closed_form(x, p) if _applies(use_nlb, x.shape[0]) else x
                real.append(torch.softmax(F.linear(z, p["attention_scorer.weight"], p["attention_scorer.bias"]), 0))
        dx, grads = nlb_bwd(sa, pa, use_nlb, dout=dout.to(F64).abs(), _major=real)
    else:
        dx, grads = nlb_bwd(sa, pa, use_nlb, dz=[d.to(F64).abs() for d in dz])
    return [d.abs() for d in dx], {k: v.abs() for k, v in grads.items()}


def seq_rows(flat, t_stride, s_stride, lens, S, Tmax):
    """The live rows of every sequence of a strided [.., 256] buffer as the kernel reads them: sequence s is rows
    flat[s*s_stride + t*t_stride : +256] for t < min(len[s], Tmax) -- a length above Tmax is clamped, one <= 0 is empty."""
    out = []
    for s in range(S):
        T = max(0, min(int(lens[s]), Tmax))
        out.append(torch.as_strided(flat, (T, 256), (t_stride, 1), s * s_stride))
    return out
