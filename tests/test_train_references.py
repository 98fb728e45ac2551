"""The float64 references of ``train_refs.py`` (used by the GPU sweep ``test_gpu_stress_train.py``) against torch.autograd
and independent closed forms, on the CPU at tiny shapes: a wrong reference must neither pass nor fail the sweep."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_refs as TR
from oracle import heads as OH

F64 = torch.float64


def gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g).to(F64)


@pytest.mark.parametrize("n,h,w,c,k,r,s,stride,pad", [
    (2, 5, 6, 3, 4, 3, 3, 1, 1), (1, 7, 5, 2, 3, 1, 3, 2, 0), (3, 4, 4, 4, 2, 3, 1, 2, 2), (1, 1, 1, 5, 6, 1, 1, 1, 0),
    (2, 6, 6, 2, 2, 5, 5, 2, 4)])
def test_wgrad_matches_conv2d_autograd(n, h, w, c, k, r, s, stride, pad):
    g = gen(1)
    for integer in (False, True):
        x = ints((n, h, w, c), g) if integer else torch.randn((n, h, w, c), generator=g, dtype=F64)
        wt = torch.randn((k, c, r, s), dtype=F64, generator=g, requires_grad=True)
        y = F.conv2d(x.permute(0, 3, 1, 2), wt, None, stride, pad)
        assert y.shape[2:] == TR.conv_out(h, w, r, s, stride, pad)
        dy = ints(y.shape, g) if integer else torch.randn(y.shape, dtype=F64, generator=g)
        y.backward(dy)
        got = TR.wgrad(x, dy.permute(0, 2, 3, 1), r, s, stride, pad)
        if integer:                                   # small integers: every partial sum exact -> equality
            assert torch.equal(got, wt.grad)
            assert torch.equal(got, torch.round(got))
        else:
            torch.testing.assert_close(got, wt.grad, rtol=1e-12, atol=1e-12)
        ks = [k - 1, 0]
        assert torch.equal(TR.wgrad_rows(x, dy.permute(0, 2, 3, 1), r, s, stride, pad, ks), got[ks])
        maj = TR.wgrad(x.abs(), dy.permute(0, 2, 3, 1).abs(), r, s, stride, pad)
        assert bool((maj >= got.abs()).all())


def test_colsum_and_avgpool_relu_bwd():
    g = gen(2)
    x = torch.randn((7, 3, 5), generator=g, dtype=F64)
    torch.testing.assert_close(TR.colsum(x), x.sum((0, 1)), rtol=1e-15, atol=0)
    pre = torch.randn((3, 4, 6, 5), generator=g, dtype=F64, requires_grad=True)
    y = F.relu(pre)
    pool = F.relu(y.mean((1, 2)))
    dpool = torch.randn((3, 5), generator=g, dtype=F64)
    pool.backward(dpool)
    got = TR.avgpool_relu_bwd(dpool, y.detach().reshape(3, 24, 5))
    torch.testing.assert_close(got, pre.grad.reshape(3, 24, 5), rtol=1e-15, atol=0)
    v = torch.tensor([0.0, 1.0, -3.0, 1e-40], dtype=F64)
    assert TR.ulp32(v).tolist() == [2.0 ** -149, 2.0 ** -23, 2.0 ** -22, 2.0 ** -149]


@pytest.mark.parametrize("m,f,mom,buffers", [(2, 3, 0.1, True), (5, 4, 0.0, True), (9, 2, 1.0, True), (4, 3, 0.25, False)])
def test_bn_matches_module(m, f, mom, buffers):
    g = gen(3)
    x = torch.randn((m, f), generator=g, dtype=F64) * 3 + 100
    x[:, 0] = 7.0                                                  # a constant column
    gamma, beta = torch.randn(f, generator=g, dtype=F64), torch.randn(f, generator=g, dtype=F64)
    rm, rv = torch.randn(f, generator=g, dtype=F64), torch.rand(f, generator=g, dtype=F64) + 0.5
    dy = torch.randn((m, f), generator=g, dtype=F64)
    bn = torch.nn.BatchNorm1d(f, eps=1e-5, momentum=mom, track_running_stats=buffers).double()
    with torch.no_grad():
        bn.weight.copy_(gamma); bn.bias.copy_(beta)
        if buffers:
            bn.running_mean.copy_(rm); bn.running_var.copy_(rv)
    xr = x.clone().requires_grad_(True)
    y = bn.train()(xr)
    y.backward(dy)
    r = TR.bn_train(x, gamma, beta, rm if buffers else None, rv if buffers else None, mom, 1e-5, dy)
    torch.testing.assert_close(r["y"], y.detach(), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(r["dx"], xr.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(r["dgamma"], bn.weight.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(r["dbeta"], bn.bias.grad, rtol=1e-13, atol=1e-13)
    if buffers:
        torch.testing.assert_close(r["run_mean"], bn.running_mean, rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(r["run_var"], bn.running_var, rtol=1e-13, atol=1e-13)
    else:
        assert r["run_mean"] is None and r["run_var"] is None
    torch.testing.assert_close(r["mean"], x.mean(0), rtol=1e-15, atol=0)
    # the backward at given statistics: the batch's own statistics reproduce the module's gradients ...
    dx, dg, db = TR.bn_backward(dy, x, r["mean"], r["invstd"], gamma, frozen=False)
    torch.testing.assert_close(dx, xr.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dg, bn.weight.grad, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(db, bn.bias.grad, rtol=1e-13, atol=1e-13)
    # ... and frozen statistics are eval-mode BatchNorm with running_var = 1 / invstd^2 - eps
    xe = x.clone().requires_grad_(True)
    ge = gamma.clone().requires_grad_(True)
    ye = F.batch_norm(xe, r["mean"], 1.0 / r["invstd"] ** 2 - 1e-5, ge, beta, False, 0.0, 1e-5)
    ye.backward(dy)
    dx, dg, db = TR.bn_backward(dy, x, r["mean"], r["invstd"], gamma, frozen=True)
    torch.testing.assert_close(dx, xe.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(dg, ge.grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(db, dy.sum(0), rtol=1e-15, atol=0)
    # away from the exact statistics too: torch's own backward at given save_mean / save_invstd
    pm, pi = r["mean"] + 0.01, r["invstd"] * 1.01
    want = torch.ops.aten.native_batch_norm_backward(dy, x, gamma, None, None, pm, pi, True, 1e-5, [True, True, True])
    for got, w in zip(TR.bn_backward(dy, x, pm, pi, gamma, frozen=False), want):
        torch.testing.assert_close(got, w, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("q,gq,integer", [(1, 1, False), (5, 3, False), (70, 4, True), (3, 40, True)])
def test_pair_bwd_matches_autograd(q, gq, integer):
    g = gen(4)
    mk = (lambda *s: ints(s, g)) if integer else (lambda *s: torch.randn(s, generator=g, dtype=F64))
    a, b, w, bias = mk(q, 256), mk(gq, 256), mk(2, 256), mk(2)
    up = mk(q, gq, 2)
    up[0, 0, 0] = 0.0
    leaves = [t.clone().requires_grad_(True) for t in (a, b, w, bias)]
    OH.pair_logits(*leaves).backward(up)
    vals, majs = TR.pair_bwd(a, b, w, up, chunk=16)
    for got, leaf, maj in zip(vals, leaves, majs):
        if integer:
            assert torch.equal(got, leaf.grad)
        else:
            torch.testing.assert_close(got, leaf.grad, rtol=1e-12, atol=1e-12)
        assert bool((maj >= got.abs()).all())


def test_ce2_matches_closed_form_and_nan():
    g = gen(5)
    x = torch.randn((9, 2), generator=g, dtype=F64) * 30
    y = torch.tensor([0, 1, 1, 0, 0, 1, 0, 1, 1])
    w = torch.tensor([1e-3, 1e3], dtype=F64)
    loss, dl = TR.ce2(x, y, w)
    lse = torch.logsumexp(x, 1)
    wi = w[y]
    torch.testing.assert_close(loss, (wi * (lse - x[torch.arange(9), y])).sum() / wi.sum(), rtol=1e-13, atol=0)
    p = torch.softmax(x, 1)
    want = wi[:, None] / wi.sum() * (p - F.one_hot(y, 2))
    torch.testing.assert_close(dl, want, rtol=1e-12, atol=1e-15)     # want cancels like autograd at saturation
    # ... and autograd itself where it is accurate; saturated (gap 60): the non-target column is k p1 in both, the target's
    # column is -k p1 in the closed form where autograd's softmax - onehot has cancelled to 0
    xr = x.clone().requires_grad_(True)
    F.cross_entropy(xr, y, weight=w).backward()
    torch.testing.assert_close(dl, xr.grad, rtol=1e-9, atol=1e-12)
    xs = torch.tensor([[30.0, -30.0], [-30.0, 30.0]], dtype=F64)
    ys = torch.tensor([0, 1])
    _, dls = TR.ce2(xs, ys, torch.tensor([1.0, 1.0], dtype=F64))
    p_small = torch.sigmoid(torch.tensor(-60.0, dtype=F64))
    torch.testing.assert_close(dls, torch.stack([torch.stack([-p_small, p_small]), torch.stack([p_small, -p_small])]) / 2,
                               rtol=1e-15, atol=0)
    # every selected weight 0: 0 / 0 -> NaN loss and NaN gradients, as the kernel must give
    loss, dl = TR.ce2(x, torch.zeros(9, dtype=torch.int64), torch.tensor([0.0, 1.0], dtype=F64))
    assert bool(torch.isnan(loss)) and bool(torch.isnan(dl).all())


def nlb_pack(g, integer_ab=False):
    mk = lambda *s, sc=1.0: torch.randn(s, generator=g, dtype=F64) * sc  # noqa: E731
    pk = dict(w_proj_t=mk(256, 384, sc=0.06), b_proj=mk(384, sc=0.1), w_cat=mk(256, sc=0.1), w_out_t=mk(128, 256, sc=0.09),
              b_out=mk(256, sc=0.1), w_att=mk(256, sc=0.1), b_att=mk(1))
    if integer_ab:
        pk["w_proj_t"][:, :256] = ints((256, 256), g, -1, 1)
        pk["b_proj"][:256] = ints((256,), g)
        pk["w_cat"] = ints((256,), g)
    return pk


def nlb_closed_backward(x, p, dz):
    """Independent restatement of the block's backward (the derivation the kernel follows) for one sequence X [T,256]."""
    T = x.shape[0]
    g = lambda k: p["newnlb." + k]  # noqa: E731
    Wg, Wth, Wph, Ww = g("g.weight")[:, :, 0], g("theta.weight")[:, :, 0], g("phi.weight")[:, :, 0], g("W.weight")[:, :, 0]
    wc = g("concat_project.0.weight").reshape(-1)
    G = x @ Wg.t() + g("g.bias")
    a = (x @ Wth.t() + g("theta.bias")) @ wc[:128]
    b = (x @ Wph.t() + g("phi.bias")) @ wc[128:]
    s = a[:, None] + b[None, :]
    f = F.relu(s) / T
    Y = f @ G
    dY = dz @ Ww
    dS = (dY @ G.t()) * (s > 0) / T
    da, db = dS.sum(1), dS.sum(0)
    dG = f.t() @ dY
    dx = dz + da[:, None] * (Wth.t() @ wc[:128])[None] + db[:, None] * (Wph.t() @ wc[128:])[None] + dG @ Wg
    return dx, {"newnlb.g.weight": (dG.t() @ x)[:, :, None], "newnlb.W.weight": (dz.t() @ Y)[:, :, None],
                "newnlb.W.bias": dz.sum(0), "newnlb.theta.bias": wc[:128] * da.sum()}


def test_nlb_reference_matches_closed_form_backward():
    g = gen(6)
    p = TR.nlb_params(nlb_pack(g))
    for T in (1, 2, 5):
        x = torch.randn((T, 256), generator=g, dtype=F64)
        dz = torch.randn((T, 256), generator=g, dtype=F64)
        dx, grads = TR.nlb_bwd([x], p, 2, dz=[dz])
        wdx, wgr = nlb_closed_backward(x, p, dz)
        torch.testing.assert_close(dx[0], wdx, rtol=1e-11, atol=1e-11)
        for k, v in wgr.items():
            torch.testing.assert_close(grads[k], v, rtol=1e-11, atol=1e-11)
        assert float(grads["attention_scorer.weight"].abs().max()) == 0.0     # no scorer behind a block call
        mdx, mgr = TR.nlb_majorants([x], p, 2, dz=[dz])
        assert bool((mdx[0] >= dx[0].abs() * (1 - 1e-12)).all())
        assert all(bool((mgr[k] >= grads[k].abs() * (1 - 1e-12) - 1e-300).all()) for k in grads)


def test_nlb_pooled_ragged_clamped_and_layouts():
    g = gen(7)
    pk = nlb_pack(g)
    p = TR.nlb_params(pk)
    assert torch.equal(p["newnlb.W.weight"][:, :, 0].t(), pk["w_out_t"])
    S, Tmax = 5, 4
    lens = [3, 0, 1, 9, 4]                                   # 0 empty, 1 bypassed under use_nlb 1, 9 clamped to Tmax
    tm = torch.randn((Tmax, S, 256), generator=g, dtype=F64)
    bm = torch.zeros((S, Tmax, 260), dtype=F64)              # batch-major, padded row stride
    bm[:, :, :256] = tm.permute(1, 0, 2)
    a = TR.seq_rows(tm.reshape(-1), S * 256, 256, lens, S, Tmax)
    b = TR.seq_rows(bm.reshape(-1), 260, Tmax * 260, lens, S, Tmax)
    assert [r.shape[0] for r in a] == [3, 0, 1, 4, 4]
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    clamped = TR.seq_rows(tm.reshape(-1), S * 256, 256, [3, 0, 1, 4, 4], S, Tmax)
    assert all(torch.equal(u, v) for u, v in zip(a, clamped))
    dout = torch.randn((S, 256), generator=g, dtype=F64)
    live = [i for i in range(S) if a[i].shape[0] > 0]
    for use in (0, 1, 2):
        dx, grads = TR.nlb_bwd([a[i] for i in live], p, use, dout=dout[live])
        # vs autograd through the module-level helper the heads use (length-1 bypass only under use_nlb 1)
        q = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        xs = [a[i].clone().requires_grad_(True) for i in live]
        if use == 1:
            out, _ = OH.aggregate_sequences(xs, q)
        elif use == 0:
            out, _ = OH.aggregate_sequences(xs, q, use_nlb=False)
        else:
            out = torch.cat([OH.attention_pool(OH.nlb_closed_form(x, q), q)[0][None] for x in xs])
        (out * dout[live]).sum().backward()
        for u, x in zip(dx, xs):
            torch.testing.assert_close(u, x.grad, rtol=1e-12, atol=1e-12)
        for k in grads:
            want = q[k].grad if q[k].grad is not None else torch.zeros_like(q[k])
            torch.testing.assert_close(grads[k], want, rtol=1e-12, atol=1e-12)
        mdx, mgr = TR.nlb_majorants([a[i] for i in live], p, use, dout=dout[live])
        assert all(bool((m >= d.abs() * (1 - 1e-12)).all()) for m, d in zip(mdx, dx))
        assert all(bool((mgr[k] >= grads[k].abs() * (1 - 1e-12) - 1e-300).all()) for k in grads)


def test_relu_margin():
    g = gen(8)
    pk = nlb_pack(g, integer_ab=True)
    p = TR.nlb_params(pk)
    x = ints((6, 256), g)
    a, b, ma, mb = TR.nlb_ab(x, p)
    assert torch.equal(a, torch.round(a)) and torch.equal(b, torch.round(b))
    assert bool((ma >= a.abs()).all()) and bool((mb >= b.abs()).all())
    assert TR.relu_margin_hits(x, p) == 0                   # exact a, b: no pair can flip, not even a + b == 0
    # a pair a_0 + b_1 just off zero (inside the bound) is a hit; the same pair 1.0 off is not
    p2 = {k: v.clone() for k, v in p.items()}
    shift = -(a[0] + b[1]).item() + 1e-9
    p2["newnlb.theta.bias"] = p2["newnlb.theta.bias"] + shift / p["newnlb.concat_project.0.weight"].reshape(-1)[:128].sum()
    assert TR.relu_margin_hits(x, p2) >= 1
    a2, b2, ma2, mb2 = TR.nlb_ab(x, p2)
    assert abs((a2[0] + b2[1]).item()) < 1e-6
    s = a2[:, None] + b2[None, :]
    want = int(((s.abs() <= TR.bound(ma2[:, None] + mb2[None, :], TR.NLB_AB_CHAIN)) & (s != 0)).sum())
    assert TR.relu_margin_hits(x, p2) == want
    p2["newnlb.theta.bias"] = p2["newnlb.theta.bias"] + 10.0 / p["newnlb.concat_project.0.weight"].reshape(-1)[:128].sum()
    a2, b2, ma2, mb2 = TR.nlb_ab(x, p2)
    assert abs((a2[0] + b2[1]).item()) > float(TR.bound(ma2[0] + mb2[1], TR.NLB_AB_CHAIN))
    assert np.isclose(TR.bound(1.0, 10), 2 * 10 * 2.0 ** -24)
