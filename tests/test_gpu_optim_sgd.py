"""GPU: ``seam_sgd_step_f32`` through ``optim.SGD(model=None)`` against ``optim_refs.sgd32`` bit for bit (NaN equal to NaN) and against
``optim_refs.sgd64`` within ``optim_refs.bound``.

Parameters, gradients and momentum buffers are views into ONE padded buffer filled with a sentinel, each start a chosen number of
floats past a 16-byte boundary, so the guard floats on both sides of every tensor can be checked untouched (the 16-byte path, the
4-byte path and the tail of a vector chunk all end somewhere inside that buffer)."""
import copy

import numpy as np
import pytest
import torch

import optim_refs as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SENTINEL = 12345.678
GUARD = 8
CHUNK = 8192
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 4099, 3 * CHUNK + 77]


def SGD(*a, **k):
    from seam_match_rcnn_amd.optim import SGD as S
    return S(*a, **k)


class Arena:
    """views of ``numel`` floats starting ``off`` floats past a 16-byte boundary, GUARD sentinel floats around each"""

    def __init__(self, specs, seed, scale=1.0):
        starts, pos = [], 0
        for n, off in specs:
            pos = (pos + GUARD + 3) // 4 * 4 + off
            starts.append(pos)
            pos += n
        self.buf = torch.full((pos + GUARD + 4,), SENTINEL, dtype=torch.float32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        g = torch.Generator().manual_seed(seed)
        self.views, self.mask = [], torch.ones(self.buf.numel(), dtype=torch.bool)
        for (n, off), s in zip(specs, starts):
            v = self.buf[s:s + n]
            assert n == 0 or (v.data_ptr() // 4) % 4 == off
            v.copy_((torch.randn(n, generator=g) * scale * torch.logspace(-2, 2, max(n, 1))[:n]).to(DEV))
            self.views.append(v)
            self.mask[s:s + n] = False
        self.mask = self.mask.to(DEV)

    def guards_intact(self) -> bool:
        return bool((self.buf[self.mask] == SENTINEL).all())


def offsets(i):
    """parameter, gradient and buffer misalignments of tensor i, varied independently (all 64 combinations over 64 tensors)"""
    return i % 4, (i // 4) % 4, (i // 16) % 4


def make(numels, seed, buffers=True):
    pa = Arena([(n, offsets(i)[0]) for i, n in enumerate(numels)], seed)
    ga = Arena([(n, offsets(i)[1]) for i, n in enumerate(numels)], seed + 1)
    ba = Arena([(n, offsets(i)[2]) for i, n in enumerate(numels)], seed + 2) if buffers else None
    params = [torch.nn.Parameter(v) for v in pa.views]
    for p, v, g in zip(params, pa.views, ga.views):
        assert p.data_ptr() == v.data_ptr()
        p.grad = g
    return pa, ga, ba, params


def snap(ts):
    return [None if t is None else t.detach().cpu().numpy().copy() for t in ts]


def check(params, opt, before_p, grads, before_b, first, hyper):
    """every parameter (and buffer) against the restatement bit for bit and against float64 within the bound"""
    kw = {k: hyper[k] for k in ("momentum", "dampening", "weight_decay", "nesterov", "maximize")}
    for i, p in enumerate(params):
        if grads[i] is None or p.numel() == 0:
            continue
        f = first if isinstance(first, bool) else first[i]
        p32, b32 = R.sgd32(before_p[i], grads[i], before_b[i], f, hyper["lr"], **kw)
        p64, _ = R.sgd64(before_p[i], grads[i], before_b[i], f, hyper["lr"], **kw)
        got = p.detach().cpu().numpy()
        assert R.same_bits(got, p32), f"tensor {i} ({p.numel()} elements): not the restatement's bits"
        assert R.within(got, p64, R.bound(before_p[i], grads[i], before_b[i], hyper["lr"], kw["momentum"], kw["weight_decay"])), i
        if kw["momentum"] != 0:
            assert R.same_bits(opt.state[p]["momentum_buffer"].cpu().numpy(), b32), f"buffer {i}"


HYPER = dict(lr=0.02, momentum=0.9, dampening=0.0, weight_decay=1e-4, nesterov=False, maximize=False)


def test_sizes_alignments_and_guards_with_existing_buffers():
    numels = SIZES + [5] * 64 + [257] * 64 + [4099] * 16 + [CHUNK + 3] * 4 + [2 * CHUNK]
    pa, ga, ba, params = make(numels, 1)
    opt = SGD(params, **HYPER)
    for p, b in zip(params, ba.views):
        if p.numel():
            opt.state[p]["momentum_buffer"] = b
    bp, bg, bb = snap(pa.views), snap(ga.views), snap(ba.views)
    opt.step()
    torch.cuda.synchronize()
    check(params, opt, bp, bg, bb, False, HYPER)
    assert pa.guards_intact() and ga.guards_intact() and ba.guards_intact()
    assert all(torch.equal(g, torch.from_numpy(b).to(DEV)) for g, b in zip(ga.views, bg))          # gradients are only read
    assert "momentum_buffer" not in opt.state.get(params[0], {})                                      # the 0-element tensor
    assert all(opt.state[p]["momentum_buffer"].data_ptr() == b.data_ptr() for p, b in zip(params, ba.views) if p.numel())


def test_first_step_creates_buffers_and_skips_a_missing_gradient():
    numels = SIZES + [5] * 16 + [4099] * 4
    pa, ga, _, params = make(numels, 2, buffers=False)
    mid = len(SIZES) + 3
    params[mid].grad = None
    before_mid = params[mid].detach().clone()
    opt = SGD(params, **HYPER)
    bp, bg = snap(pa.views), snap(ga.views)
    bg[mid] = None
    opt.step()
    torch.cuda.synchronize()
    check(params, opt, bp, bg, [None] * len(params), True, HYPER)
    assert pa.guards_intact() and ga.guards_intact()
    assert torch.equal(params[mid].detach(), before_mid) and "momentum_buffer" not in opt.state.get(params[mid], {})
    assert params[0].numel() == 0 and "momentum_buffer" not in opt.state.get(params[0], {})
    # the gradient arrives later: that tensor's buffer is new while the others' exist (one group, two kernel slots)
    bp, bb = snap(pa.views), [None if p.numel() == 0 or i == mid else opt.state[p]["momentum_buffer"].cpu().numpy() for i, p in enumerate(params)]
    params[mid].grad = ga.views[mid]
    bg = snap(ga.views)
    opt.step()
    torch.cuda.synchronize()
    check(params, opt, bp, bg, bb, [i == mid for i in range(len(params))], HYPER)
    assert pa.guards_intact()


@pytest.mark.parametrize("momentum,dampening,weight_decay,nesterov,maximize", R.OPTIONS)
def test_every_option_first_and_second_step(momentum, dampening, weight_decay, nesterov, maximize):
    hyper = dict(lr=0.02, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
    pa, ga, _, params = make([1, 5, 257, 1023, 4099, CHUNK + 3], 3, buffers=False)
    opt = SGD(params, **hyper)
    for step in range(2):
        bp, bg = snap(pa.views), snap(ga.views)
        bb = [opt.state[p]["momentum_buffer"].cpu().numpy() if momentum and step else None for p in params]
        opt.step()
        torch.cuda.synchronize()
        check(params, opt, bp, bg, bb, step == 0, hyper)
        if not momentum:
            assert all("momentum_buffer" not in opt.state.get(p, {}) for p in params)
    assert pa.guards_intact() and ga.guards_intact()


def test_two_groups_with_their_own_hyper_parameters():
    pa, ga, _, params = make([257, 4099, 5, 1023, CHUNK + 3, 3], 4, buffers=False)
    h0 = dict(HYPER, lr=0.05, momentum=0.9, weight_decay=0.0)
    h1 = dict(HYPER, lr=0.003, momentum=0.5, weight_decay=1e-2)
    opt = SGD([dict(params=params[:3]), dict(params=params[3:], lr=h1["lr"], momentum=h1["momentum"], weight_decay=h1["weight_decay"])],
              lr=h0["lr"], momentum=h0["momentum"], weight_decay=h0["weight_decay"])
    for step in range(2):
        bp, bg = snap(pa.views), snap(ga.views)
        bb = [opt.state[p]["momentum_buffer"].cpu().numpy() if step else None for p in params]
        opt.step()
        torch.cuda.synchronize()
        check(params[:3], opt, bp[:3], bg[:3], bb[:3], step == 0, h0)
        check(params[3:], opt, bp[3:], bg[3:], bb[3:], step == 0, h1)
    assert pa.guards_intact() and ga.guards_intact()


def test_inf_and_nan_gradients():
    pa, ga, _, params = make([257, 4099, 6], 5, buffers=False)
    for g in ga.views:
        g[0], g[1], g[-1] = float("inf"), float("-inf"), float("nan")
    ga.views[1][1000:1003] = torch.tensor([float("nan"), float("inf"), -0.0], device=DEV)
    opt = SGD(params, **HYPER)
    for step in range(2):
        bp, bg = snap(pa.views), snap(ga.views)
        bb = [opt.state[p]["momentum_buffer"].cpu().numpy() if step else None for p in params]
        opt.step()
        torch.cuda.synchronize()
        check(params, opt, bp, bg, bb, step == 0, HYPER)
    assert not bool(torch.isfinite(params[0][:2]).any()) and bool(torch.isfinite(params[0][2:-1]).all())
    assert pa.guards_intact() and ga.guards_intact()


def test_a_scheduler_changes_lr_without_a_table_upload():
    pa, ga, _, params = make([257, 4099, 2 * CHUNK + 1], 6, buffers=False)
    opt = SGD(params, **HYPER)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: (0.25, 0.5, 1.0, 1.0)[e])
    lrs = []
    for step in range(3):
        lr = opt.param_groups[0]["lr"]
        lrs.append(lr)
        bp, bg = snap(pa.views), snap(ga.views)
        bb = [opt.state[p]["momentum_buffer"].cpu().numpy() if step else None for p in params]
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        check(params, opt, bp, bg, bb, step == 0, dict(HYPER, lr=lr))
        assert opt.table_uploads == 1, "a changed lr must not rebuild or upload the tables"
    assert lrs == [0.02 * 0.25, 0.02 * 0.5, 0.02]
    opt.zero_grad(set_to_none=False)
    opt.step()
    assert opt.table_uploads == 1
    params[1].grad = params[1].grad.clone()              # one pointer moved: the small table is uploaded again
    opt.step()
    assert opt.table_uploads == 2
    opt.add_param_group(dict(params=[torch.nn.Parameter(torch.ones(7, device=DEV))]))
    opt.param_groups[1]["params"][0].grad = torch.ones(7, device=DEV)
    opt.step()
    want, _ = R.sgd32(np.ones(7, np.float32), np.ones(7, np.float32), None, True, **HYPER)
    assert opt.table_uploads == 3 and R.same_bits(opt.param_groups[1]["params"][0].detach().cpu().numpy(), want)


def test_multistep_lr_schedule():
    pa, ga, _, params = make([257, CHUNK + 3], 8, buffers=False)
    opt = SGD(params, **HYPER)
    sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1, 2], gamma=0.1)
    seen = []
    for step in range(3):
        lr = opt.param_groups[0]["lr"]
        seen.append(lr)
        bp, bg = snap(pa.views), snap(ga.views)
        bb = [opt.state[p]["momentum_buffer"].cpu().numpy() if step else None for p in params]
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        check(params, opt, bp, bg, bb, step == 0, dict(HYPER, lr=lr))
    assert seen[0] == 0.02 and abs(seen[1] - 0.002) < 1e-12 and abs(seen[2] - 0.0002) < 1e-12 and opt.table_uploads == 1


def test_state_dict_round_trip_with_torch_sgd():
    pa, ga, _, params = make([257, 4099, 5], 7, buffers=False)
    opt = SGD(params, **HYPER)
    opt.step()
    opt.step()
    # ours -> torch.optim.SGD over clones
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.SGD(clones, lr=1.0)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))       # as through a checkpoint file: load_state_dict itself keeps tensors that fit
    assert ref.param_groups[0]["lr"] == HYPER["lr"] and ref.param_groups[0]["momentum"] == 0.9
    bp, bg = snap(pa.views), snap(ga.views)
    bb = [opt.state[p]["momentum_buffer"].cpu().numpy() for p in params]
    for c, p in zip(clones, params):
        c.grad = p.grad.clone()
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    kw = {k: HYPER[k] for k in ("momentum", "dampening", "weight_decay", "nesterov", "maximize")}
    for i, (c, p) in enumerate(zip(clones, params)):
        p64, _ = R.sgd64(bp[i], bg[i], bb[i], False, HYPER["lr"], **kw)
        tol = R.bound(bp[i], bg[i], bb[i], HYPER["lr"], 0.9, 1e-4)
        assert R.within(c.detach().cpu().numpy(), p64, tol) and R.within(p.detach().cpu().numpy(), p64, tol)
    # torch -> ours
    back = SGD([torch.nn.Parameter(c.detach().clone()) for c in clones], lr=1.0)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert back.param_groups[0]["lr"] == HYPER["lr"] and set(back.state_dict()["state"][0]) == {"momentum_buffer"}
    mine = back.param_groups[0]["params"]
    bp2 = snap(mine)
    bb2 = [ref.state[c]["momentum_buffer"].cpu().numpy() for c in clones]
    for m, c in zip(mine, clones):
        m.grad = c.grad.clone()
    ref.step()
    back.step()
    torch.cuda.synchronize()
    for i, (m, c) in enumerate(zip(mine, clones)):
        p32, b32 = R.sgd32(bp2[i], bg[i], bb2[i], False, HYPER["lr"], **kw)
        p64, _ = R.sgd64(bp2[i], bg[i], bb2[i], False, HYPER["lr"], **kw)
        tol = R.bound(bp2[i], bg[i], bb2[i], HYPER["lr"], 0.9, 1e-4)
        assert R.same_bits(m.detach().cpu().numpy(), p32)
        assert R.within(m.detach().cpu().numpy(), p64, tol) and R.within(c.detach().cpu().numpy(), p64, tol)


def test_closure_zero_grad_and_a_non_contiguous_gradient():
    p = torch.nn.Parameter(torch.arange(12, dtype=torch.float32, device=DEV).reshape(3, 4).clone())
    opt = SGD([p], lr=0.5)
    calls = []

    def closure():
        opt.zero_grad()
        loss = (p * p).sum()
        loss.backward()
        calls.append(torch.is_grad_enabled())
        return loss
    before = p.detach().clone()
    loss = opt.step(closure)
    assert calls == [True] and float(loss.detach()) == float((before * before).sum()) and torch.equal(p.detach(), before - 0.5 * (2 * before))
    v0 = p._version
    p.grad = torch.ones(4, 3, device=DEV).t()                      # a transposed view: made contiguous for this step
    assert not p.grad.is_contiguous()
    opt.step()
    assert torch.equal(p.detach(), before - 0.5 * (2 * before) - 0.5) and p._version == v0 + 1
    opt.zero_grad()
    assert p.grad is None
    opt.step()                                                     # nothing has a gradient: nothing happens
    assert p._version == v0 + 1


def test_refused_inputs_name_the_parameter():
    from seam_match_rcnn_amd.optim import MAX_GROUPS
    lin = torch.nn.Linear(4, 3).to(DEV)
    with pytest.raises(TypeError, match="float16"):
        SGD([torch.nn.Parameter(torch.zeros(3, device=DEV, dtype=torch.float16))], lr=0.1)
    with pytest.raises(ValueError, match="not contiguous"):
        SGD([torch.nn.Parameter(torch.zeros(3, 4, device=DEV).t())], lr=0.1)
    opt = SGD(lin.parameters(), lr=0.1)
    lin.weight.grad = torch.zeros(3, 4, device=DEV).to_sparse()
    with pytest.raises(TypeError, match="parameter 0 of group 0.*sparse"):
        opt.step()
    lin.weight.grad = None
    with pytest.raises(ValueError, match=f"at most {MAX_GROUPS}"):
        SGD([dict(params=[torch.nn.Parameter(torch.zeros(1, device=DEV))]) for _ in range(MAX_GROUPS + 1)], lr=0.1)
