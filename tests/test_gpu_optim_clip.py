"""GPU: gradient clipping by global norm and non-finite steps inside ``optim.SGD`` (``seam_grad_norm_f32``,
``seam_sgd_step_clip_f32``) and the stand-alone ``optim.clip_grad_norm_`` (``seam_grad_norm_f32`` + ``seam_grad_scale_f32``) against
``optim_clip_refs``.

Parameters and gradients are views into the guarded, sentinel-filled arenas of ``test_gpu_optim_sgd.py``; tensor i has
``NUMELS[i % 11]`` elements and its parameter and gradient start ``i % 4`` and ``(i // 4) % 4`` floats past a 16-byte boundary: every
size -- 1..5 (below a vector), 255..257 (one lane round), 8191..8193 (the chunk edge), 3 * 8192 + 7 (several blocks, a tail) -- at
the 16 placements of the two.  Momentum buffers are the optimizer's own (``buffers=False``: aligned, unguarded) except in
``test_buffers_in_the_guarded_arena_applied_and_skipped``, which installs arena views starting ``(i // 16) % 4`` floats past a
boundary as ``momentum_buffer``: there 66 tensors cover all 64 placements of parameter, gradient and buffer, a chunk forced onto
the 4-byte path by its buffer alone included, with guards around every buffer.

Tolerances.  The norm: the kernel adds exact fp64 squares, so its relative error before the one rounding to fp32 is below
n * 2^-53 + 2^-53 (n < 2^20 here: below 2^-32, against half an fp32 ulp of 2^-25 relative); the reference has the same error, so the
two fp32 values are roundings of numbers 2^-31 apart and differ by at most ONE ulp.  The inf norm, the coefficient, the scaled
gradients and the step are bit for bit.  ``torch.optim.SGD`` on the device may fuse ``x + alpha * y``; where it is compared bit for
bit every multiplier is a power of two, so each product is exact either way (tests/test_optim_clip_host.py)."""
import copy

import numpy as np
import pytest
import torch

import optim_clip_refs as CR
import optim_refs as R
from test_gpu_optim_sgd import CHUNK, DEV, HYPER, make, snap

pytestmark = pytest.mark.gpu

INF = float("inf")
NUMELS = [1, 3, 4, 5, 255, 256, 257, 8191, 8192, 8193, 3 * CHUNK + 7]
ALL = [NUMELS[i % 11] for i in range(66)]
SMALL = [1, 5, 257, 8193, 3, CHUNK]


def SGD(*a, **k):
    from seam_match_rcnn_amd.optim import SGD as S
    return S(*a, **k)


def clip_grad_norm_(*a, **k):
    from seam_match_rcnn_amd.optim import clip_grad_norm_ as f
    return f(*a, **k)


def bits(x):
    return np.asarray(x, np.float32).reshape(-1).view(np.uint32)


def state_bufs(opt, params):
    return [opt.state[p]["momentum_buffer"].cpu().numpy() if "momentum_buffer" in opt.state.get(p, {}) else None for p in params]


def check(params, opt, before_p, grads, before_b, first, hyper, coef):
    """every parameter and buffer bit for bit against ``sgd32`` on ``g * coef``"""
    kw = {k: hyper[k] for k in ("momentum", "dampening", "weight_decay", "nesterov", "maximize")}
    for i, p in enumerate(params):
        if grads[i] is None:
            continue
        f = first if isinstance(first, bool) else first[i]
        p32, b32 = CR.clipped_sgd32(before_p[i], grads[i], coef, before_b[i], f, hyper["lr"], **kw)
        assert R.same_bits(p.detach().cpu().numpy(), p32), f"tensor {i} ({p.numel()} elements): not the restatement's bits"
        if kw["momentum"] != 0:
            assert R.same_bits(opt.state[p]["momentum_buffer"].cpu().numpy(), b32), f"buffer {i}"


def unchanged(views, before):
    return all(R.same_bits(v.cpu().numpy(), b) for v, b in zip(views, before))


# ---- 1, 2: the norm and the coefficient ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def norm_case():
    pa, ga, _, params = make(ALL, 11, buffers=False)
    grads = snap(ga.views)
    return pa, ga, params, grads, {t: CR.total_norm64(grads, t) for t in (2.0, INF)}


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_total_norm_against_float64_and_twice_the_same_bits(norm_case, norm_type):
    pa, ga, params, grads, want = norm_case
    got = [float(clip_grad_norm_(params, 1e30, norm_type=norm_type)) for _ in range(2)]     # coefficient 1: the gradients stay
    print("norm", norm_type, "device", got[0], "float64", want[norm_type])
    assert CR.within_ulp32(got[0], want[norm_type]) and bits(got[0]) == bits(got[1])
    if norm_type == INF:
        assert got[0] == want[norm_type]
    assert unchanged(ga.views, grads) and ga.guards_intact() and pa.guards_intact()


@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_clip_coefficient_above_below_and_at_max_norm(norm_case, norm_type):
    pa, ga, params, grads, want = norm_case
    seen = None
    for case in ("above", "below", "equal"):
        # the norm against max_norm; "equal" takes the device's own total, so max_norm / (total + 1e-6) is just below 1
        max_norm = float(np.float32(want[norm_type])) / 7.0 if case == "above" else seen * 3.0 if case == "below" else seen
        own = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for q, p in zip(own, params):
            q.grad = p.grad
        opt = SGD(own, lr=0.0, max_norm=max_norm, norm_type=norm_type)
        opt.step()
        got_total, got_coef = float(opt.total_norm), np.float32(float(opt.clip_coef))
        print(case, "max_norm", max_norm, "total", got_total, "coef", got_coef)
        assert CR.within_ulp32(got_total, want[norm_type]) and (seen is None or got_total == seen)
        seen = got_total
        assert bits(got_coef) == bits(CR.coef32(got_total, max_norm)) == bits(CR.coef32_np(got_total, max_norm))
        assert got_coef < 1.0 if case == "above" else got_coef == 1.0 if case == "below" else got_coef <= 1.0
    assert unchanged(ga.views, grads) and opt.skipped_steps() == 0


# ---- 3: the fused step -----------------------------------------------------------------------------------------------------------
def test_sizes_alignments_guards_two_groups_and_a_missing_gradient():
    pa, ga, _, params = make(ALL, 12, buffers=False)
    h0 = dict(HYPER, lr=0.05, momentum=0.9, weight_decay=0.0)
    h1 = dict(HYPER, lr=0.003, momentum=0.5, weight_decay=1e-2, dampening=0.1)
    cut, mid = 40, 9
    params[mid].grad = None
    before_mid = params[mid].detach().clone()
    opt = SGD([dict(params=params[:cut]), dict(params=params[cut:], lr=h1["lr"], momentum=h1["momentum"], weight_decay=h1["weight_decay"],
                                               dampening=h1["dampening"])],
              lr=h0["lr"], momentum=h0["momentum"], weight_decay=h0["weight_decay"], max_norm=2.5)
    for step in range(2):
        bp, bg, bb = snap(pa.views), snap(ga.views), state_bufs(opt, params)
        bg[mid] = None
        opt.step()
        torch.cuda.synchronize()
        total, coef = float(opt.total_norm), float(opt.clip_coef)
        assert CR.within_ulp32(total, CR.total_norm64(bg, 2.0)) and bits(coef) == bits(CR.coef32(total, 2.5)) and coef < 1.0
        check(params[:cut], opt, bp[:cut], bg[:cut], bb[:cut], step == 0, h0, coef)
        check(params[cut:], opt, bp[cut:], bg[cut:], bb[cut:], step == 0, h1, coef)
        assert all(R.same_bits(g.cpu().numpy(), b) for i, (g, b) in enumerate(zip(ga.views, bg)) if i != mid), ".grad was modified"
    assert pa.guards_intact() and ga.guards_intact()
    assert torch.equal(params[mid].detach(), before_mid) and "momentum_buffer" not in opt.state.get(params[mid], {})
    # the gradient arrives later: that tensor's buffer is new while the others' exist
    bp, bb = snap(pa.views), state_bufs(opt, params)
    params[mid].grad = ga.views[mid]
    bg = snap(ga.views)
    opt.step()
    torch.cuda.synchronize()
    coef = float(opt.clip_coef)
    first = [i == mid for i in range(len(params))]
    check(params[:cut], opt, bp[:cut], bg[:cut], bb[:cut], first[:cut], h0, coef)
    check(params[cut:], opt, bp[cut:], bg[cut:], bb[cut:], first[cut:], h1, coef)
    assert pa.guards_intact() and opt.skipped_steps() == 0


@pytest.mark.parametrize("norm_type", [2.0, INF])
@pytest.mark.parametrize("momentum,dampening,weight_decay,nesterov,maximize", R.OPTIONS)
def test_every_option_first_and_second_step(momentum, dampening, weight_decay, nesterov, maximize, norm_type):
    hyper = dict(lr=0.02, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
    pa, ga, _, params = make(SMALL, 13, buffers=False)
    opt = SGD(params, max_norm=1.5, norm_type=norm_type, **hyper)
    for step in range(2):
        bp, bg, bb = snap(pa.views), snap(ga.views), state_bufs(opt, params)
        opt.step()
        torch.cuda.synchronize()
        total, coef = float(opt.total_norm), float(opt.clip_coef)
        assert CR.within_ulp32(total, CR.total_norm64(bg, norm_type)) and bits(coef) == bits(CR.coef32(total, 1.5)) and coef < 1.0
        check(params, opt, bp, bg, bb, step == 0, hyper, coef)
        assert unchanged(ga.views, bg)
        if not momentum:
            assert all("momentum_buffer" not in opt.state.get(p, {}) for p in params)
    assert pa.guards_intact() and ga.guards_intact()


def test_buffers_in_the_guarded_arena_applied_and_skipped():
    pa, ga, ba, params = make(ALL, 21)                           # buffers from the arena too: p, g and buf placed independently
    hyper = dict(HYPER, dampening=0.1)
    opt = SGD(params, max_norm=2.5, skip_nonfinite=True, **hyper)
    for p, b in zip(params, ba.views):
        opt.state[p]["momentum_buffer"] = b

    def intact():
        return pa.guards_intact() and ga.guards_intact() and ba.guards_intact()
    bp, bg, bb = snap(pa.views), snap(ga.views), snap(ba.views)
    opt.step()                                                   # applied: the buffers are read and written where they lie
    torch.cuda.synchronize()
    coef = float(opt.clip_coef)
    assert coef < 1.0 and opt.skipped_steps() == 0
    check(params, opt, bp, bg, bb, False, hyper, coef)
    assert intact() and unchanged(ga.views, bg)
    assert all(opt.state[p]["momentum_buffer"].data_ptr() == b.data_ptr() for p, b in zip(params, ba.views))
    for bad in (INF, float("nan")):                              # skipped: no parameter byte, no buffer byte, no guard
        clean = float(ga.views[37][2])
        ga.views[37][2] = bad
        bp, bb = snap(pa.views), snap(ba.views)
        n = opt.skipped_steps()
        opt.step()
        torch.cuda.synchronize()
        assert opt.skipped_steps() == n + 1 and not np.isfinite(float(opt.total_norm))
        assert unchanged(pa.views, bp), "a skipped step wrote a parameter"
        assert unchanged(ba.views, bb), "a skipped step wrote a momentum buffer"
        assert intact()
        ga.views[37][2] = clean
    bg = snap(ga.views)
    opt.step()                                                   # applied again: an ordinary step on the buffers of before
    torch.cuda.synchronize()
    check(params, opt, bp, bg, bb, False, hyper, float(opt.clip_coef))
    assert intact() and opt.skipped_steps() == 2


# ---- 4: coefficient 1 is the unclipped step ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip", [False, True])
def test_a_coefficient_of_one_gives_the_unclipped_bits(skip):
    out = []
    for kw in (dict(), dict(max_norm=None if skip else 1e30, skip_nonfinite=skip)):
        pa, ga, _, params = make(ALL, 14, buffers=False)
        opt = SGD(params, **HYPER, **kw)
        assert opt.clipping == bool(kw)
        for _ in range(2):
            opt.step()
        out.append((snap(pa.views), state_bufs(opt, params), pa.guards_intact()))
        if kw:
            assert float(opt.clip_coef) == 1.0 and opt.skipped_steps() == 0
    (p0, b0, g0), (p1, b1, g1) = out
    assert g0 and g1 and all(R.same_bits(a, b) for a, b in zip(p0, p1)) and all(R.same_bits(a, b) for a, b in zip(b0, b1))


# ---- 5: non-finite steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [INF, float("nan")], ids=["inf", "nan"])
@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_a_non_finite_step_is_skipped_and_the_next_one_is_a_first_step(bad, norm_type):
    hyper = dict(HYPER, dampening=0.5)
    pa, ga, _, params = make(ALL, 15, buffers=False)
    clean = snap(ga.views)
    ga.views[37][2] = bad
    opt = SGD(params, max_norm=1.5, norm_type=norm_type, skip_nonfinite=True, **hyper)
    bp = snap(pa.views)
    opt.step()
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and not np.isfinite(float(opt.total_norm))
    assert unchanged(pa.views, bp) and pa.guards_intact(), "a skipped step wrote a parameter"
    # the buffers the host created on the dropped step are zeros, not uninitialised memory (a state_dict() may be taken now)
    assert all(not bool(opt.state[p]["momentum_buffer"].any()) for p in params)
    # the next step, finite: a first step (buf = g') although the host created the buffers a step ago
    ga.views[37][2] = float(clean[37][2])
    bg = snap(ga.views)
    opt.step()
    torch.cuda.synchronize()
    coef = float(opt.clip_coef)
    assert opt.skipped_steps() == 1 and np.isfinite(float(opt.total_norm)) and coef < 1.0
    check(params, opt, bp, bg, [None] * len(params), True, hyper, coef)
    fresh_pa, fresh_ga, _, fresh = make(ALL, 15, buffers=False)
    fopt = SGD(fresh, max_norm=1.5, norm_type=norm_type, skip_nonfinite=True, **hyper)
    fopt.step()
    assert all(torch.equal(a, b) for a, b in zip(pa.views, fresh_pa.views)), "not the first step of a fresh optimizer"
    assert all(torch.equal(opt.state[p]["momentum_buffer"], fopt.state[q]["momentum_buffer"]) for p, q in zip(params, fresh))
    # and the one after it reads the buffers like any second step
    bp, bb = snap(pa.views), state_bufs(opt, params)
    opt.step()
    torch.cuda.synchronize()
    check(params, opt, bp, bg, bb, False, hyper, float(opt.clip_coef))
    assert pa.guards_intact() and ga.guards_intact() and opt.skipped_steps() == 1


def test_a_skipped_step_leaves_existing_buffers_and_marks_only_the_new_ones():
    h0, h1 = dict(HYPER, dampening=0.5), dict(HYPER, lr=0.003, momentum=0.5, dampening=0.1)
    pa, ga, _, params = make(SMALL + SMALL, 16, buffers=False)
    cut = len(SMALL)
    opt = SGD([dict(params=params[:cut], dampening=0.5), dict(params=params[cut:], lr=0.003, momentum=0.5, dampening=0.1)],
              lr=HYPER["lr"], momentum=0.9, weight_decay=HYPER["weight_decay"], max_norm=1.5, skip_nonfinite=True)
    held = [p.grad for p in params[cut:]]
    for p in params[cut:]:
        p.grad = None
    opt.step()                                                   # group 0 alone: its buffers exist from here on
    for p, g in zip(params[cut:], held):
        p.grad = g
    clean = float(ga.views[2][1])
    ga.views[2][1] = INF
    bp, bb = snap(pa.views), state_bufs(opt, params)
    opt.step()                                                   # skipped: group 1's buffers are created and stay unwritten
    torch.cuda.synchronize()
    assert opt.skipped_steps() == 1 and unchanged(pa.views, bp)
    assert unchanged([opt.state[p]["momentum_buffer"] for p in params[:cut]], bb[:cut]), "a skipped step wrote a momentum buffer"
    ga.views[2][1] = clean
    bg = snap(ga.views)
    opt.step()
    torch.cuda.synchronize()
    coef = float(opt.clip_coef)
    check(params[:cut], opt, bp[:cut], bg[:cut], bb[:cut], False, h0, coef)
    check(params[cut:], opt, bp[cut:], bg[cut:], [None] * cut, True, h1, coef)
    assert pa.guards_intact() and opt.skipped_steps() == 1


@pytest.mark.parametrize("bad", [INF, float("nan")], ids=["inf", "nan"])
def test_without_skip_nonfinite_the_step_is_torchs_after_clip_grad_norm(bad):
    pa, ga, _, params = make(SMALL, 17, buffers=False)
    ga.views[3][5] = bad
    opt = SGD(params, max_norm=1.5, **HYPER)
    bp, bg = snap(pa.views), snap(ga.views)
    opt.step()
    torch.cuda.synchronize()
    coef = float(opt.clip_coef)
    assert (coef == 0.0) if bad == INF else np.isnan(coef)
    assert bits(coef) == bits(CR.coef32(float(opt.total_norm), 1.5)) or np.isnan(coef)
    check(params, opt, bp, bg, [None] * len(params), True, HYPER, coef)
    assert opt.skipped_steps() == 1 and pa.guards_intact()       # counted, not dropped


# ---- 6: the stand-alone function -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type", [2.0, INF])
def test_clip_grad_norm_scales_the_gradients_in_place(norm_type):
    pa, ga, _, params = make(ALL, 18, buffers=False)
    params[5].grad = None
    bp, raw = snap(pa.views), snap(ga.views)
    bg = [None if i == 5 else g for i, g in enumerate(raw)]
    total = clip_grad_norm_(params, 2.5, norm_type=norm_type)
    assert total.dim() == 0 and total.dtype == torch.float32 and total.is_cuda
    got = float(total)
    assert CR.within_ulp32(got, CR.total_norm64(bg, norm_type))
    coef = CR.coef32(got, 2.5)
    assert coef < 1.0
    for i, (g, b) in enumerate(zip(ga.views, bg)):
        assert R.same_bits(g.cpu().numpy(), CR.scaled32(b, coef) if b is not None else raw[i]), f"gradient {i}"
    assert ga.guards_intact() and pa.guards_intact() and unchanged(pa.views, bp)
    # a following torch.optim.SGD.step() and a following optim.SGD.step() agree (power-of-two multipliers: see the docstring)
    params[5].grad = ga.views[5]
    hyper = dict(lr=2.0 ** -6, momentum=0.5, dampening=0.5, weight_decay=2.0 ** -13)
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for c, p in zip(clones, params):
        c.grad = p.grad.clone()
    ref, opt = torch.optim.SGD(clones, **hyper), SGD(params, **hyper)
    for _ in range(2):
        ref.step()
        opt.step()
    assert all(torch.equal(c.detach(), p.detach()) for c, p in zip(clones, params))
    assert all(torch.equal(ref.state[c]["momentum_buffer"], opt.state[p]["momentum_buffer"]) for c, p in zip(clones, params))
    assert pa.guards_intact()


def test_clip_grad_norm_refusals_and_edge_cases():
    from seam_match_rcnn_amd import _native
    pa, ga, _, params = make(SMALL, 19, buffers=False)
    bg = snap(ga.views)
    ga.views[1][0] = INF
    with pytest.raises(RuntimeError, match="non-finite"):
        clip_grad_norm_(params, 1.0, error_if_nonfinite=True)
    assert float(ga.views[1][1]) == float(bg[1][1]), "nothing is scaled before the error"
    assert float(clip_grad_norm_(params, 1.0)) == INF             # torch's behaviour: coefficient 0
    assert float(ga.views[0][0]) == 0.0 and np.isnan(float(ga.views[1][0]))
    ok = torch.nn.Parameter(torch.ones(4, device=DEV))
    ok.grad = torch.ones(4, device=DEV)
    half = torch.nn.Parameter(torch.ones(4, device=DEV, dtype=torch.float16))
    half.grad = torch.ones(4, device=DEV, dtype=torch.float16)
    with pytest.raises(TypeError, match="parameter 1 .*float16"):
        clip_grad_norm_([ok, half], 1.0)
    cpu = torch.nn.Parameter(torch.ones(4))
    cpu.grad = torch.ones(4)
    with pytest.raises(_native.SeamNativeError, match="parameter 1 .*not on the HIP device"):
        clip_grad_norm_([ok, cpu], 1.0)
    nc = torch.nn.Parameter(torch.ones(3, 4, device=DEV))
    nc.grad = torch.ones(4, 3, device=DEV).t()
    with pytest.raises(ValueError, match="parameter 2 .*not contiguous"):
        clip_grad_norm_([ok, ok, nc], 1.0)
    with pytest.raises(ValueError, match="3.0"):
        clip_grad_norm_([ok], 1.0, norm_type=3.0)
    assert torch.equal(ok.grad, torch.ones(4, device=DEV)), "a refused call scaled a gradient"
    assert float(clip_grad_norm_([], 1.0)) == 0.0 and float(clip_grad_norm_([torch.nn.Parameter(torch.ones(2, device=DEV))], 1.0)) == 0.0
    assert float(clip_grad_norm_(ok, 1.0, foreach=True)) == 2.0 and torch.equal(ok.grad, torch.full((4,), float(CR.coef32(2.0, 1.0)), device=DEV))


# ---- 7: schedulers and checkpoints ---------------------------------------------------------------------------------------------------
def test_a_scheduler_between_clipped_steps_uploads_no_table_and_state_dict_round_trips():
    pa, ga, _, params = make([257, 4099, 2 * CHUNK + 1], 20, buffers=False)
    opt = SGD(params, max_norm=1.5, skip_nonfinite=True, **HYPER)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda e: (0.25, 0.5, 1.0, 1.0)[e])
    for step in range(3):
        lr = opt.param_groups[0]["lr"]
        bp, bg, bb = snap(pa.views), snap(ga.views), state_bufs(opt, params)
        opt.step()
        sched.step()
        torch.cuda.synchronize()
        check(params, opt, bp, bg, bb, step == 0, dict(HYPER, lr=lr), float(opt.clip_coef))
        assert opt.table_uploads == 1, "a changed lr must not rebuild or upload the tables"
    sd = opt.state_dict()
    # the clipping settings belong to the instance: the groups hold torch.optim.SGD's keys (and the scheduler's initial_lr) only
    assert set(sd["param_groups"][0]) - {"initial_lr"} == set(torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1).state_dict()["param_groups"][0])
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    ref = torch.optim.SGD(clones, lr=1.0)
    ref.load_state_dict(copy.deepcopy(sd))
    assert ref.param_groups[0]["momentum"] == 0.9 and all(torch.equal(ref.state[c]["momentum_buffer"], opt.state[p]["momentum_buffer"])
                                                          for c, p in zip(clones, params))
    back = SGD([torch.nn.Parameter(c.detach().clone()) for c in clones], lr=1.0, max_norm=1.5, skip_nonfinite=True)
    back.load_state_dict(copy.deepcopy(ref.state_dict()))
    mine = back.param_groups[0]["params"]
    for m, p in zip(mine, params):
        m.grad = p.grad.clone()
    bp, bg, bb = snap(mine), snap(ga.views), state_bufs(back, mine)
    back.step()
    torch.cuda.synchronize()
    check(mine, back, bp, bg, bb, False, dict(HYPER, lr=back.param_groups[0]["lr"]), float(back.clip_coef))
