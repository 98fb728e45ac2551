"""CPU: the yardsticks of the clipping tests.  ``optim_clip_refs`` against ``torch.nn.utils.clip_grad_norm_`` followed by
``torch.optim.SGD`` on the CPU: the float64 norm within one fp32 ulp of torch's, ``coef32`` and its NumPy restatement equal to
torch's coefficient bit for bit, and -- given torch's own coefficient -- the parameters after the step bit-identical to
``clipped_sgd32``.  Also here: the new C entries are declared in the header and bound with the same number of arguments, and what
the Python layer refuses without a GPU."""
import re
import os

import numpy as np
import pytest
import torch

import optim_clip_refs as CR
import optim_refs as R

INF = float("inf")
NUMELS = (4099, 257, 5)
# torch's CPU kernels may fuse ``x + alpha * y`` into one rounding (tests/test_optim_refs_host.py holds them to a bound for that
# reason).  With every multiplier a power of two each product is exact, fused or not, so torch and the restatement, one rounding per
# operation, must then agree BIT FOR BIT: that is the grid below.  (momentum, dampening, weight_decay, nesterov, maximize)
LR = 2.0 ** -6
OPTIONS = [(m, d, wd, nes, mx)
           for m in (0.0, 0.5) for d in (0.0, 0.5) for wd in (0.0, 2.0 ** -13) for nes in (False, True) for mx in (False, True)
           if not (nes and (m == 0.0 or d != 0.0))]


def _state(seed, scale=1.0, dyadic=False):
    """parameters and gradients.  ``dyadic``: tensor i's gradient is +-2^e_i on its first 4^m_i elements and 0 elsewhere, so every
    fp32 partial sum of squares is exact in any order, each per-tensor norm 2^(m_i + e_i) is exact, and torch's fp32 total (the norm
    of the stacked per-tensor norms) is the correctly rounded square root of an exact sum: torch's own summation error, which on
    random data of these sizes is several ulps, is zero, and 1 ulp is what two roundings of the same number can differ by."""
    g = torch.Generator().manual_seed(seed)
    ps = [torch.randn(n, generator=g) * torch.logspace(-3, 2, n) for n in NUMELS]
    gs = [torch.randn(n, generator=g) * torch.logspace(2, -3, n) * scale for n in NUMELS]
    if dyadic:
        for i, x in enumerate(gs):
            k = 4 ** int(np.log(x.numel()) / np.log(4))
            x[:k] = torch.sign(x[:k] + 1e-30) * 2.0 ** (i - 1) * (2.0 ** round(np.log2(scale)))
            x[k:] = 0
    return ps, gs


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "random"])
@pytest.mark.parametrize("norm_type", [2.0, INF])
@pytest.mark.parametrize("momentum,dampening,weight_decay,nesterov,maximize", OPTIONS)
def test_references_agree_with_torch_clip_and_sgd(norm_type, momentum, dampening, weight_decay, nesterov, maximize, dyadic):
    """The 1 ulp between the float64 norm and torch's is asserted where torch's own fp32 summation adds no error: on the ``dyadic``
    gradients, and for the inf norm on any data (exact).  On ``random`` data with norm 2 torch's fp32 sums are themselves several
    ulps from float64, so nothing is asserted about its total there; the coefficient, the scaled gradients and the step are
    asserted on both kinds of data."""
    kw = dict(momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
    ps, _ = _state(1)
    params = [torch.nn.Parameter(p.clone()) for p in ps]
    opt = torch.optim.SGD(params, lr=LR, **kw)
    for step, (max_norm, scale) in enumerate(((1.0, 1.0), (1e9, 1.0), (2.0 ** -10, 0.01))):   # clipped, not clipped, clipped again
        _, gs = _state(10 + step, scale, dyadic)
        before = [p.detach().numpy().copy() for p in params]
        bufs = [opt.state[p]["momentum_buffer"].numpy().copy() if momentum != 0 and step else None for p in params]
        for p, g in zip(params, gs):
            p.grad = g.clone()
        total = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=norm_type)
        assert total.dtype == torch.float32
        want = CR.total_norm64([g.numpy() for g in gs], norm_type)
        if dyadic or norm_type == INF:
            assert CR.within_ulp32(total.item(), want), (total.item(), want)
        if norm_type == INF:
            assert float(total) == want
        coef = torch.clamp(max_norm / (total + 1e-6), max=1.0).numpy()[()]              # torch's own coefficient
        assert coef.dtype == np.float32 and (coef < 1.0) == (max_norm < 1e9)
        assert R.same_bits(CR.coef32(total.item(), max_norm), coef) and R.same_bits(CR.coef32_np(total.item(), max_norm), coef)
        for p, g in zip(params, gs):
            assert R.same_bits(p.grad.numpy(), CR.scaled32(g.numpy(), coef))
        opt.step()
        for p, b0, g, buf in zip(params, before, gs, bufs):
            p32, b32 = CR.clipped_sgd32(b0, g.numpy(), coef, buf, momentum != 0 and step == 0, LR, **kw)
            assert R.same_bits(p.detach().numpy(), p32), f"step {step}: not torch's bits"
            if momentum != 0:
                assert R.same_bits(opt.state[p]["momentum_buffer"].numpy(), b32)


def test_coefficient_restatement_over_many_norms():
    rng = np.random.default_rng(3)
    totals = np.concatenate([np.float32(10.0) ** rng.uniform(-8, 8, 4000).astype(np.float32),
                             np.array([0.0, 1e-6, 1.0, 2.5, np.inf, np.nan], np.float32)])
    for max_norm in (0.1, 1.0, 2.5, 35.0):
        for t in totals:
            assert R.same_bits(CR.coef32(t, max_norm), CR.coef32_np(t, max_norm)), (t, max_norm)
    assert CR.coef32(np.inf, 1.0) == 0.0 and np.isnan(CR.coef32(np.nan, 1.0)) and CR.coef32(0.5, 1.0) == 1.0


def test_norm_reference_propagates_nan_and_inf():
    g = [np.array([1.0, -3.0], np.float32), np.array([2.0], np.float32)]
    assert CR.total_norm64(g, INF) == 3.0 and CR.total_norm64(g, 2.0) == np.sqrt(14.0) and CR.total_norm64([], 2.0) == 0.0
    g[1][0] = np.nan
    assert np.isnan(CR.total_norm64(g, INF)) and np.isnan(CR.total_norm64(g, 2.0))
    g[1][0] = -np.inf
    assert CR.total_norm64(g, INF) == np.inf and CR.total_norm64(g, 2.0) == np.inf
    assert CR.within_ulp32(np.float32(np.inf), np.inf) and not CR.within_ulp32(np.float32(1.0), np.nan)
    assert CR.within_ulp32(np.float32(1.0) + np.spacing(np.float32(1.0)), 1.0) and not CR.within_ulp32(np.float32(1.0) + 3 * np.spacing(np.float32(1.0)), 1.0)


NEW_ENTRIES = ("seam_grad_norm_workspace_bytes", "seam_grad_norm_f32", "seam_grad_scale_f32", "seam_sgd_step_clip_f32")


def test_new_entries_are_declared_and_bound_with_equal_arity():
    import ctypes as C
    from seam_match_rcnn_amd import _native as N
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "seam_hip.h")).read()
    for name in NEW_ENTRIES:
        m = re.search(r"\b" + name + r"\(([^;]*?)\);", header, re.S)
        assert m, f"{name} is not declared in include/seam_hip.h"
        declared = [a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"]
        assert name in N.SIGNATURES and len(N.SIGNATURES[name][1]) == len(declared), name
        assert hasattr(N.lib(), name)
    assert C.sizeof(N.ClipRecord) == 24 and N.ClipRecord.nonfinite_steps.offset == 16 and C.sizeof(N.SgdTensor) == 40
    assert N.SgdTensor.slot.offset == 36
    assert N.lib().seam_grad_norm_workspace_bytes(0) == 8 and N.lib().seam_grad_norm_workspace_bytes(5) == 40
    assert N.lib().seam_grad_norm_workspace_bytes(-1) < 0


def test_refused_arguments_without_a_gpu():
    from seam_match_rcnn_amd import _native, optim
    for bad in (1.0, 3.0, 0.0, -INF):
        with pytest.raises(ValueError, match=re.escape(str(float(bad)))):
            optim.clip_grad_norm_([], 1.0, norm_type=bad)
        with pytest.raises(ValueError, match=re.escape(str(float(bad)))):
            optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1, max_norm=1.0, norm_type=bad)
    p = torch.nn.Parameter(torch.zeros(3))
    p.grad = torch.ones(3)
    with pytest.raises(_native.SeamNativeError, match="parameter 0 .*not on the HIP device"):
        optim.clip_grad_norm_([p], 1.0)
    out = optim.clip_grad_norm_([torch.nn.Parameter(torch.zeros(3))], 1.0, foreach=True)      # no gradient anywhere: torch's zero
    assert out.dtype == torch.float32 and out.dim() == 0 and float(out) == 0.0
    assert float(optim.clip_grad_norm_([], 1.0, norm_type=INF)) == 0.0
