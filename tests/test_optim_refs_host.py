"""CPU: the yardsticks of the optimizer tests.  ``optim_refs.sgd32`` (the NumPy float32 restatement of the update) and
``torch.optim.SGD`` on the CPU are both stepped from a common state and both must lie within ``optim_refs.bound`` of the float64
evaluation -- torch too, because its ``add_(x, alpha=a)`` may fuse.  Both are re-seeded from torch's state before every step, so
nothing compounds.  Also here: the host logic of the kernel's chunk table, and what the optimizer refuses without a GPU."""
import numpy as np
import pytest
import torch

import optim_refs as R

LR = 0.02


def _state(seed, n=4099):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g) * torch.logspace(-3, 2, n)
    grad = torch.randn(n, generator=g) * torch.logspace(2, -3, n)
    return p, grad


@pytest.mark.parametrize("momentum,dampening,weight_decay,nesterov,maximize", R.OPTIONS)
def test_restatement_and_torch_stay_inside_the_bound(momentum, dampening, weight_decay, nesterov, maximize):
    kw = dict(momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov, maximize=maximize)
    p0, _ = _state(1)
    param = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([param], lr=LR, **kw)
    for step in range(3):                       # the first step creates the buffer, the later ones read it
        _, grad = _state(10 + step)
        lr = LR * (1.0, 0.5, 0.25)[step]
        opt.param_groups[0]["lr"] = lr
        p = param.detach().numpy().copy()       # both references start from torch's state
        buf = opt.state[param].get("momentum_buffer") if param in opt.state else None
        buf = None if buf is None else buf.numpy().copy()
        first = momentum != 0 and buf is None
        assert first == (momentum != 0 and step == 0)
        param.grad = grad.clone()
        opt.step()
        p32, b32 = R.sgd32(p, grad.numpy(), buf, first, lr, **kw)
        p64, b64 = R.sgd64(p, grad.numpy(), buf, first, lr, **kw)
        tol = R.bound(p, grad.numpy(), buf, lr, momentum, weight_decay)
        assert R.within(p32, p64, tol), f"step {step}: restatement outside the bound"
        assert R.within(param.detach().numpy(), p64, tol), f"step {step}: torch outside the bound"
        if momentum != 0:
            tb = opt.state[param]["momentum_buffer"].numpy()
            # the buffer: at most three roundings of partial results that |g| + wd |p| + momentum |buf| dominates
            btol = 4 * R.U * (np.abs(grad.numpy().astype(np.float64)) + weight_decay * np.abs(p.astype(np.float64))
                              + momentum * (0.0 if buf is None else np.abs(buf.astype(np.float64))))
            assert R.within(b32, b64, btol) and R.within(tb, b64, btol)
        else:
            assert b32 is None and opt.state.get(param, {}).get("momentum_buffer") is None


def test_restatement_propagates_inf_and_nan():
    p = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    g = np.array([np.inf, -np.inf, np.nan, 1.0], np.float32)
    out, buf = R.sgd32(p, g, None, True, 0.1, momentum=0.9)
    assert out[0] == -np.inf and out[1] == np.inf and np.isnan(out[2]) and out[3] == np.float32(4.0) - np.float32(0.1) * np.float32(1.0)
    assert R.same_bits(buf, g)


@pytest.mark.parametrize("chunk", [1, 4, 8192])
def test_chunk_table_covers_every_element_once(chunk):
    from seam_match_rcnn_amd import ops
    numels = [0, 1, 3, 4, 5, 255, 0, 256, 257, 1023, 4099, 8191, 8192, 8193, 3 * 8192 + 77, 0]
    rows = ops.sgd_chunk_table(numels, chunk)
    R.check_chunk_table(rows, numels, chunk)
    assert len(rows) == sum(-(-n // chunk) for n in numels)
    assert ops.sgd_chunk_table([], chunk) == [] and ops.sgd_chunk_table([0, 0], chunk) == []
    with pytest.raises(ValueError):
        ops.sgd_chunk_table([3, -1], chunk)


def test_the_uploaded_tables_are_the_abi_structs():
    import ctypes as C
    from seam_match_rcnn_amd import _native as N
    assert (C.sizeof(N.SgdTensor), C.sizeof(N.SgdChunk), C.sizeof(N.SgdGroup)) == (40, 16, 32)
    assert C.sizeof(N.SgdGroups) == 16 + 32 * N.SGD_MAX_SLOTS and C.sizeof(N.RepackJob) == 80
    assert N.lib().seam_sgd_chunk_elems() == 8192


def test_optimizer_refuses_cpu_parameters_and_bad_arguments():
    from seam_match_rcnn_amd import _native
    from seam_match_rcnn_amd.optim import SGD
    with pytest.raises(_native.SeamNativeError, match="parameter 0 of group 0"):
        SGD([torch.nn.Parameter(torch.zeros(3))], lr=0.1)
    m = torch.nn.Linear(3, 2)
    with pytest.raises(_native.SeamNativeError, match="bias"):
        SGD([{"params": [m.bias]}], lr=0.1, model=_Named(m))
    for bad in (dict(lr=-1.0), dict(lr=0.1, momentum=-0.5), dict(lr=0.1, weight_decay=-1.0), dict(lr=0.1, nesterov=True),
                dict(lr=0.1, momentum=0.9, dampening=0.1, nesterov=True)):
        with pytest.raises(ValueError):
            SGD([torch.nn.Parameter(torch.zeros(3))], **bad)


class _Named(torch.nn.Module):
    """a model without the covered sub-modules: the optimizer still takes its parameter names from it"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner
