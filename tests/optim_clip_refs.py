"""References for gradient clipping by global norm (seam_match_rcnn_amd.optim: ``SGD(max_norm=...)``, ``clip_grad_norm_``;
csrc/seam_optim.hip).

``total_norm64``  the global norm of a list of fp32 gradients in float64: norm 2 as the square root of the sum of the exact float64
                  squares (NumPy's pairwise sum: relative error below n * 2^-53), norm inf as the largest magnitude; a NaN anywhere
                  makes the total NaN, as ``torch.max`` does.
``coef32``        ``clip_grad_norm_``'s coefficient with torch CPU fp32 ops exactly as torch writes them:
                  ``clamp(max_norm / (total_norm + 1e-6), max=1.0)`` on an fp32 tensor.  ``max_norm / tensor`` is
                  ``Tensor.__rtruediv__``: ``tensor.reciprocal() * max_norm``, two roundings, and the clamp keeps NaN.
``coef32_np``     the same, one NumPy fp32 operation per line: what the kernel computes.
``clipped_sgd32`` the clipped step: ``optim_refs.sgd32`` on ``g * coef`` (one rounded fp32 multiply, what ``g.mul_(coef)`` stores).
``within_ulp32``  |got - want64| <= one fp32 unit in the last place of want64 (non-finite values: the same kind).
"""
import numpy as np
import torch

import optim_refs as R

F = np.float32


def total_norm64(grads, norm_type):
    grads = [np.asarray(g, F).astype(np.float64).reshape(-1) for g in grads if g is not None]
    if not grads:
        return 0.0
    with np.errstate(all="ignore"):
        if norm_type == float("inf"):
            if any(np.isnan(g).any() for g in grads):
                return float("nan")
            return float(max([np.abs(g).max() for g in grads if g.size] + [0.0]))
        assert norm_type == 2.0
        return float(np.sqrt(np.sum(np.concatenate([g * g for g in grads]), dtype=np.float64)))


def coef32(total32, max_norm):
    total = torch.tensor(float(total32), dtype=torch.float32)
    clip_coef = float(max_norm) / (total + 1e-6)
    return F(torch.clamp(clip_coef, max=1.0).item())


def coef32_np(total32, max_norm):
    with np.errstate(all="ignore"):
        den = F(F(total32) + F(1e-6))
        rcp = F(F(1.0) / den)
        c = F(rcp * F(max_norm))
        return F(1.0) if c > F(1.0) else c


def scaled32(grad, coef):
    with np.errstate(all="ignore"):
        return (np.asarray(grad, F) * F(coef)).astype(F)


def clipped_sgd32(p, grad, coef, buf, first, lr, **kw):
    return R.sgd32(p, scaled32(grad, coef), buf, first, lr, **kw)


def within_ulp32(got32, want64, ulps=1) -> bool:
    got, want = float(got32), float(want64)
    if not np.isfinite(want) or not np.isfinite(got):
        return (np.isnan(want) and np.isnan(got)) or got == want
    with np.errstate(all="ignore"):
        w32 = F(want)
    if not np.isfinite(w32):
        return False
    return abs(got - want) <= ulps * float(np.spacing(np.abs(w32)))
