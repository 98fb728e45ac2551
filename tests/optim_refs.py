"""References for the optimizer step (seam_match_rcnn_amd.optim.SGD, csrc/seam_optim.hip).

``sgd32``  torch.optim.SGD's update restated in NumPy float32, one operation per line, every result rounded to fp32 on its own.
``sgd64``  the same formulas in float64 from the same fp32 inputs (hyper-parameters as the Python floats the optimizer holds).
``bound``  the per-element error budget of ANY fp32 evaluation of these formulas, fused or not, against ``sgd64``:
               8 * u * scale,   u = 2^-24,   scale = |p| + lr * (1 + momentum) * (|g| + weight_decay * |p| + momentum * |buf|)
           The update has at most six roundings (wd * p, its sum, momentum * buf, (1 - dampening) * g, their sum -- or the
           Nesterov product and sum -- lr * g, the final difference), each bounded by u times a partial result that ``scale``
           dominates; 8 leaves room for the fp32 rounding of the hyper-parameters themselves (lr, momentum, 1 - dampening, wd:
           one u each, relative).
"""
import numpy as np

U = 2.0 ** -24
F = np.float32

# the option grid of the host test and the GPU test: (momentum, dampening, weight_decay, nesterov, maximize)
OPTIONS = [(m, d, wd, nes, mx)
           for m in (0.0, 0.9) for d in (0.0, 0.1) for wd in (0.0, 1e-4) for nes in (False, True) for mx in (False, True)
           if not (nes and (m == 0.0 or d != 0.0))]


def sgd32(p, grad, buf, first, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    """-> (p', buf') as float32 arrays; ``buf`` may be None when momentum == 0 or first."""
    with np.errstate(all="ignore"):
        p = np.asarray(p, F)
        g = np.asarray(grad, F)
        if maximize:
            g = -g
        if weight_decay != 0:
            t = (F(weight_decay) * p).astype(F)
            g = (g + t).astype(F)
        if momentum != 0:
            if first:
                buf = g.copy()
            else:
                a = (F(momentum) * np.asarray(buf, F)).astype(F)
                b = (F(1 - dampening) * g).astype(F)
                buf = (a + b).astype(F)
            if nesterov:
                t = (F(momentum) * buf).astype(F)
                g = (g + t).astype(F)
            else:
                g = buf
        s = (F(lr) * g).astype(F)
        return (p - s).astype(F), buf


def sgd64(p, grad, buf, first, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False):
    with np.errstate(all="ignore"):
        p = np.asarray(p, F).astype(np.float64)
        g = np.asarray(grad, F).astype(np.float64)
        if maximize:
            g = -g
        if weight_decay != 0:
            g = g + weight_decay * p
        if momentum != 0:
            if first:
                buf = g.copy()
            else:
                buf = momentum * np.asarray(buf, F).astype(np.float64) + (1 - dampening) * g
            g = g + momentum * buf if nesterov else buf
        return p - lr * g, buf


def bound(p, grad, buf, lr, momentum=0.0, weight_decay=0.0):
    p = np.abs(np.asarray(p, F).astype(np.float64))
    g = np.abs(np.asarray(grad, F).astype(np.float64))
    b = 0.0 if buf is None else np.abs(np.asarray(buf, F).astype(np.float64))
    return 8 * U * (p + lr * (1 + momentum) * (g + weight_decay * p + momentum * b))


def within(got, want64, tol) -> bool:
    """|got - want| <= tol elementwise, NaN equal to NaN, infinities equal by sign."""
    got = np.asarray(got).astype(np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(want64) & np.isfinite(got)
        ok = np.where(fin, np.abs(got - want64) <= tol, (np.isnan(got) & np.isnan(want64)) | (got == want64))
    return bool(ok.all())


def same_bits(a, b) -> bool:
    """bit for bit, except that any NaN equals any NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def check_chunk_table(rows, numels, chunk):
    """Every element of every tensor in exactly one chunk, chunk sizes in 1..chunk, offsets multiples of chunk, none for an empty tensor."""
    seen = [np.zeros(n, np.int32) for n in numels]
    for t, cnt, off in rows:
        assert 0 <= t < len(numels) and 1 <= cnt <= chunk and off % chunk == 0 and off + cnt <= numels[t], (t, cnt, off)
        seen[t][off:off + cnt] += 1
    for t, s in enumerate(seen):
        assert bool((s == 1).all()), f"tensor {t}: an element is covered {s.min()}..{s.max()} times"
    assert all(numels[t] > 0 for t, _, _ in rows)
