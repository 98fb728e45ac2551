#!/usr/bin/env python3
"""Time of gradient clipping around the optimizer step of the phase-1 training loop (GPU box; HIP events): the parameter set of
tools/optim_step_timing.py (``body234``: the 8-frame 800x1333 step's model, layer2..4 + FPN + RPN + heads trainable), with seeded
random gradients of the parameters' shapes -- the routes' times depend on the tensor list and its bytes, not on the values -- and
``model=None``: the pack refresh is the same launch on every route and is timed in profiles/optim_step.txt.

  (a) parent   ``torch.nn.utils.clip_grad_norm_`` followed by ``optim.SGD.step()``
  (b) two-step ``optim.clip_grad_norm_`` followed by ``optim.SGD.step()``
  (c) fused    ``optim.SGD(max_norm=..., skip_nonfinite=True).step()``
  (d) floor    ``optim.SGD.step()`` without clipping
  norm         ``seam_grad_norm_f32`` alone: back to back (the 193 MB of gradients stay in the 256 MiB Infinity Cache: a cache-warm
               rate, not an HBM one) and one call at a time after a 512 MiB fill has evicted them (the HBM rate; the single call's
               launch latency is inside the figure).  Routes (c) and (d) are timed the second way too, because back to back the
               step's read of the gradients can hit what the norm just pulled into that cache.

The routes alternate in one process -- a, b, c, d, a, c -- so the two (a) lines and the two (c) lines show the run-to-run spread.
Every route has its own optimizer (its own momentum buffers) over the same parameters and gradients.  Launches per route are
counted with the torch profiler over one call (device kernels and memsets), when it is available.
Usage: python tools/optim_clip_timing.py [--reps N] [out.txt]"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from body_train_timing import body_model  # noqa: E402
from fpn_train_timing import N, dev, timeit  # noqa: E402

import torch  # noqa: E402

from seam_match_rcnn_amd import _native  # noqa: E402
from seam_match_rcnn_amd.optim import SGD, clip_grad_norm_  # noqa: E402

HBM_ROOF = 6.3e12          # bytes/s a streaming kernel reaches on this chip
LR, MOMENTUM, MAX_NORM = 1e-4, 0.9, 10.0


def launches(fn):
    """names of the device activities (kernels, memsets, copies) of one call, or None without a working profiler"""
    try:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")
                 and not e.name.startswith("Optimizer.step")]           # the optimizer's own range marker is mirrored on the device line
        return names or None
    except Exception as e:                      # the count is a note in the record, not what the tool is for
        print(f"launch count not measured: {type(e).__name__}: {e}")
        return None


def cold(fn, reps=10):
    """mean time of single calls, each after a fill of twice the Infinity Cache's size has evicted what the last one touched"""
    scratch = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total = 0.0
    for _ in range(reps):
        scratch.fill_(1)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        total += e0.elapsed_time(e1)
    return total / reps


def short(names):
    """'3 x kernel_a, 1 x kernel_b' with template arguments and namespaces dropped"""
    seen = {}
    for n in names:
        n = n.replace("(anonymous namespace)::", "").split("(")[0].split("<")[0].split("::")[-1].replace("void ", "")[:48]
        seen[n] = seen.get(n, 0) + 1
    return ", ".join(f"{c} x {n}" for n, c in seen.items())


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 50
    if "--reps" in sys.argv:
        args = [a for a in args if a != str(reps)]
    m = body_model(3)
    params = [p for p in m.parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(0)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=dev) * 1e-2
    numel = sum(p.numel() for p in params)
    kw = dict(lr=LR, momentum=MOMENTUM)
    plain, two, fused, floor = SGD(params, **kw), SGD(params, **kw), SGD(params, max_norm=MAX_NORM, skip_nonfinite=True, **kw), SGD(params, **kw)

    def route_a():
        torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        plain.step()

    def route_b():
        clip_grad_norm_(params, MAX_NORM)
        two.step()

    def route_c():
        fused.step()

    def route_d():
        floor.step()

    # the routes agree before anything is timed: the same norm (fp32 sums against fp64: 1e-5 relative), the same clipped gradients
    want = float(torch.nn.utils.get_total_norm([p.grad for p in params]))
    got = float(clip_grad_norm_(params, 1e30))
    assert abs(got - want) <= 1e-5 * want, (got, want)
    res = {}
    for name, fn in (("a1", route_a), ("b", route_b), ("c1", route_c), ("d", route_d), ("a2", route_a), ("c2", route_c)):
        res[name] = timeit(fn, reps)
    assert fused.skipped_steps() == 0 and abs(float(fused.total_norm) - float(clip_grad_norm_(params, 1e30))) <= 1e-5 * want
    count = {name: launches(fn) for name, fn in (("a", route_a), ("b", route_b), ("c", route_c), ("d", route_d))}
    # the norm alone on the fused optimizer's own tables
    tt, ct, n_chunks = fused._tables
    lib, stream = _native.lib(), torch.cuda.current_stream().cuda_stream
    ws, rec = fused._norm_ws, fused._rec

    def norm():
        _native.check(lib.seam_grad_norm_f32(C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()), n_chunks, 0, 1, MAX_NORM, 1,
                                             C.c_void_p(ws.data_ptr()), ws.numel() * 8, C.c_void_p(rec.data_ptr()), stream), "seam_grad_norm_f32")
    tn = timeit(norm, 50)
    tn_cold, c_cold, d_cold = cold(norm), cold(route_c), cold(route_d)
    a, c = 0.5 * (res["a1"] + res["a2"]), 0.5 * (res["c1"] + res["c2"])
    spread = max(abs(res["a1"] - res["a2"]), abs(res["c1"] - res["c2"]))
    read = 4 * numel / HBM_ROOF * 1e3
    cnt = lambda k: "not measured" if count[k] is None else str(len(count[k]))
    lines = [
        f"gradient clipping around the optimizer step, body234 parameter set ({numel / 1e6:.1f} M elements in {len(params)} tensors, {n_chunks} chunks), "
        f"{N}-frame configuration; ms (HIP events, 3 warm-up + {reps} timed), model=None, max_norm {MAX_NORM}",
        f"(a) parent   torch clip_grad_norm_ + optim.SGD.step()        {res['a1']:8.3f}   launches {cnt('a')}",
        f"(b) two-step optim.clip_grad_norm_ + optim.SGD.step()        {res['b']:8.3f}   launches {cnt('b')}",
        f"(c) fused    optim.SGD(max_norm=, skip_nonfinite=).step()    {res['c1']:8.3f}   launches {cnt('c')}",
        f"(d) floor    optim.SGD.step(), no clipping                   {res['d']:8.3f}   launches {cnt('d')}",
        f"(a) parent   again                                           {res['a2']:8.3f}",
        f"(c) fused    again                                           {res['c2']:8.3f}",
        f"spread       {spread:.3f} ms (the larger of the two repeats' differences)",
        f"(a) - (c)    {a - c:.3f} ms = {(a - c) / max(spread, 1e-9):.1f} x the spread; (c) / (a) = {c / a:.3f}: "
        + ("(c) is faster than (a) by more than three times the spread" if a - c > 3 * spread
           else "(c) is NOT faster than (a) by more than three times the spread"),
        f"(c) - (d)    {c - res['d']:.3f} ms against one read of the gradients at the {HBM_ROOF / 1e12:.1f} TB/s streaming roof, {read:.3f} ms "
        f"({(c - res['d']) / read:.2f} x that floor)",
        f"norm         seam_grad_norm_f32 alone (two launches: per-chunk fp64 partials, one-block finish), back to back: {tn:.4f} ms = "
        f"{4 * numel / tn * 1e-6:.0f} GB/s of 4 B/element -- CACHE-WARM: the {4 * numel / 1e6:.0f} MB of gradients fit the 256 MiB Infinity Cache, "
        f"this is not an HBM rate",
        f"norm cold    one call at a time after a 512 MiB fill evicted the gradients (10 calls, launch latency included): {tn_cold:.4f} ms = "
        f"{4 * numel / tn_cold * 1e-6:.0f} GB/s = {4 * numel / (tn_cold * 1e-3) / HBM_ROOF * 100:.0f} % of the {HBM_ROOF / 1e12:.1f} TB/s streaming roof",
        f"(c), (d) cold  single calls after the same eviction: fused {c_cold:.3f}, unclipped {d_cold:.3f}; (c) - (d) = {c_cold - d_cold:.3f} ms = "
        f"{(c_cold - d_cold) / read:.2f} x one read of the gradients at the roof (back to back, above, the step's read of g can hit the cache)",
    ]
    lines += [f"launches ({k})  {short(v)}" for k, v in count.items() if v is not None]
    print("\n".join(lines))
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
