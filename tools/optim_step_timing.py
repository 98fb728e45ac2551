#!/usr/bin/env python3
"""Time of the optimizer step of the phase-1 training loop (GPU box; HIP events): the step of tools/body_train_timing.py in the
``body234`` configuration (8 frames 800x1333, layer2..4 + FPN + RPN + heads trainable, synthetic weights), with

  (a) torch   ``torch.optim.SGD.step()`` plus the repack the next forward triggers: ``packed()`` of body, FPN and RPN head
  (b) seam    ``seam_match_rcnn_amd.optim.SGD.step()`` including ``PackPlan.refresh()``
  (c) loop    the whole iteration (zero_grad, forward, backward, step) on both routes
  kernel      ``seam_sgd_step_f32`` alone, back to back: GB/s with the bytes counted from the shapes (20 per element with momentum)

The routes alternate in one call -- a, b, a -- so the two (a) lines show the run-to-run spread.  Before timing, the two routes take
one step from the same state and the tool asserts: parameters within twice the per-element bound of the SGD arithmetic
(tests/optim_refs.py: each route is within the bound of float64), and refresh_packs on versus off bit for bit.  The next step's
losses of the two routes are printed and held to 2e-2 relative only: last-bit differences of the parameters reorder proposals and
swap sampled RoIs, and one swapped sample of the 8 x 512 moves the classifier's mean cross-entropy (about ln 14 per untrained
sample) by up to 6e-4 of itself.

``--repack-only``: nothing but REPS repacks of route (a) (for ``rocprofv3 --kernel-trace --stats -- python tools/optim_step_timing.py
--repack-only --reps N``; the difference of two such runs with different N counts the repack's launches and kernel time).
Usage: python tools/optim_step_timing.py [--reps N] [--repack-only] [out.txt]"""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from body_train_timing import body_model  # noqa: E402
from fpn_train_timing import N, batch, dev, step_of, timeit  # noqa: E402

import torch  # noqa: E402

from seam_match_rcnn_amd import _native  # noqa: E402
from seam_match_rcnn_amd.optim import SGD  # noqa: E402

HBM_ROOF = 6.3e12          # bytes/s a streaming kernel reaches on this chip
LR, MOMENTUM = 1e-4, 0.9


def covered(m):
    return (m.backbone.body, m.backbone.fpn, m.rpn.head)


def trainable(m):
    return [p for p in m.parameters() if p.requires_grad]


def wall(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def repack_only(reps):
    m = body_model(3)
    ps = trainable(m)
    for mod in covered(m):
        mod.packed()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        for p in ps:
            torch.autograd.graph.increment_version(p)
        for mod in covered(m):
            mod.packed()
    torch.cuda.synchronize()
    print(f"repack-only: {reps} repacks of body + FPN + RPN head, wall {(time.perf_counter() - t0) * 1e3 / max(reps, 1):.3f} ms each")


def check_outputs(images, targets):
    """one step on each route from the same state: parameters within the arithmetic's bound, next-step losses close; on == off"""
    outs = {}
    base = body_model(3)
    step_of(base, images, targets)()
    for name in ("torch", "seam", "seam_off"):
        m = body_model(3)                          # the same synthetic weights; the gradients are base's
        for p, q in zip(m.parameters(), base.parameters()):
            p.grad = None if q.grad is None else q.grad.clone()
        before = [p.detach().double() for p in trainable(m)]
        grads = [p.grad.detach().double().abs() for p in trainable(m)]
        if name == "torch":
            opt = torch.optim.SGD(trainable(m), lr=LR, momentum=MOMENTUM)
        else:
            opt = SGD(trainable(m), lr=LR, momentum=MOMENTUM, model=m, refresh_packs=name == "seam")
        opt.step()
        m.rpn.sample_generator = torch.Generator(device=dev).manual_seed(1)
        m.roi_heads.sample_generator = torch.Generator(device=dev).manual_seed(2)
        losses = {k: float(v) for k, v in m(images, targets).items()}
        outs[name] = ([p.detach().clone() for p in trainable(m)], losses, before, grads)
        del m, opt
        torch.cuda.empty_cache()
    (pt, lt, before, grads), (ps, ls, _, _), (po, lo, _, _) = outs["torch"], outs["seam"], outs["seam_off"]
    worst = 0.0
    for a, b, p0, g in zip(pt, ps, before, grads):
        bound = 8 * 2.0 ** -24 * (p0.abs() + LR * (1 + MOMENTUM) * g)           # first step: no buffer, no weight decay
        worst = max(worst, float(((a.double() - b.double()).abs() / (2 * bound).clamp_min(1e-300)).max()))
    assert worst <= 1.0, f"parameters of the two routes differ by {worst:.2f} x twice the bound of the SGD arithmetic"
    nan = lambda x: x != x
    assert all(nan(lt[k]) == nan(ls[k]) for k in lt), (lt, ls)
    rel = max([abs(lt[k] - ls[k]) / max(abs(lt[k]), 1e-12) for k in lt if not nan(lt[k])] + [0.0])
    assert rel <= 2e-2, (lt, ls)
    assert all(torch.equal(a, b) for a, b in zip(ps, po)) and all(ls[k] == lo[k] or (nan(ls[k]) and nan(lo[k])) for k in ls), \
        "refresh_packs on / off must agree bit for bit"
    return worst, rel


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 10
    if "--reps" in sys.argv:
        args = [a for a in args if a != str(reps)]
    if "--repack-only" in sys.argv:
        return repack_only(reps)
    images, targets = batch()
    worst, rel = check_outputs(images, targets)
    lines = [f"optimizer step of the phase-1 training loop, body234, {N} frames 800x1333; ms (HIP events / host clock, 3 warm-up + {reps} timed)",
             f"outputs   one step, torch route vs this optimizer: parameters within {worst:.2f} x (2 x bound of the SGD arithmetic), next-step "
             f"losses within {rel:.1e} relative; refresh_packs on vs off: bit for bit"]
    mt, ms = body_model(3), body_model(3)
    it_t, it_s = step_of(mt, images, targets), step_of(ms, images, targets)
    it_t()
    it_s()
    ot = torch.optim.SGD(trainable(mt), lr=LR, momentum=MOMENTUM)
    osm = SGD(trainable(ms), lr=LR, momentum=MOMENTUM, model=ms)
    numel = sum(p.numel() for p in trainable(ms))

    def route_a():
        ot.step()
        for mod in covered(mt):
            mod.packed()

    def repack_a():
        for p in trainable(mt):
            torch.autograd.graph.increment_version(p)
        for mod in covered(mt):
            mod.packed()

    def route_b():
        osm.step()

    def loop_a():
        it_t()
        ot.step()

    def loop_b():
        it_s()
        osm.step()

    res = {}
    for name, fn in (("a1", route_a), ("b", route_b), ("a2", route_a)):
        res[name] = (timeit(fn, reps), wall(fn, reps))
    res["repack"] = (timeit(repack_a, reps), wall(repack_a, reps))
    for name, fn in (("loop_a1", loop_a), ("loop_b", loop_b), ("loop_a2", loop_a)):
        res[name] = (timeit(fn, max(3, reps // 2), warm=2), 0.0)
    # the SGD kernel alone, back to back on the optimizer's own tables
    tt, ct, n_chunks = osm._tables
    groups = _native.SgdGroups()
    groups.n = 2
    for s in (0, 1):
        groups.g[s].lr, groups.g[s].momentum, groups.g[s].one_minus_dampening = LR, MOMENTUM, 1.0
    lib, stream = _native.lib(), torch.cuda.current_stream().cuda_stream
    def kernel(fp):
        return lambda: _native.check(lib.seam_sgd_step_f32(C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()), n_chunks, C.byref(groups),
                                                           fp, stream), "seam_sgd_step_f32")
    tk = timeit(kernel(None), 50)
    tkf = timeit(kernel(C.c_void_p(osm._fp[0].data_ptr())), 50)        # with the parameter fingerprint (and its 1 KiB clear)
    tk2 = timeit(kernel(None), 50)
    spread = abs(res["a1"][0] - res["a2"][0])
    a = 0.5 * (res["a1"][0] + res["a2"][0])
    lines += [
        f"(a) torch  SGD.step() + packed() of body, FPN, RPN head      {res['a1'][0]:8.3f}   (host clock {res['a1'][1]:8.3f})",
        f"(b) seam   optim.SGD.step() with PackPlan.refresh()          {res['b'][0]:8.3f}   (host clock {res['b'][1]:8.3f})",
        f"(a) torch  again                                             {res['a2'][0]:8.3f}   (host clock {res['a2'][1]:8.3f})",
        f"    the repack of route (a) alone (versions bumped, packed()) {res['repack'][0]:7.3f}   (host clock {res['repack'][1]:8.3f})",
        f"(c) loop   zero_grad + forward + backward + step, torch      {res['loop_a1'][0]:8.2f}   seam {res['loop_b'][0]:8.2f}   torch again {res['loop_a2'][0]:8.2f}",
        f"ratio      (b) / (a) = {res['b'][0] / a:.3f}; (a) - (b) = {a - res['b'][0]:.3f} ms against a spread of {spread:.3f} ms between the two (a) lines: "
        + ("(b) is below (a) by more than the spread" if a - res['b'][0] > spread else "(b) is NOT below (a) by more than the spread"),
        f"kernel     seam_sgd_step_f32 over {numel / 1e6:.1f} M elements in {len(trainable(ms))} tensors, {n_chunks} chunks: {tk:.4f} ms = "
        f"{20 * numel / tk * 1e-6:.0f} GB/s of 20 B/element = {20 * numel / (tk * 1e-3) / HBM_ROOF * 100:.0f} % of the {HBM_ROOF / 1e12:.1f} TB/s streaming roof",
        f"           with the fingerprint of the parameters read and written (what step() launches when it refreshes packs): {tkf:.4f} ms = "
        f"{20 * numel / tkf * 1e-6:.0f} GB/s; without, again: {tk2:.4f} ms",
        f"refresh    launches_per_refresh {osm.plan.launches_per_refresh}, fallback_calls {osm.plan.fallback_calls} (torch re-derivations), "
        f"table_uploads {osm.plan.table_uploads} (plan) + {osm.table_uploads} (tensor table), rebuilds {osm.plan.rebuilds}, refreshes {osm.plan.refreshes}",
    ]
    print("\n".join(lines))
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
