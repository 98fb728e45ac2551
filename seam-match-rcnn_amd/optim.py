"""``SGD``: the optimizer step of the training loop on the device -- a drop-in for ``torch.optim.SGD`` (ref train_matchrcnn.py:70-72,
stuffs/engine.py:62-64).

``step()`` is one launch of ``seam_sgd_step_f32`` over every parameter that has a gradient (csrc/seam_optim.hip: torch's arithmetic,
each multiply and add rounded on its own), then one version bump per updated parameter (every pack cache keyed on versions
invalidates by its usual rule) and, when ``model`` is given, ``ops.PackPlan.refresh``: the cached packs of the ResNet body, the FPN
and the RPN head are rewritten in place in one more launch, so the next forward finds them valid.  Everything else that caches a
pack (the eval-mode heads, the match heads) repacks lazily as before.

State (``momentum_buffer``), ``state_dict()`` / ``load_state_dict()``, ``add_param_group``, ``zero_grad`` and the schedulers are
those of ``torch.optim.Optimizer``; a checkpoint written by either optimizer loads into the other.
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.optim.optimizer import Optimizer

from . import _native, ops

MAX_GROUPS = _native.SGD_MAX_SLOTS // 2      # a group takes two kernel slots: buffers that exist, buffers created this step


class SGD(Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, model=None, refresh_packs=True):
        """``torch.optim.SGD``'s arguments (``foreach`` / ``fused`` are accepted and ignored: there is one implementation), plus
        ``model``: the detector whose body / FPN / RPN-head packs ``step()`` refreshes in place (None: the kernel only), and
        ``refresh_packs``: False keeps ``model``'s packs on the lazy route."""
        if isinstance(lr, torch.Tensor):
            raise ValueError("SGD: lr must be a number (it travels in the kernel arguments)")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if differentiable:
            raise ValueError("SGD: differentiable=True is not supported")
        self._names = {}
        if model is not None:
            self._names = {id(p): n for n, p in model.named_parameters()}
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)
        self.refresh_packs = bool(refresh_packs)
        self.plan = ops.PackPlan(model) if model is not None else None
        if self.plan is not None and self.refresh_packs:
            with torch.no_grad():
                self.plan.build()
        self.table_uploads = 0
        self._key = None
        self._tables = None
        self._fp = None              # (device uint64 sums, pinned host copy, event) of the kernel's parameter fingerprint
        self._fp_last = None         # (parameter list, "as written" sum) of the previous step

    def __setstate__(self, state):
        super().__setstate__(state)
        for group in self.param_groups:
            group.setdefault("nesterov", False)
            group.setdefault("maximize", False)
            group.setdefault("foreach", None)
            group.setdefault("differentiable", False)
            group.setdefault("fused", None)

    def _name(self, p) -> str:
        n = self._names.get(id(p))
        if n is not None:
            return n
        for gi, group in enumerate(self.param_groups):
            for pi, q in enumerate(group["params"]):
                if q is p:
                    return f"parameter {pi} of group {gi} (shape {tuple(p.shape)})"
        return f"parameter of shape {tuple(p.shape)}"

    def _check_param(self, p) -> None:
        if p.is_sparse or p.layout != torch.strided:
            raise TypeError(f"SGD: {self._name(p)} is sparse: only dense fp32 parameters are supported")
        if not p.is_cuda:
            raise _native.SeamNativeError(f"SGD: {self._name(p)} is not on the HIP device (no CPU path exists)")
        if p.dtype != torch.float32:
            raise TypeError(f"SGD: {self._name(p)} is {p.dtype}: only float32 parameters are supported")
        if not p.is_contiguous():
            raise ValueError(f"SGD: {self._name(p)} is not contiguous")

    def add_param_group(self, param_group) -> None:
        super().add_param_group(param_group)
        if len(self.param_groups) > MAX_GROUPS:
            self.param_groups.pop()
            raise ValueError(f"SGD: at most {MAX_GROUPS} parameter groups")
        for p in self.param_groups[-1]["params"]:
            self._check_param(p)
        self._key = None             # a new group rebuilds the tables

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._key = None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"SGD: at most {MAX_GROUPS} parameter groups")
        rows, keep, updated = [], [], []
        groups = _native.SgdGroups()
        groups.n = 2 * len(self.param_groups)
        device = None
        for gi, group in enumerate(self.param_groups):
            lr, mom = float(group["lr"]), float(group["momentum"])
            act = []
            for p in group["params"]:
                g = p.grad
                if g is None or p.numel() == 0:
                    continue                 # torch's rule: nothing happens to it, no buffer is created
                self._check_param(p)
                if g.is_sparse or g.layout != torch.strided:
                    raise TypeError(f"SGD: the gradient of {self._name(p)} is sparse")
                if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape:
                    raise TypeError(f"SGD: the gradient of {self._name(p)} is {g.dtype} {tuple(g.shape)} on {g.device}; expected "
                                    f"float32 {tuple(p.shape)} on {p.device}")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise ValueError(f"SGD: {self._name(p)} is on {p.device}, other parameters on {device}")
                if not g.is_contiguous():
                    g = g.contiguous()       # for this step only
                    keep.append(g)
                buf, first = None, False
                if mom != 0:
                    st = self.state[p]
                    buf = st.get("momentum_buffer")
                    if buf is None:
                        buf = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                        first = True
                    elif buf.dtype != torch.float32 or buf.device != p.device or buf.shape != p.shape or not buf.is_contiguous():
                        buf = st["momentum_buffer"] = buf.to(device=p.device, dtype=torch.float32).contiguous()
                act.append((p, g, buf, first))
            # slot 2 gi: the group's tensors; slot 2 gi + 1: those whose buffer is new this step while others' are not
            split = len({a[3] for a in act}) == 2
            for s, first in ((2 * gi, bool(act) and not split and act[0][3]), (2 * gi + 1, True)):
                h = groups.g[s]
                h.lr, h.momentum, h.one_minus_dampening, h.weight_decay = lr, mom, 1 - group["dampening"], group["weight_decay"]
                h.nesterov, h.maximize, h.first = int(bool(group["nesterov"])), int(bool(group["maximize"])), int(first)
            for p, g, buf, first in act:
                rows.append((p, g, buf, 2 * gi + (1 if split and first else 0)))
                updated.append(p)
        if rows:
            key = tuple((p.data_ptr(), g.data_ptr(), 0 if b is None else b.data_ptr(), p.numel(), s) for p, g, b, s in rows)
            lib = _native.lib()
            with torch.cuda.device(device):
                if key != self._key:
                    self._tables = self._build_tables(lib, key, device)
                    self._key = key
                    self.table_uploads += 1
                tt, ct, n_chunks = self._tables
                planned = self.plan is not None and self.refresh_packs
                if planned and self._fp is None:
                    self._fp = (torch.zeros(2 * _native.SGD_FP_SLOTS, dtype=torch.int64, device=device),
                                torch.zeros(2 * _native.SGD_FP_SLOTS, dtype=torch.int64).pin_memory(), torch.cuda.Event())
                fp = self._fp if planned else None
                _native.check(lib.seam_sgd_step_f32(C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()), n_chunks, C.byref(groups),
                                                    None if fp is None else C.c_void_p(fp[0].data_ptr()),
                                                    torch.cuda.current_stream().cuda_stream), "seam_sgd_step_f32")
                if fp is not None:
                    fp[1].copy_(fp[0], non_blocking=True)
                    fp[2].record()
            for p in updated:
                torch.autograd.graph.increment_version(p)
            del keep
            if fp is not None:
                with torch.cuda.device(device):
                    in_place = self.plan.refresh(updated)
                # Everything of this step is queued; now wait for the fingerprint.  What the kernel read must be what the previous
                # step wrote: an edit through ``p.data`` moves no version counter, so this is the only place it shows.  The packs
                # just written are right either way (they come from the current weights); the plan is rebuilt as after any edit.
                fp[2].synchronize()
                sums = fp[1].numpy().view("uint64").reshape(-1, 2).sum(0)
                plist = tuple(k[0] for k in key) + tuple(k[3] for k in key)
                edited = self._fp_last is not None and self._fp_last[0] == plist and self._fp_last[1] != int(sums[0])
                self._fp_last = (plist, int(sums[1]))
                if edited and in_place:
                    with torch.cuda.device(device):
                        self.plan.rebuild_after_edit()
        return loss

    @staticmethod
    def _build_tables(lib, key, device):
        chunk = int(lib.seam_sgd_chunk_elems())
        tensors = (_native.SgdTensor * len(key))()
        for t, (pp, gp, bp, n, slot) in zip(tensors, key):
            t.p, t.g, t.buf, t.numel, t.group = pp, gp, bp or None, n, slot
        crows = ops.sgd_chunk_table([k[3] for k in key], chunk)
        chunks = (_native.SgdChunk * len(crows))()
        for c, (ti, cnt, off) in zip(chunks, crows):
            c.tensor, c.count, c.offset = ti, cnt, off
        return ops._upload(tensors, device), ops._upload(chunks, device), len(crows)
