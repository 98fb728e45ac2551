"""``SGD``: the optimizer step of the training loop on the device -- a drop-in for ``torch.optim.SGD`` (ref train_matchrcnn.py:70-72,
stuffs/engine.py:62-64).

``step()`` is one launch of ``seam_sgd_step_f32`` over every parameter that has a gradient (csrc/seam_optim.hip: torch's arithmetic,
each multiply and add rounded on its own), then one version bump per updated parameter (every pack cache keyed on versions
invalidates by its usual rule) and, when ``model`` is given, ``pack_plan.PackPlan.refresh``: the cached packs of the ResNet body, the FPN
and the RPN head are rewritten in place in one more launch, so the next forward finds them valid.  Everything else that caches a
pack (the eval-mode heads, the match heads) repacks lazily as before.

State (``momentum_buffer``), ``state_dict()`` / ``load_state_dict()``, ``add_param_group``, ``zero_grad`` and the schedulers are
those of ``torch.optim.Optimizer``; a checkpoint written by either optimizer loads into the other.

``SGD(..., max_norm=, norm_type=, skip_nonfinite=)`` clips by the global gradient norm and drops non-finite steps inside the step:
``seam_grad_norm_f32`` (the norm, the clip coefficient and a finite flag in a small device record), then ``seam_sgd_step_clip_f32``
(the update on ``g * clip_coef``; nothing written when the step is dropped).  No host synchronisation is added.
``clip_grad_norm_`` is ``torch.nn.utils.clip_grad_norm_`` as two launches, for loops that keep another optimizer.
"""
from __future__ import annotations

import ctypes as C
import math

import torch
from torch.optim.optimizer import Optimizer

from . import _native, ops, pack_plan

MAX_GROUPS = _native.SGD_MAX_SLOTS // 2      # a group takes two kernel slots: buffers that exist, buffers created this step


class SGD(Optimizer):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, *, maximize=False,
                 foreach=None, differentiable=False, fused=None, model=None, refresh_packs=True, max_norm=None, norm_type=2.0,
                 skip_nonfinite=False):
        """``torch.optim.SGD``'s arguments (``foreach`` / ``fused`` are accepted and ignored: there is one implementation), plus
        ``model``: the detector whose body / FPN / RPN-head packs ``step()`` refreshes in place (None: the kernel only), and
        ``refresh_packs``: False keeps ``model``'s packs on the lazy route.

        ``max_norm`` (None: no clipping), ``norm_type`` (2 or inf) and ``skip_nonfinite`` make ``step()`` what
        ``torch.nn.utils.clip_grad_norm_(all parameters, max_norm, norm_type)`` followed by ``step()`` is: the norm over every
        parameter of every group that has a gradient this step, torch's coefficient ``min(1, max_norm / (total_norm + 1e-6))`` in
        fp32, and the update on ``g * coefficient``.  ``.grad`` itself is NOT modified on this route: the product lives in the
        kernel's registers.  With ``skip_nonfinite`` a step whose norm is inf or NaN writes no parameter and no momentum buffer
        (what a loop does that leaves ``optimizer.step()`` out for that batch); ``max_norm=None`` with ``skip_nonfinite=True`` runs
        the norm for the flag alone, coefficient 1.  A dropped step still bumps the parameters' versions and refreshes the packs --
        from unchanged weights, so to the same bytes -- because avoiding that would take the synchronisation this route exists to
        avoid.  Without either argument ``step()`` launches exactly what it launched before.

        The three are settings of the instance, not of a group, and are not part of ``state_dict()``, which stays interchangeable
        with ``torch.optim.SGD``'s: pass them again when an optimizer is rebuilt from a checkpoint.  ``total_norm`` and
        ``skipped_steps()`` report what the last step saw.

        One narrow case: a momentum buffer created on a dropped step holds zeros until the first applied step writes ``buf = g'``
        into it, and the device flag that says so is not part of ``state_dict()``.  A checkpoint taken exactly between the two
        carries that zero buffer; an optimizer that loads it takes the buffer as it is (``momentum * 0 + (1 - dampening) * g'`` on
        its next step, which is ``g'`` unless ``dampening`` is set).  Take checkpoints after an applied step, or check
        ``skipped_steps()`` first."""
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
        self.max_norm = None if max_norm is None else float(max_norm)
        self.norm_type = _check_norm_type(norm_type)
        self.skip_nonfinite = bool(skip_nonfinite)
        self._names = {}
        if model is not None:
            self._names = {id(p): n for n, p in model.named_parameters()}
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov,
                        maximize=maximize, foreach=foreach, differentiable=differentiable, fused=fused)
        super().__init__(params, defaults)
        self.refresh_packs = bool(refresh_packs)
        self.plan = pack_plan.PackPlan(model) if model is not None else None
        if self.plan is not None and self.refresh_packs:
            with torch.no_grad():
                self.plan.build()
        self.table_uploads = 0
        self._key = None
        self._tables = None
        self._fp = None              # (device uint64 sums, pinned host copy, event) of the kernel's parameter fingerprint
        self._fp_last = None         # (parameter list, "as written" sum) of the previous step
        self._rec = None             # seam_clip_record_t on the device, as six int32 words
        self._norm_ws = None         # the norm's per-chunk fp64 partials
        self._slots = {}             # id(parameter) -> its index in the pending_first arrays, for the optimizer's life
        self._pending = None         # [2, slots] int32: pending_first as the next launch reads it ([self._pin]) and writes it
        self._pin = 0

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
        if self._pending is not None:
            self._pending.zero_()    # every buffer that exists now was loaded, none is waiting for its first write

    @property
    def clipping(self) -> bool:
        """whether ``step()`` takes the norm + clipped-step route"""
        return self.max_norm is not None or self.skip_nonfinite

    @property
    def total_norm(self):
        """The gradient norm of the last step on the clipped route: a 0-d fp32 device tensor (None before the first such step).  It
        is a view of the device record, so reading it is the caller's synchronisation and the next step overwrites it."""
        return None if self._rec is None else _rec_field(self._rec, "total_norm")

    @property
    def clip_coef(self):
        """The coefficient the last clipped step multiplied the gradients by: a 0-d fp32 view of the device record, as ``total_norm``."""
        return None if self._rec is None else _rec_field(self._rec, "clip_coef")

    def skipped_steps(self) -> int:
        """How many steps had a non-finite norm so far (with ``skip_nonfinite``: how many were dropped).  Reads the device counter:
        the one call here that waits for the device."""
        return 0 if self._rec is None else int(_rec_field(self._rec, "nonfinite_steps").item())

    def _clip_state(self, rows, device):
        """(record, pending_in, pending_out) for this launch; every row's parameter has a slot inside the pending arrays"""
        for p, _, _, _ in rows:
            self._slots.setdefault(id(p), len(self._slots))
        if self._rec is None or self._rec.device != device:
            self._rec = torch.zeros(_REC_WORDS, dtype=torch.int32, device=device)
        n = len(self._slots)
        if self._pending is None or self._pending.device != device or self._pending.shape[1] < n:
            grown = torch.zeros((2, max(n, 16) * 2), dtype=torch.int32, device=device)
            if self._pending is not None and self._pending.device == device:
                grown[:, :self._pending.shape[1]] = self._pending
            self._pending = grown    # both rows copied: they still agree on every tensor outside the tables
        return self._rec, self._pending[self._pin], self._pending[1 - self._pin]

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
                        # the clipped route may drop this step on the device and leave the buffer unwritten until the first
                        # applied one: zeros, so that a state_dict() taken in between holds no uninitialised memory
                        new = torch.zeros_like if self.clipping else torch.empty_like
                        buf = st["momentum_buffer"] = new(p, memory_format=torch.contiguous_format)
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
            clip = self.clipping
            if clip:
                rec, pend_in, pend_out = self._clip_state(rows, device)
            key = tuple((p.data_ptr(), g.data_ptr(), 0 if b is None else b.data_ptr(), p.numel(), s,
                         self._slots[id(p)] if clip else 0) for p, g, b, s in rows)
            lib = _native.lib()
            with torch.cuda.device(device):
                if clip and key != self._key:
                    # a launch writes pending_out only for the tensors of its table: when the table changes, carry the flags of
                    # the tensors that leave it (both arrays agree on a tensor while it is outside every launch)
                    pend_out.copy_(pend_in)
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
                stream = torch.cuda.current_stream().cuda_stream
                if clip:
                    if self._norm_ws is None or self._norm_ws.device != device or self._norm_ws.numel() < max(n_chunks, 1):
                        self._norm_ws = torch.empty(int(lib.seam_grad_norm_workspace_bytes(n_chunks)) // 8, dtype=torch.float64, device=device)
                    _native.check(lib.seam_grad_norm_f32(C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()), n_chunks,
                                                         int(math.isinf(self.norm_type)), int(self.max_norm is not None),
                                                         0.0 if self.max_norm is None else self.max_norm, 1,
                                                         C.c_void_p(self._norm_ws.data_ptr()), self._norm_ws.numel() * 8,
                                                         C.c_void_p(rec.data_ptr()), stream), "seam_grad_norm_f32")
                    _native.check(lib.seam_sgd_step_clip_f32(C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()), n_chunks, C.byref(groups),
                                                             None if fp is None else C.c_void_p(fp[0].data_ptr()),
                                                             C.c_void_p(rec.data_ptr()), int(self.skip_nonfinite),
                                                             C.c_void_p(pend_in.data_ptr()), C.c_void_p(pend_out.data_ptr()), stream),
                                  "seam_sgd_step_clip_f32")
                    self._pin = 1 - self._pin
                else:
                    _native.check(lib.seam_sgd_step_f32(C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()), n_chunks, C.byref(groups),
                                                        None if fp is None else C.c_void_p(fp[0].data_ptr()), stream), "seam_sgd_step_f32")
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
        for t, (pp, gp, bp, n, group, slot) in zip(tensors, key):
            t.p, t.g, t.buf, t.numel, t.group, t.slot = pp or None, gp, bp or None, n, group, slot
        crows = ops.sgd_chunk_table([k[3] for k in key], chunk)
        chunks = (_native.SgdChunk * len(crows))()
        for c, (ti, cnt, off) in zip(chunks, crows):
            c.tensor, c.count, c.offset = ti, cnt, off
        return ops._upload(tensors, device), ops._upload(chunks, device), len(crows)


def _check_norm_type(norm_type) -> float:
    norm_type = float(norm_type)
    if norm_type != 2.0 and not (math.isinf(norm_type) and norm_type > 0):
        raise ValueError(f"norm_type {norm_type} is not supported: the device norm is 2 or inf")
    return norm_type


_CLIP_TABLES = {}        # device -> (key, tensor table, chunk table, chunk count, workspace) of the last clip_grad_norm_ call
_REC_WORDS = C.sizeof(_native.ClipRecord) // 4
_REC_DTYPES = {C.c_float: torch.float32, C.c_int: torch.int32, C.c_uint64: torch.int64}


def _rec_field(rec, name):
    """field ``name`` of a device ``seam_clip_record_t`` held as int32 words: a 0-d view, placed by ``_native.ClipRecord``"""
    f = getattr(_native.ClipRecord, name)
    ctype = dict(_native.ClipRecord._fields_)[name]
    return rec[f.offset // 4:(f.offset + f.size) // 4].view(_REC_DTYPES[ctype]).reshape(())


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False, foreach=None):
    """``torch.nn.utils.clip_grad_norm_`` in two launches: ``seam_grad_norm_f32`` over every gradient, then ``seam_grad_scale_f32``,
    ``g *= min(1, max_norm / (total_norm + 1e-6))`` in place with the coefficient read on the device.  Returns the 0-d fp32 device
    ``total_norm``.  ``error_if_nonfinite=True`` raises torch's ``RuntimeError`` before anything is scaled and is the only option
    that waits for the device; ``foreach`` is accepted and ignored.  Parameters must be dense fp32 on the HIP device with contiguous
    gradients (a gradient is scaled where it lies); ``norm_type`` is 2 or inf.  No parameter with a gradient: a zero, as torch.

    The device tables and the norm's workspace of the last call are kept per device for the life of the process and reused while
    the gradients stay where they are (the training loop's case).  Calls share them, so the function is for one stream per device
    at a time: two calls in flight on different streams of one device would write the same workspace."""
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    max_norm = float(max_norm)
    norm_type = _check_norm_type(norm_type)
    rows, device = [], None
    for i, p in enumerate(parameters):
        g = p.grad
        if g is None:
            continue
        name = f"parameter {i} (shape {tuple(p.shape)})"
        if p.is_sparse or p.layout != torch.strided or g.is_sparse or g.layout != torch.strided:
            raise TypeError(f"clip_grad_norm_: {name} or its gradient is sparse: only dense fp32 is supported")
        if not p.is_cuda or not g.is_cuda:
            raise _native.SeamNativeError(f"clip_grad_norm_: {name} is not on the HIP device (no CPU path exists)")
        if p.dtype != torch.float32 or g.dtype != torch.float32:
            raise TypeError(f"clip_grad_norm_: {name} is {p.dtype} with a {g.dtype} gradient: only float32 is supported")
        if not g.is_contiguous():
            raise ValueError(f"clip_grad_norm_: the gradient of {name} is not contiguous")
        if device is None:
            device = g.device
        elif g.device != device:
            raise ValueError(f"clip_grad_norm_: {name} is on {g.device}, other parameters on {device}")
        if g.numel():
            rows.append(g)
    if device is None:
        return torch.tensor(0.0)
    lib = _native.lib()
    key = tuple((0, g.data_ptr(), 0, g.numel(), 0, 0) for g in rows)
    with torch.cuda.device(device):
        cached = _CLIP_TABLES.get(device)
        if cached is None or cached[0] != key:
            tt, ct, n_chunks = SGD._build_tables(lib, key, device) if key else (None, None, 0)
            ws = torch.empty(int(lib.seam_grad_norm_workspace_bytes(n_chunks)) // 8, dtype=torch.float64, device=device)
            cached = _CLIP_TABLES[device] = (key, tt, ct, n_chunks, ws)
        _, tt, ct, n_chunks, ws = cached
        rec = torch.empty(_REC_WORDS, dtype=torch.int32, device=device)         # a record of this call's own: the norm writes every field
        tp, cp = (None, None) if tt is None else (C.c_void_p(tt.data_ptr()), C.c_void_p(ct.data_ptr()))
        stream = torch.cuda.current_stream().cuda_stream
        _native.check(lib.seam_grad_norm_f32(tp, cp, n_chunks, int(math.isinf(norm_type)), 1, max_norm, 0, C.c_void_p(ws.data_ptr()),
                                             ws.numel() * 8, C.c_void_p(rec.data_ptr()), stream), "seam_grad_norm_f32")
        total = _rec_field(rec, "total_norm")
        if error_if_nonfinite and not bool(_rec_field(rec, "finite").item()):
            raise RuntimeError(f"The total norm of order {norm_type} for gradients from `parameters` is non-finite, so it cannot be "
                               "clipped. To disable this error and scale the gradients by the non-finite norm anyway, set "
                               "`error_if_nonfinite=False`")
        _native.check(lib.seam_grad_scale_f32(tp, cp, n_chunks, C.c_void_p(rec.data_ptr()), stream), "seam_grad_scale_f32")
    return total
