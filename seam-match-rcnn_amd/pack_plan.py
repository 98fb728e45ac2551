"""``PackPlan``: the in-place refresh of the cached weight packs after an optimizer step.  The one module above
``ops``: it reads the pack recorder there and the pack-cache interface of ``models.packed``."""
from __future__ import annotations

from typing import Sequence

import torch

from . import _native
from ._ops_common import F32, _ptr, _stream, _upload
from .models.packed import PackedWeights
from .ops import _SX_TERMS, record_packs


class PackPlan:
    """The in-place refresh of the cached packs of ``backbone.body``, ``backbone.fpn`` and ``rpn.head`` after an optimizer step.

    Built once: every covered module repacks by its own ``packed()`` under ``record_packs``, which yields, per pack, the source (a
    parameter, or a ``derived_source``) and the destination buffers.  ``rebuilds`` counts every later build.  ``refresh(updated)``
      * checks on the host that the plan still describes the model, by the two parts of ``models.packed.PackedWeights._pack_key``
        (the same ``_pk`` objects; tensors: the same parameter / buffer pointers, versions that moved by exactly the optimizer's
        one bump and only on updated parameters; switches: equal); otherwise it drops everything and rebuilds by the modules' own
        route -- it never writes through a stale pointer;
      * recomputes the derived sources whose parameters moved (torch; counted in ``fallback_calls``);
      * rewrites every weight-dependent buffer of every pack whose source moved in ONE ``seam_repack_many_f32`` launch on the
        current stream (``launches_per_refresh``); epilogue vectors of a frozen BN and packs of frozen layers are not touched;
      * sets each module's ``_pk_key`` to what ``packed()`` now computes: the next ``packed()`` is a hit on the same tensors.
    fp32 compute only (the exact packs and their split-bf16 twins)."""

    COVERED = ("backbone.body", "backbone.fpn", "rpn.head")

    def __init__(self, model):
        self.modules = []
        for path in self.COVERED:
            m = model
            for part in path.split("."):
                m = getattr(m, part, None)
                if m is None:
                    break
            if isinstance(m, PackedWeights):
                self.modules.append((path, m))
        if not self.modules:
            raise ValueError("PackPlan: the model has none of " + ", ".join(self.COVERED))
        self.refreshes = self.rebuilds = self.table_uploads = 0
        self.launches_per_refresh = self.fallback_calls = 0
        self._built = self._ever_built = False

    # -- build
    def build(self):
        """Build the plan now (``optim.SGD`` does, when it is given the model): every covered module repacks once by its own route."""
        if not self._built:
            self._build()
        return self

    def rebuild_after_edit(self):
        """The last in-place refresh followed an edit of a parameter that no version counter showed (``optim.SGD`` found the
        parameters changed under it): treat it like any other edit -- drop the plan and rebuild by the modules' own route."""
        self.refreshes -= 1
        self._build()

    def _build(self):
        self._built = False
        self._pk, self._keys, self._entries, self._derived = [], [], [], []
        self._table_for, self._table = None, None
        for path, m in self.modules:
            m._pk_key = None
            with record_packs() as rec:
                pk = m.packed()
            params = {p.data_ptr(): p for p in m.parameters() if p.numel()}
            derived = {t.data_ptr(): (t, fn, deps) for t, fn, deps in rec.derived}
            self._derived += [d for d in rec.derived if d[2]]

            def deps_of(t, what):
                if t.data_ptr() in params:
                    return (params[t.data_ptr()],)
                if t.data_ptr() in derived:
                    return derived[t.data_ptr()][2]
                raise NotImplementedError(f"PackPlan: {path}: the {what} of a pack is neither a parameter nor a derived_source")

            for weight, bias, bn, mode, pc in rec.records:
                wdeps = deps_of(weight, "weight")
                if bias is not None:
                    if bn is not None or pc.shift is None or pc.shift.data_ptr() != bias.data_ptr():
                        raise NotImplementedError(f"PackPlan: {path}: a pack whose shift is computed from its bias is not covered")
                    deps_of(bias, "bias")           # a parameter (the shift aliases it) or a derived_source (refreshed with it)
                self._entries.append((wdeps, self._jobs_of(path, weight, mode, pc)))
            self._pk.append(pk)
            self._keys.append(m._pack_key())
        self.rebuilds += self._ever_built
        self._built = self._ever_built = True

    @staticmethod
    def _jobs_of(path, weight, mode, pc):
        N = _native

        def job(form, dst, R=1, S=1, cs=pc.Cstore, cin=pc.Cin, md=0, scale=None):
            return N.RepackJob(src=weight.data_ptr(), dst=dst.data_ptr(), scale=None if scale is None else scale.data_ptr(), form=form,
                               K=pc.K, Cin=cin, R=R, S=S, Cstore=cs, mode=md)

        if pc.dtype in _SX_TERMS:
            jobs = [job(N.REPACK_SPLIT3, pc.w, pc.R, pc.S, md=mode)]
            if pc.wx is not None:
                jobs.append(job(N.REPACK_SXPC, pc.wx))
            if pc.wxs is not None:
                jobs.append(job(N.REPACK_SXPC64, pc.wxs))
            if pc.wx64 is not None:
                jobs.append(job(N.REPACK_SXPC64, pc.wx64))
            if pc.u24x is not None:
                jobs.append(job(N.REPACK_W24SX, pc.u24x, 3, 3, md=mode))
            return jobs
        if pc.dtype != F32 or pc.wh is not None or pc.wsh is not None or pc.wph is not None:
            raise NotImplementedError(f"PackPlan: {path}: only fp32 packs are refreshed in place (pass refresh_packs=False)")
        jobs = [job(N.REPACK_IGEMM, pc.w, pc.R, pc.S, md=mode)]
        if pc.u is not None:
            jobs.append(job(N.REPACK_WINO, pc.u, 3, 3, md=mode))
        if pc.u24 is not None:
            jobs.append(job(N.REPACK_WINO24, pc.u24, 3, 3, md=mode))
        if (pc.wn is not None or pc.ws is not None or pc.wq is not None) and mode != 0:
            raise NotImplementedError(f"PackPlan: {path}: the pointwise forms of a transposed conv are not covered")
        if pc.wn is not None:
            jobs.append(job(N.REPACK_NARROW, pc.wn))
        if pc.ws is not None and pc.ws.data_ptr() != weight.data_ptr():      # (without a scale the rows ARE the weight: nothing to do)
            jobs.append(job(N.REPACK_SW, pc.ws, scale=pc.scale))
        if pc.wq is not None:
            jobs.append(job(N.REPACK_PC, pc.wq))
        return jobs

    # -- the host checks
    def _valid(self, updated) -> bool:
        for (path, m), pk, old in zip(self.modules, self._pk, self._keys):
            if m._pk is not pk:
                return False
            (old_tensors, old_switches), (new_tensors, new_switches) = old, m._pack_key()
            if new_switches != old_switches or len(new_tensors) != len(old_tensors):      # compute dtype, split twins, pack-time knobs
                return False
            for t, a, b in zip(m._pack_tensors(), old_tensors, new_tensors):
                bump = 1 if id(t) in updated else 0
                if a[0] != b[0] or a[1] + bump != b[1]:
                    return False
        return True

    @torch.no_grad()
    def refresh(self, updated: Sequence[torch.Tensor]) -> bool:
        """``updated``: the parameters the optimizer just changed, their versions bumped once.  True: refreshed in place; False:
        the plan was (re)built by the modules' own route."""
        ids = frozenset(id(p) for p in updated)
        if not self._built or not self._valid(ids):
            self._build()
            return False
        lib = _native.lib()
        calls = 0
        for t, fn, deps in self._derived:
            if any(id(d) in ids for d in deps):
                t.copy_(fn())
                calls += 1
        if self._table_for != ids:
            jobs = [j for deps, js in self._entries if any(id(d) in ids for d in deps) for j in js]
            arr = (_native.RepackJob * max(1, len(jobs)))(*jobs)
            blocks = int(lib.seam_repack_layout(arr, len(jobs)))
            if blocks < 0:
                raise _native.SeamNativeError(f"seam_repack_layout refused job {-1 - blocks}")
            dev = self.modules[0][1]._pack_tensors()[0].device
            self._table = (_upload(arr, dev) if jobs else None, len(jobs), blocks)
            self._table_for = ids
            self.table_uploads += 1
        table, n, blocks = self._table
        if n:
            _native.check(lib.seam_repack_many_f32(_ptr(table), n, blocks, _stream()), "seam_repack_many_f32")
        for i, (path, m) in enumerate(self.modules):
            m._pk_key = self._keys[i] = m._pack_key()
        self.refreshes += 1
        self.launches_per_refresh = 1 if n else 0
        self.fallback_calls = calls
        return True
