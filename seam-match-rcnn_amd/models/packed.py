"""The cache of a module's packed weights.  A module that inherits ``PackedWeights`` writes ``_build_packs()`` -- what it hands to
the kernels, built from its tensors -- and reads it through ``packed()``.  The cache key is a pair ``(tensors, switches)``:
  tensors    one ``(data_ptr, _version)`` per entry of ``_pack_tensors()``: a tensor replaced, moved or edited in place misses
  switches   ``_pack_switches()``: everything else ``_build_packs`` reads (the compute dtype, split twins, pack-time knobs)
``pack_plan.PackPlan`` reads the two parts by name.  The state is ``_pk`` / ``_pk_key`` on the module itself (``module._pk = None`` drops
the packs), so a copied or unpickled module misses and rebuilds against its own tensors."""
from __future__ import annotations

import torch


class PackedWeights:
    _pk = None          # what ``_build_packs`` returned
    _pk_key = None      # the ``_pack_key`` it was built under

    def _pack_tensors(self, *args) -> list:
        return list(self.parameters())

    def _pack_switches(self) -> tuple:
        return (getattr(self, "compute_dtype", torch.float32),)

    def _pack_key(self, *args) -> tuple:
        return tuple([(t.data_ptr(), t._version) for t in self._pack_tensors(*args)]), tuple(self._pack_switches())

    def packed(self, *args):
        key = self._pack_key(*args)
        if self._pk is None or key != self._pk_key:
            with torch.no_grad():
                pk = self._build_packs(*args)
            self._pk, self._pk_key = pk, key
        return self._pk
