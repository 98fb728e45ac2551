"""Host side of the pack cache (models/packed.py ``PackedWeights``) and of the split-twin rule (models/detection.py
``split_twin``): hits and misses of ``packed()`` on a toy module, the two-part key, copies, the keys of the real modules (built on
the CPU: ``_pack_key`` launches nothing) and the rule's truth table against the expressions it replaced."""
import copy
import itertools

import pytest
import torch
from torch import nn

from seam_match_rcnn_amd.models.packed import PackedWeights


class Toy(PackedWeights, nn.Module):
    def __init__(self):
        super().__init__()
        self.a = nn.Linear(3, 2)
        self.b = nn.Linear(2, 2, bias=False)
        self.knob = 0
        self.builds = 0

    def _pack_switches(self):
        return super()._pack_switches() + (self.knob,)

    def _build_packs(self):
        assert not torch.is_grad_enabled()
        self.builds += 1
        return {"sum": self.a.weight.sum() + self.b.weight.sum(), "ptr": self.a.weight.data_ptr()}


def test_a_second_packed_is_a_hit():
    m = Toy()
    first = m.packed()
    assert m.packed() is first and m.packed() is first and m.builds == 1
    assert m._pk is first and m._pk_key == m._pack_key()


def edits():
    def in_place(m):
        with torch.no_grad():
            m.b.weight.add_(1)

    def storage(m):
        m.a.bias.data = m.a.bias.data.clone()

    def dtype(m):
        m.compute_dtype = torch.float16

    def switch(m):
        m.knob = 1

    def drop(m):
        m._pk = None
    return [in_place, storage, dtype, switch, drop]


@pytest.mark.parametrize("edit", edits(), ids=lambda f: f.__name__)
def test_each_edit_misses_exactly_once(edit):
    m = Toy()
    first = m.packed()
    edit(m)
    second = m.packed()
    assert second is not first and m.builds == 2
    assert m.packed() is second and m.builds == 2


def test_the_key_is_a_pair_of_tensors_and_switches():
    m = Toy()
    key = m._pack_key()
    assert isinstance(key, tuple) and len(key) == 2
    tensors, switches = key
    assert len(tensors) == len(m._pack_tensors()) == 3
    assert tensors == tuple((t.data_ptr(), t._version) for t in m._pack_tensors())
    assert switches == (torch.float32, 0) and switches == tuple(m._pack_switches())
    assert PackedWeights._pack_switches(m) == (torch.float32,)
    assert [id(t) for t in PackedWeights._pack_tensors(m)] == [id(p) for p in m.parameters()]


def test_a_copy_builds_against_its_own_tensors():
    m = Toy()
    m.packed()
    c = copy.deepcopy(m)
    assert c.builds == 1
    mine = c.packed()
    assert c.builds == 2 and mine["ptr"] == c.a.weight.data_ptr() != m.a.weight.data_ptr()
    with torch.no_grad():
        m.a.weight.add_(1)
    assert c.packed() is mine and c.builds == 2
    assert m.packed()["ptr"] == m.a.weight.data_ptr() and m.builds == 2
    assert not any(isinstance(v, nn.Module) or callable(v) for v in (m._pk_key,) + tuple(m._pk_key[0]) + tuple(m._pk_key[1]))


# ---------------------------------------------------------------------------------------- the real modules, on the CPU
def det_and_ops():
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    return det, ops


class knobs:
    NAMES = ("SPLIT_F32", "SPLIT_DTYPE", "SPLIT_CLASSES", "FUSE_SHORTCUT", "STEM_SWH")

    def __enter__(self):
        self.det = det_and_ops()[0]
        self.saved = [getattr(self.det, n) for n in self.NAMES]
        return self.det

    def __exit__(self, *exc):
        for n, v in zip(self.NAMES, self.saved):
            setattr(self.det, n, v)
        return False


ALL = ("c1", "c2s2", "c3", "c3ds", "lat", "mdeconv")
MODULES = [("ResNet50Body", "c1"), ("ResNet50Body", "c2s2"), ("ResNet50Body", "c3"), ("ResNet50Body", "c3ds"),
           ("FeaturePyramidNetwork", "lat"), ("MaskRCNNPredictor", "mdeconv")]
_BUILT = {}


def module(name):
    """One instance per class for the whole file: only its attributes move, and every test puts them back."""
    if name not in _BUILT:
        _BUILT[name] = getattr(det_and_ops()[0], name)().eval()
    return _BUILT[name]


@pytest.mark.parametrize("name,cls", MODULES)
def test_switches_of_the_real_modules_follow_their_split_class(name, cls):
    det, ops = det_and_ops()
    with knobs():
        det.SPLIT_F32, det.SPLIT_DTYPE, det.SPLIT_CLASSES = True, ops.SX6, frozenset(ALL)
        m = module(name)
        try:
            tensors, base = m._pack_key()
            assert len(tensors) == len(m._pack_tensors()) and m._pack_key() == (tensors, base)
            det.SPLIT_CLASSES = frozenset(ALL) - {cls}
            assert m._pack_key()[1] != base and m._pack_key()[0] == tensors
            det.SPLIT_CLASSES = frozenset(ALL)
            assert m._pack_key()[1] == base
            others = frozenset(ALL) - set(getattr(m, "SPLIT_TWINS", (cls,)))       # a class of another module: not in this key
            det.SPLIT_CLASSES = frozenset(ALL) - others
            assert m._pack_key()[1] == base
            det.SPLIT_CLASSES = frozenset(ALL)
            det.set_split_f32(m, False)
            assert m._pack_key()[1] != base
            det.set_split_f32(m, True)
            assert m._pack_key()[1] == base
            det.set_compute_dtype(m, torch.float16)
            assert m._pack_key()[1] != base
            det.set_compute_dtype(m, torch.float32)
            assert m._pack_key() == (tensors, base)
            m.train()                                                             # run-time state is split_on's, not the key's
            assert m._pack_key() == (tensors, base)
        finally:
            m.eval()
            det.set_split_f32(m, True)
            det.set_compute_dtype(m, torch.float32)


def test_the_body_key_holds_every_knob_its_build_reads():
    det, ops = det_and_ops()
    with knobs():
        det.SPLIT_F32, det.SPLIT_DTYPE, det.SPLIT_CLASSES = True, ops.SX6, frozenset(ALL)
        body = module("ResNet50Body")
        tensors, base = body._pack_key()
        assert len(tensors) == len(list(body.parameters())) + len(list(body.buffers())) == 53 + 4 * 53
        assert sorted(map(id, body._pack_tensors())) == sorted(map(id, list(body.parameters()) + list(body.buffers())))
        for name, other in (("SPLIT_DTYPE", ops.SX9), ("FUSE_SHORTCUT", not det.FUSE_SHORTCUT), ("STEM_SWH", not det.STEM_SWH),
                            ("SPLIT_F32", False)):
            was = getattr(det, name)
            setattr(det, name, other)
            assert body._pack_key()[1] != base, name
            setattr(det, name, was)
            assert body._pack_key() == (tensors, base), name


def old_predicates(det, ops, m):
    """The expressions ``split_twin`` replaced, written out: the body's ``sx`` with its per-class tests, the FPN's
    ``_split_twins``, the mask predictor's ``twin``."""
    dt = det.cdt(m)
    sx = dt == torch.float32 and det.SPLIT_F32 and getattr(m, "split_f32", True)
    return {"c1": bool(sx and "c1" in det.SPLIT_CLASSES),
            "c2s2": bool(sx and "c2s2" in det.SPLIT_CLASSES),
            "c3": bool(sx and "c3" in det.SPLIT_CLASSES),
            "c3ds": bool(sx and "c3ds" in det.SPLIT_CLASSES and det.SPLIT_DTYPE == ops.SX6),
            "lat": bool(det.cdt(m) == torch.float32 and det.SPLIT_F32 and getattr(m, "split_f32", True)
                        and "lat" in det.SPLIT_CLASSES and det.SPLIT_DTYPE == ops.SX6),
            "mdeconv": bool(dt == torch.float32 and det.SPLIT_F32 and getattr(m, "split_f32", True)
                            and "mdeconv" in det.SPLIT_CLASSES and det.SPLIT_DTYPE == ops.SX6)}


def test_split_twin_truth_table():
    det, ops = det_and_ops()
    m = nn.Identity()
    seen = set()
    with knobs():
        for cls, dt, glob, own, terms, inside in itertools.product(ALL, (torch.float32, torch.float16), (True, False), (True, False),
                                                                   (ops.SX6, ops.SX9), (True, False)):
            m.compute_dtype, m.split_f32 = dt, own
            det.SPLIT_F32, det.SPLIT_DTYPE = glob, terms
            det.SPLIT_CLASSES = frozenset(ALL) if inside else frozenset(ALL) - {cls}
            got = det.split_twin(m, cls)
            assert got is old_predicates(det, ops, m)[cls], (cls, dt, glob, own, terms, inside)
            seen.add(got)
    assert seen == {True, False}
    del m.split_f32                          # the attribute's default is on
    m.compute_dtype = torch.float32
    assert det.split_twin(m, "c1") is bool(det.SPLIT_F32 and "c1" in det.SPLIT_CLASSES)


def test_pick_pack():
    det, _ = det_and_ops()
    m = nn.Identity().eval()
    with knobs():
        det.SPLIT_F32 = True
        with torch.no_grad():
            assert det.split_on(m)
            assert det.pick_pack(m, "exact", "twin") == "twin" and det.pick_pack(m, "exact", None) == "exact"
            assert det.pick_pack(m, "exact") == "exact"
            m.train()
            assert det.pick_pack(m, "exact", "twin") == "exact"
            m.eval()
        assert det.pick_pack(m, "exact", "twin") == "exact"                      # a gradient tape: the exact pack
        det.SPLIT_F32 = False
        with torch.no_grad():
            assert det.pick_pack(m, "exact", "twin") == "exact"
