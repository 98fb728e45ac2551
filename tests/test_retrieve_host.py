"""Host side of the unlabelled-video retrieval: the ProductBank container, the refusals that need no device, and the device
linker's symbols in the header and the library."""
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT
from seam_match_rcnn_amd import retrieval as R


def _bank(g, base=0.0, keys=None, missing=()):
    m = torch.arange(g * 256, dtype=torch.float32).view(g, 256) + base
    return R.ProductBank(match=m, aggr=m * 2 + 1, boxes=torch.arange(g * 4, dtype=torch.float32).view(g, 4) + base,
                         scores=torch.linspace(0.1, 0.9, g) if g else torch.zeros(0),
                         keys=list(range(g)) if keys is None else list(keys), missing=list(missing))


def _equal(a, b):
    return (torch.equal(a.match, b.match) and torch.equal(a.aggr, b.aggr) and torch.equal(a.boxes, b.boxes)
            and torch.equal(a.scores, b.scores) and a.keys == b.keys and a.missing == b.missing)


def test_product_bank_round_trip(tmp_path):
    bank = _bank(5, keys=["a", "b", 7, "d", "e"], missing=["x"])
    path = str(tmp_path / "bank.pt")
    bank.save(path)
    back = R.ProductBank.load(path)
    assert _equal(bank, back) and len(back) == 5
    assert not back.match.is_cuda and back.match.dtype == torch.float32
    assert _equal(R.ProductBank.load(path, "cpu"), bank)
    torch.save({"something": 1}, path)
    with pytest.raises(ValueError):
        R.ProductBank.load(path)


def test_product_bank_extend():
    a, b = _bank(2, keys=["p", "q"], missing=["m0"]), _bank(3, base=1000.0, keys=["r", "s", "t"], missing=["m1"])
    a0 = _bank(2, keys=["p", "q"], missing=["m0"])
    assert a.extend(b) is a
    assert len(a) == 5 and a.keys == ["p", "q", "r", "s", "t"] and a.missing == ["m0", "m1"]
    for name in ("match", "aggr", "boxes", "scores"):
        assert torch.equal(getattr(a, name), torch.cat([getattr(a0, name), getattr(b, name)]))
    assert len(b) == 3 and b.keys == ["r", "s", "t"]            # the argument is left alone
    empty = _bank(0)
    assert len(empty.extend(b)) == 3 and torch.equal(empty.match, b.match)


def test_retrieve_refusals_need_no_device():
    """Refused before the model or the device is touched (the model here is None)."""
    from seam_match_rcnn_amd import _native
    with pytest.raises(ValueError, match="unknown strategy"):
        R.retrieve(None, [], _bank(3), strategy="max_dist")
    with pytest.raises(ValueError, match="empty"):
        R.retrieve(None, [], _bank(0))
    cap = int(_native.lib().seam_rank_topk_max_k())
    with pytest.raises(ValueError, match=rf"k = {cap + 1} exceeds the top-k capacity of {cap}"):
        R.retrieve(None, [], _bank(cap + 1), k=cap + 1)
    with pytest.raises(ValueError, match="one key per image"):
        R.build_bank(None, [torch.zeros(3, 8, 8)], keys=[1, 2])


def test_linker_symbols_in_header_and_library():
    from seam_match_rcnn_amd import _native
    header = open(os.path.join(ROOT, "include", "seam_hip.h")).read()
    out = subprocess.run(["nm", "-D", "--defined-only", _native.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (seam_[a-z0-9_]+)", out))
    for name in ("seam_build_tracklets_f32", "seam_build_tracklets_max_rows"):
        assert re.search(rf"\b{name}\s*\(", header), name
        assert name in exported and name in _native.SIGNATURES
    lib = _native.lib()
    assert lib.seam_build_tracklets_max_rows() >= 1024
    # refused or a no-op before anything is launched: no device is needed for these
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, 0, 0, 0.3, None, None, None, None, None) == 0
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, -1, 0, 0.3, None, None, None, None, None) != 0
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, 1, lib.seam_build_tracklets_max_rows() + 1, 0.3,
                                        None, None, None, None, None) != 0
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, 1, 1, 0.3, None, None, None, None, None) != 0
