"""Host side of conv1x1_sxpc (csrc/seam_pwsx.hip): the exported entries, the eligibility and size rules, and the repack table's
checks for the SEAM_REPACK_SXPC form.  No GPU: every call here runs on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("seam_conv1x1_sxpc_supported", "seam_conv1x1_sxpc_weight_bytes", "seam_pack_conv1x1_weight_sxpc", "seam_conv1x1_sxpc")


def test_header_exports_and_signatures_agree_for_the_new_entries():
    from seam_match_rcnn_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seam_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(seam_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared and name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert sorted(_native.SIGNATURES) == sorted(declared)
    # the launch entry takes what seam_conv1x1_pc_f32 takes; the pack entry what seam_pack_conv1x1_weight_f16pc takes
    assert _native.SIGNATURES["seam_conv1x1_sxpc"] == _native.SIGNATURES["seam_conv1x1_pc_f32"]
    assert _native.SIGNATURES["seam_pack_conv1x1_weight_sxpc"] == _native.SIGNATURES["seam_pack_conv1x1_weight_f16pc"]
    assert re.search(r"SEAM_REPACK_SXPC\s*=\s*%d\b" % _native.REPACK_SXPC, txt)


@pytest.mark.parametrize("m,c,k,ok", [
    (1, 256, 128, 1), (37, 256, 384, 1), (1 << 20, 2048, 512, 1), (100000, 320, 1024, 1), (5, 1024, 2048, 1),
    (1, 64, 128, 0), (1, 192, 128, 0), (1, 288, 128, 0), (1, 256, 96, 0), (1, 256, 64, 0), (0, 256, 128, 0), (-3, 256, 128, 0),
    (1 << 31, 256, 128, 0)])
def test_supported_rule(m, c, k, ok):
    from seam_match_rcnn_amd import _native
    assert _native.lib().seam_conv1x1_sxpc_supported(m, c, k) == ok


def test_weight_bytes_are_three_bf16_planes():
    from seam_match_rcnn_amd import _native
    lib = _native.lib()
    for k, c in ((128, 256), (512, 2048), (1024, 320)):
        assert lib.seam_conv1x1_sxpc_weight_bytes(k, c) == 6 * k * c


def test_repack_layout_takes_and_refuses_the_new_form_by_the_per_layer_rules():
    from seam_match_rcnn_amd import _native
    lib = _native.lib()

    def job(**kw):
        d = dict(src=0x10000, dst=0x20000, scale=None, form=_native.REPACK_SXPC, K=256, Cin=512, R=1, S=1, Cstore=512, mode=0)
        d.update(kw)
        return _native.RepackJob(**d)

    arr = (_native.RepackJob * 1)(job())
    blocks = lib.seam_repack_layout(arr, 1)
    assert blocks > 0 and arr[0].items == 256 * 512 // 8 and arr[0].first_block == 0 and arr[0].n_blocks == blocks
    for bad in (job(K=96), job(Cin=64, Cstore=64), job(Cin=288, Cstore=288), job(R=3, S=3), job(mode=2), job(Cin=500), job(src=None),
                job(dst=None)):
        arr = (_native.RepackJob * 2)(job(), bad)
        assert lib.seam_repack_layout(arr, 2) == -2
    assert C.sizeof(_native.RepackJob) == 80
