"""Host side of conv1x1_sxpc_dual (csrc/seam_pwsx.hip): the exported entries, the eligibility rule, the launch's own refusals (they
are decided before anything touches the device, so null pointers and no GPU do here) and the Python twin of its geometry rule."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("seam_conv1x1_sxpc_dual_supported", "seam_conv1x1_sxpc_dual")


def test_header_exports_and_signatures_agree_for_the_new_entries():
    from seam_match_rcnn_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seam_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(seam_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared and name in _native.SIGNATURES and hasattr(_native.lib(), name)
    # the launch entry takes what seam_conv2d_dual_f32 takes
    assert _native.SIGNATURES["seam_conv1x1_sxpc_dual"] == _native.SIGNATURES["seam_conv2d_dual_f32"]


@pytest.mark.parametrize("m,c1,c2,k,ok", [
    (1, 64, 192, 128, 1), (1, 192, 64, 128, 1), (400000, 128, 256, 512, 1), (50000, 512, 1024, 2048, 1), (37, 256, 64, 384, 1),
    (1, 32, 256, 128, 0), (1, 256, 32, 128, 0), (1, 64, 128, 128, 0), (1, 96, 160, 128, 0), (1, 0, 256, 128, 0), (1, 256, 0, 128, 0),
    (1, 64, 192, 96, 0), (1, 64, 192, 64, 0), (0, 64, 192, 128, 0), (-3, 64, 192, 128, 0), (1 << 31, 64, 192, 128, 0)])
def test_supported_rule(m, c1, c2, k, ok):
    from seam_match_rcnn_amd import _native
    lib = _native.lib()
    assert lib.seam_conv1x1_sxpc_dual_supported(m, c1, c2, k) == ok
    if ok:      # the plain kernel's rule for the concatenated reduction
        assert lib.seam_conv1x1_sxpc_supported(m, c1 + c2, k) == 1


def launch(n, ho, wo, c1, h2, w2, c2, s, k, relu, x2=1):
    """the launch entry with pointers nobody follows: every call here is refused on the host"""
    from seam_match_rcnn_amd import _native
    return _native.lib().seam_conv1x1_sxpc_dual(None, x2 or None, None, None, None, None, n, ho, wo, c1, h2, w2, c2, s, k, relu, None)


@pytest.mark.parametrize("args", [
    (2, 5, 7, 32, 10, 13, 256, 2, 128, 0),           # C1 = 32
    (2, 5, 7, 64, 10, 13, 128, 2, 128, 0),           # C1 + C2 = 192
    (2, 5, 7, 64, 10, 13, 192, 2, 96, 0),            # K = 96
    (2, 5, 7, 64, 8, 13, 192, 2, 128, 0),            # (Ho - 1) s >= H2
    (2, 5, 7, 64, 10, 12, 192, 2, 128, 0),           # (Wo - 1) s >= W2
    (2, 5, 7, 64, 10, 13, 192, 0, 128, 0),           # stride2 = 0
    (2, 5, 7, 64, 10, 13, 192, 2, 128, 2),           # relu 0 | 1
    (0, 5, 7, 64, 10, 13, 192, 2, 128, 0),           # M = 0
    (2, 0, 7, 64, 10, 13, 192, 2, 128, 0),
    (2, 5, 7, 64, 0, 13, 192, 2, 128, 0),
    (2, 8, 8, 64, 724, 724, 1024, 2, 128, 0),        # two images of 2.1 GB under one tile: past the descriptor
    (1, 8, 8, 64, 1024, 1024, 1024, 2, 128, 0),      # one image of 4 GiB
    (70000, 200, 200, 64, 200, 200, 192, 1, 128, 0), # M >= 2^31
])
def test_the_launch_refuses_on_the_host(args):
    assert launch(*args) != 0


def test_a_null_second_source_is_refused():
    assert launch(2, 5, 7, 64, 10, 13, 192, 2, 128, 0, x2=0) != 0


@pytest.mark.parametrize("n,ho,wo,h2,w2,c2,ok", [
    (80, 100, 100, 200, 200, 256, True), (80, 25, 25, 50, 50, 1024, True), (18, 125, 125, 250, 250, 1024, True),
    (1, 8, 8, 724, 724, 1024, True),                 # one image just under 2 GiB, alone
    (2, 8, 8, 724, 724, 1024, False), (1, 8, 8, 1024, 1024, 1024, False),
    (200, 1, 1, 2048, 2048, 64, False),              # 128 images of 1 GiB under one tile
    (200, 1, 1, 16, 16, 2048, True),
])
def test_the_python_twin_of_the_geometry_rule(n, ho, wo, h2, w2, c2, ok):
    """ops._sxpc_dual_map_ok decides, without a launch, what sxpc_dual_plan decides about the map; what it turns away the entry
    refuses too (the accepted maps are launched by tests/test_gpu_sxpc_dual.py)."""
    from seam_match_rcnn_amd import ops
    assert ops._sxpc_dual_map_ok(n, ho, wo, h2, w2, c2) == ok
    if not ok:
        assert launch(n, ho, wo, 192, h2, w2, c2, 1, 128, 0) != 0


def test_split_class_and_rule_are_geometry_only():
    from seam_match_rcnn_amd.models import detection as det
    assert "c3ds" in det.SPLIT_CLASSES and det.SPLIT_C3DS_MIN_C == 384
    body = det.ResNet50Body()
    served = [(li, bi) for li, bi, b in body.blocks()
              if b.downsample is not None and b.conv3.in_channels + b.downsample[0].in_channels >= det.SPLIT_C3DS_MIN_C]
    assert served == [(2, 0), (3, 0), (4, 0)]
