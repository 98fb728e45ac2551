"""Host side of conv1x1_sxpc_up (csrc/seam_pwsx.hip): the exported entries, the eligibility predicate over the shapes of
tests/test_gpu_sxpc_up.py, the launch's own refusals (decided before anything touches the device, so null pointers and no GPU do
here), the default split classes and the integers-only rule of ``ops.conv2d_topdown``."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("seam_conv1x1_sxpc_up_supported", "seam_conv1x1_sxpc_up")


def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def test_header_exports_and_signatures_agree_for_the_new_entries():
    from seam_match_rcnn_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seam_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(seam_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared and name in _native.SIGNATURES and hasattr(_native.lib(), name)


# (N, Ho, Wo, C, K, rH, rW, served)
TABLE = [
    (1, 16, 16, 256, 128, 8, 8, 1), (3, 5, 7, 320, 256, 3, 4, 1), (2, 25, 25, 256, 128, 13, 13, 1), (1, 13, 9, 256, 128, 5, 4, 1),
    (300, 1, 1, 256, 128, 1, 1, 1),                 # 1 x 1 maps are served
    (130, 3, 1, 256, 128, 2, 1, 1),                 # Wo == 1 is served
    (1, 43, 3, 256, 384, 22, 2, 1), (4, 100, 100, 256, 256, 50, 50, 1),
    (80, 200, 200, 256, 256, 100, 100, 1), (80, 100, 100, 512, 256, 50, 50, 1), (80, 50, 50, 1024, 256, 25, 25, 1),     # a step's three laterals
    (2, 5, 7, 192, 128, 3, 4, 0), (2, 5, 7, 256, 192, 3, 4, 0), (2, 5, 7, 288, 128, 3, 4, 0),
    (2, 5, 7, 256, 128, 0, 4, 0), (2, 5, 7, 256, 128, 3, 0, 0), (0, 5, 7, 256, 128, 3, 4, 0), (2, 0, 7, 256, 128, 3, 4, 0),
    (3, 8, 8, 256, 128, 1200, 1200, 0),             # three coarse images of 2.2 GB under one tile
    (1, 8, 8, 256, 128, 2048, 2048, 0),             # one coarse image of 2 GiB
    (2, 8, 8, 256, 128, 1200, 1200, 1),             # ... two of 0.7 GB: inside the descriptor
    (70000, 200, 200, 256, 128, 100, 100, 0),       # M >= 2^31
]


@pytest.mark.parametrize("n,ho,wo,c,k,rh,rw,ok", TABLE)
def test_supported_table(n, ho, wo, c, k, rh, rw, ok):
    l = lib()
    assert l.seam_conv1x1_sxpc_up_supported(n * ho * wo, n, ho, wo, c, k, rh, rw) == ok
    if ok:      # the plain kernel's rule for the same rows; and M must be the grid's
        assert l.seam_conv1x1_sxpc_supported(n * ho * wo, c, k) == 1
        assert l.seam_conv1x1_sxpc_up_supported(n * ho * wo + 1, n, ho, wo, c, k, rh, rw) == 0
        assert l.seam_conv1x1_sxpc_up_supported(n * ho * wo - 1, n, ho, wo, c, k, rh, rw) == 0
    else:       # what the predicate turns away the launch refuses on the host (pointers nobody follows)
        assert l.seam_conv1x1_sxpc_up(None, None, None, None, 1, None, n, ho, wo, c, k, rh, rw, 0, None) != 0


def test_the_launch_refuses_a_null_top_and_a_bad_relu():
    l = lib()
    assert l.seam_conv1x1_sxpc_up(None, None, None, None, None, None, 2, 5, 7, 256, 128, 3, 4, 0, None) != 0
    assert l.seam_conv1x1_sxpc_up(None, None, None, None, 1, None, 2, 5, 7, 256, 128, 3, 4, 2, None) != 0


def test_default_split_classes():
    from seam_match_rcnn_amd.models import detection as det
    if "SEAM_SPLIT_CLASSES" not in os.environ:
        assert {"c1", "c3", "c2s2", "c3ds", "lat", "mdeconv"} <= det.SPLIT_CLASSES
    src = open(os.path.join(ROOT, "seam-match-rcnn_amd", "models", "detection.py")).read()
    default = re.search(r'"SEAM_SPLIT_CLASSES",\s*"([^"]*)"', src).group(1).split(",")
    assert "lat" in default and "mdeconv" in default


def test_conv2d_topdown_chooses_by_integers_only():
    """ops._sxpc_up_ok: the pack's integers, the launch's integers, the knobs -- the pack's tensors are placeholders here"""
    from seam_match_rcnn_amd import ops
    T = object()
    pc = ops.PackedConv(T, None, None, 256, 512, 1, 1, Cin=512, dtype=ops.SX6, wx=T)
    saved = (ops.SXPC, ops.SXPC_RULE, ops.SXPC_MIN_TILES)
    try:
        ops.SXPC, ops.SXPC_RULE, ops.SXPC_MIN_TILES = True, True, 196
        ok = lambda n, h=100, w=100, c=512, tn=None, th=50, tw=50, tk=256: ops._sxpc_up_ok(lib(), pc, n, h, w, c, n if tn is None else tn, th, tw, tk)
        assert ok(80) and ok(2)                     # 2 x 100 x 100 rows: 157 x 2 tiles
        assert not ok(1)                            # 79 x 2 = 158 tiles: below SXPC_MIN_TILES -- conv2d + upsample_add_, the same bits
        assert ok(1, 112, 112)                      # 98 x 2 = 196 tiles: at the threshold
        assert not ok(80, c=256) and not ok(80, tn=79) and not ok(80, tk=128) and not ok(80, th=0)
        ops.SXPC_RULE = False
        assert ok(1) and ok(1, 1, 1, th=1, tw=1)
        ops.SXPC = False
        assert not ok(80)
    finally:
        ops.SXPC, ops.SXPC_RULE, ops.SXPC_MIN_TILES = saved
