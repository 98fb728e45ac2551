"""GPU: the n-tile split of conv3x3_wino24sx over XCD groups (forced with
``seam_conv3x3_wino24sx_set_nsplit``, csrc/seam_wino24sx.hip; the decode is w24_tile in
csrc/seam_wino24_common.h).  The split only renumbers the blocks, so for every forced value the output through the C ABI is the
output of nsplit = 1 byte for byte, and that one passes the float64 gates of tests/test_gpu_w24sx.py.  Outputs are NaN-filled between
0x5A guard zones (that file's ``Out``): a tile no block covers stays NaN, a stray store shows in the guards.

Shapes: the smallest that reach each branch of the decode (C = 64 is four k-steps).  With `parts` = 8 / nsplit partitions of the
patch blocks, part_q = blocks // parts and part_r = blocks % parts:
  * 1 x 8 x 8, 64 -> 256, pad 1: one patch block, four n-tiles; part_q = 0, so all but one partition are padding blocks that return.
  * 3 x 20 x 36, 64 -> 128, pad 1: one uniform region (TX 3, TY 10) of three blocks per image; two n-tiles, so a forced 4 is
    reduced to 2.
  * 1 x 25 x 70, 128 -> 128, pad 1 (``r3-9-3-rt-100sq-c128`` of tests/w24_layout_cases.py, the layout of the 100 x 100 maps): a main
    region plus a right and a bottom strip, eight patch blocks whose region decode follows the split's renumbering.
  * 5 x 14 x 14, 64 -> 256, pad 0: stacked mode, 3 patch blocks over 4 and over 2 partitions.
  * 2 x 40 x 40, 128 -> 256, pad 1, residual + ReLU: part_r != 0 with part_q > 0.
  * 2 x 9 x 11, 64 -> 64: one n-tile, every forced value falls back to 1."""
import pytest
import torch
import torch.nn.functional as F

import test_gpu_w24sx as W
import w24_layout_cases as T

pytestmark = pytest.mark.gpu

FORCED = (1, 2, 4)

CASES = [
    pytest.param((1, 8, 8, 64, 256, 1, ""), id="one-patch-block-1x8x8-64-256"),
    pytest.param((3, 20, 36, 64, 128, 1, ""), id="regions-3x20x36-64-128"),
    pytest.param(tuple(T.BY_ID["r3-9-3-rt-100sq-c128"][1:7]) + ("",), id="three-regions-1x25x70-128-128"),
    pytest.param((5, 14, 14, 64, 256, 0, ""), id="stacked-5x14x14-64-256-pad0"),
    pytest.param((2, 40, 40, 128, 256, 1, "residual_relu"), id="part_r-2x40x40-128-256-residual-relu"),
    pytest.param((2, 9, 11, 64, 64, 1, ""), id="one-n-tile-2x9x11-64-64"),
]


@pytest.fixture(scope="module")
def env():
    import seam_match_rcnn_amd.ops as ops
    from seam_match_rcnn_amd import _native
    return ops, _native.lib(), torch.device("cuda:0")


@pytest.mark.parametrize("case", CASES)
def test_forced_split_is_bit_identical(env, case):
    ops, lib, dev = env
    n, h, w, c, k, pad, mode = case
    if (n, h, w) == (1, 25, 70):          # the case this file names as main region + both strips really is one
        assert T.signature(T.query(lib, n, h, w, c, k, pad), n, h, w, pad)["strips"] == "RB"
    p = W.problem(env, n, h, w, c, k, pad)
    ref, y24, yex, resd, relu = p["y64"], p["y24"], p["yex"], None, 0
    if mode:
        res = W.rnd(75, tuple(p["y64"].shape), "res")
        resd, relu = res.to(dev), 1
        ref = F.relu(p["y64"] + res.double())
        y24d = torch.empty(tuple(ref.shape), dtype=torch.float32, device=dev)
        yexd = torch.empty_like(y24d)
        assert lib.seam_conv3x3_wino24_f32(W.ptr(p["x"]), W.ptr(W.pack_w24(lib, p["w"], dev)), None, None, W.ptr(resd), W.ptr(y24d),
                                           n, h, w, c, k, pad, relu, None) == 0
        pc = ops.pack_conv(p["w"], None, stride=1, pad=pad)
        assert lib.seam_conv2d_f32(W.ptr(p["x"]), W.ptr(pc.w), None, None, W.ptr(resd), W.ptr(yexd), n, h, w, c, k, 3, 3, 1, pad, relu,
                                   None) == 0
        torch.cuda.synchronize()
        y24, yex = y24d.cpu(), yexd.cpu()
    before = lib.seam_conv3x3_wino24sx_get_nsplit()
    outs, blocks = {}, {}
    try:
        for ns in FORCED:
            assert lib.seam_conv3x3_wino24sx_set_nsplit(ns) == 0
            blocks[ns] = lib.seam_conv3x3_wino24sx_blocks(n, h, w, c, k, pad)
            outs[ns] = W.run_sx(lib, dev, p["x"], p["u"], None, None, resd, k, pad, relu).cpu()
    finally:
        lib.seam_conv3x3_wino24sx_set_nsplit(before)
    assert blocks[1] > 0 and blocks[2] == blocks[1] and blocks[4] == blocks[1], blocks
    W.gates(f"{case} nsplit 1", outs[1], ref, y24, yex)
    for ns in FORCED[1:]:
        assert not bool(torch.isnan(outs[ns]).any()), f"nsplit {ns}: a tile was not written"
        assert torch.equal(outs[ns].view(torch.int32), outs[1].view(torch.int32)), f"nsplit {ns} differs from nsplit 1"


def test_rule_gives_the_bits_of_forced_one(env):
    """The default (0 = the rule, whatever it picks) against forced 1 on 2 x 40 x 40, 256 -> 256, the channel counts of the routed layers."""
    _, lib, dev = env
    p = W.problem(env, 2, 40, 40, 256, 256, 1)
    before = lib.seam_conv3x3_wino24sx_get_nsplit()
    try:
        assert lib.seam_conv3x3_wino24sx_set_nsplit(0) == 0
        y0 = W.run_sx(lib, dev, p["x"], p["u"], None, None, None, 256, 1, 0).cpu()
        assert lib.seam_conv3x3_wino24sx_set_nsplit(1) == 0
        y1 = W.run_sx(lib, dev, p["x"], p["u"], None, None, None, 256, 1, 0).cpu()
    finally:
        lib.seam_conv3x3_wino24sx_set_nsplit(before)
    W.gates("2x40x40 256->256 nsplit 1", y1, p["y64"], p["y24"], p["yex"])
    assert torch.equal(y0.view(torch.int32), y1.view(torch.int32))
