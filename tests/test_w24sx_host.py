"""CPU: the host side of conv3x3_wino24sx -- the route's precedence and its geometry-only rule (``ops._conv_route`` /
``ops.w24sx_map_ok``), the knobs that restore the fp32 routes, the weight-bytes function and the class plumbing through
``split_twin``.  Packs carry sentinels where the tensors would be.  No GPU."""
import pytest

T = object()        # stands for a packed tensor: any use of it as one raises


@pytest.fixture()
def ops():
    import seam_match_rcnn_amd.ops as ops
    names = ("W24SX", "W24SX_MIN_C", "W24SX_MIN_BLOCKS", "WINOGRAD", "WINOGRAD24", "WINO_MIN_FILL", "WINO24_MARGIN")
    saved = {k: getattr(ops, k) for k in names}
    caches = dict(ops._WINO24), dict(ops._WINO_FILL)
    ops.W24SX, ops.W24SX_MIN_C, ops.WINOGRAD, ops.WINOGRAD24, ops.WINO_MIN_FILL, ops.WINO24_MARGIN = True, 128, True, 1, 55, 0.95
    ops.W24SX_MIN_BLOCKS = 0          # the precedence cases run on every map the other rules admit; the block rule has its own test
    ops._WINO24.clear()
    yield ops
    for k, v in saved.items():
        setattr(ops, k, v)
    for cache, old in zip((ops._WINO24, ops._WINO_FILL), caches):
        cache.clear()
        cache.update(old)


def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def twin(ops, c=256, k=256, pad=1, stride=1, **fields):
    return ops.PackedConv(T, None, None, k, c, 3, 3, stride=stride, pad=pad, Cin=c, dtype=ops.SX6, **{f: T for f in fields})


def route(ops, pc, n=1, h=50, w=50, relu=1, res=False, crop=False):
    return ops._conv_route(lib(), pc, n, h, w, relu, res, crop, False)


def test_route_precedence_and_the_geometry_only_rule(ops):
    pc = twin(ops, u24x=T)
    assert route(ops, pc) == "wino24sx"
    assert ops._conv_variant(lib(), "wino24sx", pc, 1, 50, 50, 50, 50) == "conv3x3_wino24sx"
    # the same (h, w, c, k, pad) gives the same route at n = 1 and n = 80, on a large map and on the ROI-sized ones
    for h, w, pad in ((200, 200, 1), (25, 25, 1), (14, 14, 1), (14, 14, 0), (12, 12, 0)):
        p = twin(ops, pad=pad, u24x=T)
        assert route(ops, p, 1, h, w) == route(ops, p, 80, h, w) == "wino24sx", (h, w, pad)
    assert route(ops, pc, res=True) == "wino24sx" and route(ops, pc, relu=0) == "wino24sx"
    # without the planes, on a cropped call or with the ReLU-mask epilogue the twin stays on the split implicit GEMM
    assert route(ops, twin(ops)) == "igemm" and route(ops, pc, crop=True) == "crop" and route(ops, pc, relu=2) == "igemm"
    # the 8 x 8 -> 6 x 6 trunk conv stays on F(2x2): F(2x4) does not pay there, so the new route is not taken
    assert not ops._wino24_pays(lib(), 1, 8, 8, 256, 1024, 0)
    assert not ops.w24sx_map_ok(8, 8, 256, 1024, 0) and route(ops, twin(ops, k=1024, pad=0, u24x=T), 2560, 8, 8) == "igemm"
    # reductions below W24SX_MIN_C stay on the fp32 kernel (layer1's 64 -> 64)
    assert not ops.w24sx_map_ok(200, 200, 64, 64, 1) and ops.w24sx_map_ok(100, 100, 128, 128, 1)
    # an exact fp32 pack never takes it
    f32 = ops.PackedConv(T, None, None, 256, 256, 3, 3, stride=1, pad=1, Cin=256, dtype=ops.F32, u=T, u24=T)
    assert route(ops, f32) == "wino24"


def test_block_rule_is_one_image_alone(ops):
    """W24SX_MIN_BLOCKS = 128 blocks of ONE image, whatever the batch: 1 x 100^2 x 256 -> 256 is 160 blocks and 1 x 200^2 is 628 (the
    single-image wins of profiles/w24sx_layer_ab.txt); 100^2 x 128 -> 128 and 64 x 80 x 256 are 80, 50^2 is 44, a 14^2 ROI map 4."""
    L = lib()
    blocks = lambda h, w, c, k, pad: L.seam_conv3x3_wino24sx_blocks(1, h, w, c, k, pad)
    assert blocks(100, 100, 256, 256, 1) == 160 and blocks(200, 200, 256, 256, 1) == 628
    assert blocks(100, 100, 128, 128, 1) == 80 and blocks(64, 80, 256, 256, 1) == 80
    assert blocks(50, 50, 256, 256, 1) == 44 and blocks(14, 14, 256, 256, 1) == 4 and blocks(8, 8, 96, 64, 1) == 0
    ops.W24SX_MIN_BLOCKS = 128
    pc = twin(ops, u24x=T)
    for n in (1, 80):
        assert route(ops, pc, n, 200, 200) == route(ops, pc, n, 100, 100) == "wino24sx"
        assert route(ops, pc, n, 50, 50) == route(ops, pc, n, 64, 80) == "igemm"
        assert route(ops, pc, 32 * n, 14, 14) == "igemm"                  # 2560 ROIs are many blocks, one ROI map is 4
    ops.W24SX_MIN_BLOCKS = 44
    assert route(ops, pc, 1, 50, 50) == "wino24sx"


def test_layout_query_on_the_pinned_shapes():
    """seam_wino24_layout on the five maps of the block rule above, 256 -> 256, one image: the per-image patch blocks behind the
    pinned tile counts (x 4 n-tiles) and the regions they come from -- (TX, TY, bx, by) per region, zeros past nreg."""
    import w24_layout_cases as T
    L = lib()
    want = {
        (100, 100): dict(nreg=3, per_img=40, TX=(8, 1, 12), TY=(4, 25, 2), bx=(3, 1, 2), by=(12, 2, 1)),
        (200, 200): dict(nreg=2, per_img=157, TX=(8, 2, 0), TY=(4, 15, 0), bx=(6, 1, 0), by=(25, 7, 0)),
        (64, 80): dict(nreg=1, per_img=20, TX=(4, 0, 0), TY=(8, 0, 0), bx=(5, 0, 0), by=(4, 0, 0)),
        (50, 50): dict(nreg=2, per_img=11, TX=(6, 1, 0), TY=(5, 25, 0), bx=(2, 1, 0), by=(5, 1, 0)),
        (14, 14): dict(nreg=1, per_img=1, TX=(4, 0, 0), TY=(7, 0, 0), bx=(1, 0, 0), by=(1, 0, 0)),
    }
    for (h, w), exp in want.items():
        lay = T.query(L, 1, h, w, 256, 256, 1)
        assert {k: lay[k] for k in exp} == exp, (h, w, lay)
        assert (lay["stack"], lay["G"], lay["PH"], lay["nt"], lay["tiles_n"], lay["nsplit"]) == (0, 1, 0, 2, 4, 1), (h, w, lay)
        assert lay["patch_blocks"] == exp["per_img"] and lay["grid_blocks"] == 4 * exp["per_img"] == L.seam_conv3x3_wino24sx_blocks(1, h, w, 256, 256, 1)
        # eighty images: the same regions, eighty times the blocks; the fp32 launcher's plan differs in the n-tiles per block alone
        many, f32 = T.query(L, 80, h, w, 256, 256, 1), T.query(L, 1, h, w, 256, 256, 1, sx=0)
        if (h, w) == (14, 14):            # ... but the ROI-sized map, which stacks: 8 of the batch's 560 tile rows per block
            assert (many["stack"], many["TX"][0], many["TY"][0], many["G"], many["patch_blocks"]) == (1, 4, 8, 2, 70), many
        else:
            assert {k: many[k] for k in exp} == exp and many["patch_blocks"] == 80 * exp["per_img"]
        assert {k: f32[k] for k in exp} == exp and f32["nt"] == L.seam_wino24_variant(1, h, w, 256, 256, 1) and f32["tiles_n"] * f32["nt"] == 8
    # a forced split shows in the query (it reads the launcher's own arguments) and pads the grid, not the tiles
    before = L.seam_conv3x3_wino24sx_get_nsplit()
    try:
        assert L.seam_conv3x3_wino24sx_set_nsplit(2) == 0
        lay = T.query(L, 1, 100, 100, 256, 256, 1)
        assert lay["nsplit"] == 2 and lay["patch_blocks"] == 40 and lay["grid_blocks"] == 8 * 10 * 2
        assert T.query(L, 1, 100, 100, 256, 256, 1, sx=0)["nsplit"] == 1
    finally:
        L.seam_conv3x3_wino24sx_set_nsplit(before)


def test_knobs_restore_the_old_route(ops):
    pc = twin(ops, u24x=T)
    for knob, off in (("W24SX", False), ("WINOGRAD", False), ("WINOGRAD24", 0), ("W24SX_MIN_C", 512), ("W24SX_MIN_BLOCKS", 128)):
        old = getattr(ops, knob)
        setattr(ops, knob, off)
        ops._WINO24.clear()
        assert not ops.w24sx_map_ok(50, 50, 256, 256, 1) and route(ops, pc) == "igemm", knob
        setattr(ops, knob, old)
    ops._WINO24.clear()
    assert route(ops, pc) == "wino24sx"


def test_weight_bytes_and_supported():
    L = lib()
    assert L.seam_wino24sx_weight_bytes(256, 256) == 144 * 256 * 256 and L.seam_wino24sx_weight_bytes(64, 128) == 144 * 64 * 128
    ok = L.seam_conv3x3_wino24sx_supported
    assert ok(1, 8, 8, 64, 64, 1, 1) == 1 and ok(80, 200, 200, 256, 256, 1, 1) == 1 and ok(2560, 14, 14, 256, 256, 0, 1) == 1
    assert ok(1, 8, 8, 96, 64, 1, 1) == 0 and ok(1, 8, 8, 64, 32, 1, 1) == 0 and ok(1, 8, 8, 64, 64, 1, 2) == 0
    assert ok(1, 8, 8, 32, 64, 1, 1) == 0 and ok(1, 8, 8, 64, 64, 2, 1) == 0 and ok(0, 8, 8, 64, 64, 1, 1) == 0
    assert ok(1, 2, 2, 64, 64, 0, 1) == 0          # no output pixel


def test_repack_form_number():
    import os
    import re
    from seam_match_rcnn_amd import _native
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "seam_hip.h")).read()
    assert re.search(r"SEAM_REPACK_W24SX\s*=\s*%d\b" % _native.REPACK_W24SX, txt) and _native.REPACK_W24SX == 9
    assert "sizeof(seam_repack_job_t) == 80" in txt or _native.C.sizeof(_native.RepackJob) == 80


def test_class_plumbing_through_split_twin():
    import torch
    from seam_match_rcnn_amd.models import detection as det
    m = torch.nn.Module()
    saved = det.SPLIT_CLASSES, det.SPLIT_F32, det.SPLIT_DTYPE, det.ops.W24SX, det.ops.W24SX_MIN_BLOCKS
    try:
        det.SPLIT_F32, det.SPLIT_DTYPE, det.ops.W24SX, det.ops.W24SX_MIN_BLOCKS = True, det.ops.SX6, True, 0
        for cls in ("c2", "fpn3", "rpn3", "mask3"):
            det.SPLIT_CLASSES = frozenset({cls})
            assert det.split_twin(m, cls) is True
            det.SPLIT_DTYPE = det.ops.SX9                     # the kernel has the six-term form only
            assert det.split_twin(m, cls) is False
            det.SPLIT_DTYPE = det.ops.SX6
            det.SPLIT_CLASSES = frozenset({"c1"})
            assert det.split_twin(m, cls) is False
            # no twin is packed without the class, with the knob off, or for a reduction that never takes the kernel
            assert det.w24sx_twin(m, cls, torch.zeros(256, 256, 3, 3)) is None
        det.SPLIT_CLASSES = frozenset({"c2"})
        det.ops.W24SX = False
        assert det.w24sx_twin(m, "c2", torch.zeros(256, 256, 3, 3)) is None
        det.ops.W24SX = True
        assert det.w24sx_twin(m, "c2", torch.zeros(64, 64, 3, 3)) is None
        # pick_w24sx: the exact pack under grad, in training mode, with split_f32 off, on a map the rule refuses
        exact = det.ops.PackedConv(T, None, None, 256, 256, 3, 3, stride=1, pad=1, Cin=256, dtype=det.ops.F32)
        tw = det.ops.PackedConv(T, None, None, 256, 256, 3, 3, stride=1, pad=1, Cin=256, dtype=det.ops.SX6, u24x=T)
        x = torch.zeros(1, 50, 50, 256)
        m.eval()
        with torch.no_grad():
            assert det.pick_w24sx(m, exact, tw, x) is tw and det.pick_w24sx(m, exact, None, x) is exact
            assert det.pick_w24sx(m, exact, tw, torch.zeros(1, 3, 3, 256)) is exact or det.ops.w24sx_map_ok(3, 3, 256, 256, 1)
            m.train()
            assert det.pick_w24sx(m, exact, tw, x) is exact
            m.eval()
            det.set_split_f32(m, False)
            assert det.pick_w24sx(m, exact, tw, x) is exact
            det.set_split_f32(m, True)
        with torch.enable_grad():
            assert det.pick_w24sx(m, exact, tw, x) is exact
    finally:
        det.SPLIT_CLASSES, det.SPLIT_F32, det.SPLIT_DTYPE, det.ops.W24SX, det.ops.W24SX_MIN_BLOCKS = saved
