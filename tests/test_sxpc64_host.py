"""Host side of the 64-output-channel form, the stem and the `short` entries of csrc/seam_pwsx.hip: the exported entries, the
eligibility and size rules, the repack form, the new routes of ``ops._conv_route`` on fake packs, and that the older ``sxpc``
predicates answer as before.  No GPU: every call here runs on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("seam_conv1x1_sxpc64_supported", "seam_pack_conv1x1_weight_sxpc64", "seam_conv1x1_sxpc64", "seam_stem_sxpc_supported",
       "seam_stem_sxpc", "seam_conv1x1_sxpc_short_supported", "seam_pack_conv1x1_weight_sxpc_short", "seam_conv1x1_sxpc_short",
       "seam_conv1x1_sxpc_dual_short_supported", "seam_conv1x1_sxpc_dual_short", "seam_preprocess_s2d_pad_batch_f32")
T = object()        # stands for a packed tensor: any use of it as one raises


def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def test_header_exports_and_signatures_agree_for_the_new_entries():
    from seam_match_rcnn_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seam_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(seam_[a-z0-9_]+)\s*\(", txt))
    for name in NEW:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib(), name), name
    assert sorted(_native.SIGNATURES) == sorted(declared)
    S = _native.SIGNATURES
    assert S["seam_conv1x1_sxpc64"] == S["seam_conv1x1_sxpc_short"] == S["seam_conv1x1_sxpc"]
    assert S["seam_pack_conv1x1_weight_sxpc64"] == S["seam_pack_conv1x1_weight_sxpc_short"] == S["seam_pack_conv1x1_weight_sxpc"]
    assert S["seam_preprocess_s2d_pad_batch_f32"] == S["seam_preprocess_s2d_pad_batch_f16"]
    assert len(S["seam_conv1x1_sxpc_dual_short"][1]) == len(S["seam_conv1x1_sxpc_dual"][1]) - 1          # no stride2
    assert re.search(r"SEAM_REPACK_SXPC64\s*=\s*%d\b" % _native.REPACK_SXPC64, txt) and _native.REPACK_SXPC64 == 8
    assert C.sizeof(_native.RepackJob) == 80


@pytest.mark.parametrize("m,c,k,ok", [
    (1, 128, 64, 1), (45, 192, 64, 1), (12_800_000, 192, 64, 1), (300, 256, 64, 1), (5, 320, 64, 1), (1 << 20, 2048, 64, 1),
    (1, 64, 64, 0), (1, 96, 64, 0), (1, 200, 64, 0), (1, 256, 128, 0), (1, 256, 32, 0), (0, 256, 64, 0), (-1, 256, 64, 0),
    (1 << 31, 256, 64, 0)])
def test_sxpc64_rule(m, c, k, ok):
    assert lib().seam_conv1x1_sxpc64_supported(m, c, k) == ok


@pytest.mark.parametrize("m,c,k,ok", [
    (1, 128, 128, 1), (38405, 128, 512, 1), (1, 128, 64, 0), (1, 128, 192, 0), (1, 64, 128, 0), (1, 192, 128, 0), (1, 256, 128, 0),
    (0, 128, 128, 0)])
def test_short_rule(m, c, k, ok):
    assert lib().seam_conv1x1_sxpc_short_supported(m, c, k) == ok
    assert lib().seam_conv1x1_sxpc_dual_short_supported(m, c // 2, c - c // 2, k) == (ok if c == 128 else 0)


def test_short_dual_rule_needs_64_and_64():
    f = lib().seam_conv1x1_sxpc_dual_short_supported
    assert f(100, 64, 64, 256) == 1 and f(100, 32, 96, 256) == 0 and f(100, 128, 64, 256) == 0 and f(100, 64, 128, 256) == 0


@pytest.mark.parametrize("n,hs,ws,ok", [
    (80, 400, 400, 1), (3, 3, 5, 1), (1, 7, 1, 1), (1, 1, 1, 1), (1, 16, 8, 1), (0, 8, 8, 0), (1, 0, 8, 0), (1, 8, -2, 0),
    (1, 1 << 16, 1 << 16, 0),          # N Hs Ws >= 2^31
    (2, 6000, 6000, 0)])               # two frames of 1.7 GB under one tile's descriptor
def test_stem_rule(n, hs, ws, ok):
    assert lib().seam_stem_sxpc_supported(n, hs, ws) == ok


def test_weight_bytes_are_three_bf16_planes_without_padding():
    for k, c in ((64, 128), (64, 192), (64, 256), (512, 128)):
        assert lib().seam_conv1x1_sxpc_weight_bytes(k, c) == 6 * k * c


def test_the_old_predicates_answer_as_before():
    f = lib().seam_conv1x1_sxpc_supported
    assert f(1, 256, 64) == 0 and f(1, 64, 128) == 0 and f(1, 192, 128) == 0 and f(1, 128, 128) == 0 and f(1, 256, 128) == 1
    g = lib().seam_conv1x1_sxpc_dual_supported
    assert g(100, 64, 64, 256) == 0 and g(100, 64, 192, 256) == 1
    assert lib().seam_conv1x1_sxpc_up_supported(100, 1, 10, 10, 128, 256, 5, 5) == 0


def test_repack_layout_takes_the_new_form_by_the_new_rules_only():
    from seam_match_rcnn_amd import _native

    def job(**kw):
        d = dict(src=0x10000, dst=0x20000, scale=None, form=_native.REPACK_SXPC64, K=64, Cin=192, R=1, S=1, Cstore=192, mode=0)
        d.update(kw)
        return _native.RepackJob(**d)

    for good in (job(), job(Cin=256, Cstore=256), job(K=512, Cin=128, Cstore=128)):
        arr = (_native.RepackJob * 1)(good)
        assert lib().seam_repack_layout(arr, 1) > 0 and arr[0].items == good.K * good.Cstore // 8
    for bad in (job(Cin=64, Cstore=64), job(K=128), job(K=96, Cin=128, Cstore=128), job(R=3, S=3), job(mode=2), job(src=None)):
        arr = (_native.RepackJob * 2)(job(), bad)
        assert lib().seam_repack_layout(arr, 2) == -2
    old = job(form=_native.REPACK_SXPC)                  # the older form still refuses what the older pack entry refuses
    assert lib().seam_repack_layout((_native.RepackJob * 1)(old), 1) == -1


# ------------------------------------------------------------------------------------------------ routes
KNOBS = dict(SXPC=True, SXPC_MIN_TILES=196, SXPC_RULE=True, SXPC64=True, SXPC_SHORT=True, SW=True, SW_MIN_HW=196)


@pytest.fixture()
def ops():
    import seam_match_rcnn_amd.ops as ops
    saved = {k: getattr(ops, k) for k in KNOBS}
    for k, v in KNOBS.items():
        setattr(ops, k, v)
    yield ops
    for k, v in saved.items():
        setattr(ops, k, v)


def pack(ops, c, k, *fields, dtype="sx6"):
    dt = {"f32": ops.F32, "sx6": ops.SX6, "sx9": ops.SX9}[dtype]
    return ops.PackedConv(T, None, None, k, c, 1, 1, Cin=c, dtype=dt, **{f: T for f in fields})


def route(ops, pc, n=1, h=14, w=14, relu=0, res=False, crop=False):
    return ops._conv_route(lib(), pc, n, h, w, relu, res, crop, False)


# 196 tiles of 128 pixels x 64 channels: M = 24961 = 109 x 229 pixels are 196 row tiles, 24960 = 156 x 160 are 195;
# with K = 512 a row tile is four tiles: 49 x 128 = 6272 = 56 x 112 pixels are 196, 6144 = 48 x 128 are 192
CASES = [
    ("sxpc64 at the tile rule", (256, 64, "wx64"), dict(h=109, w=229), {}, "sxpc64"),
    ("sxpc64 below the tile rule", (256, 64, "wx64"), dict(h=156, w=160), {}, "igemm"),
    ("sxpc64 below the rule, SXPC_RULE off", (256, 64, "wx64"), dict(h=156, w=160), dict(SXPC_RULE=False), "sxpc64"),
    ("sxpc64 with a residual", (256, 64, "wx64"), dict(h=109, w=229, res=True), {}, "sxpc64"),
    ("sxpc64 knob off (the default)", (256, 64, "wx64"), dict(h=109, w=229), dict(SXPC64=False), "igemm"),
    ("SXPC off", (256, 64, "wx64"), dict(h=109, w=229), dict(SXPC=False), "igemm"),
    ("sxpc64 cropped", (256, 64, "wx64"), dict(h=109, w=229, crop=True), {}, "crop"),
    ("sxpc64 relu = 2", (256, 64, "wx64"), dict(h=109, w=229, relu=2), {}, "igemm"),
    ("sxpc64 without the pack field", (256, 64), dict(h=109, w=229), {}, "igemm"),
    ("one chunk is not served", (64, 64, "wx64"), dict(h=109, w=229), {}, "igemm"),
    ("short at the tile rule", (128, 512, "wxs"), dict(h=56, w=112, res=True), {}, "sxpc_short"),
    ("short below the tile rule", (128, 512, "wxs"), dict(h=48, w=128, res=True), {}, "igemm"),
    ("short counts the batch on a twin", (128, 512, "wxs"), dict(n=2, h=48, w=128), {}, "sxpc_short"),
    ("short knob off", (128, 512, "wxs"), dict(h=56, w=112), dict(SXPC_SHORT=False), "igemm"),
    ("short, SXPC off", (128, 512, "wxs"), dict(h=56, w=112), dict(SXPC=False), "igemm"),
    ("short cropped", (128, 512, "wxs"), dict(h=56, w=112, crop=True), {}, "crop"),
    ("the old route is untouched", (256, 128, "wx"), dict(h=109, w=229), {}, "sxpc"),
    ("the old route goes first", (256, 128, "wx", "wxs"), dict(h=109, w=229), {}, "sxpc"),
]


@pytest.mark.parametrize("name,pk,call,knobs,want", CASES, ids=[c[0] for c in CASES])
def test_routes(ops, name, pk, call, knobs, want):
    for k, v in knobs.items():
        setattr(ops, k, v)
    assert route(ops, pack(ops, *pk), **call) == want


def test_nine_term_and_exact_packs_never_take_the_new_routes(ops):
    assert route(ops, pack(ops, 256, 64, "wx64", dtype="sx9"), h=109, w=229) == "igemm"
    assert route(ops, pack(ops, 128, 512, "wxs", dtype="sx9"), h=56, w=112) == "igemm"
    assert route(ops, pack(ops, 128, 512, "ws", dtype="f32"), h=56, w=112) == "sw"


def test_the_bodys_map_rule_is_the_maps_alone(ops):
    assert ops.sxpc_short_map_ok(100, 100, 512) and not ops.sxpc_short_map_ok(50, 50, 512)          # 316 / 80 tiles per image
    ops.SXPC_RULE = False
    assert ops.sxpc_short_map_ok(8, 12, 512)
    ops.SXPC_RULE, ops.SXPC_SHORT = True, False
    assert not ops.sxpc_short_map_ok(100, 100, 512)


def test_stem_sx_ok(ops):
    twin = ops.PackedConv(T, None, None, 64, 192, 1, 1, Cin=192, dtype=ops.SX6, wx64=T)
    assert ops.stem_sx_ok(lib(), twin, 80, 400, 400) and ops.stem_sx_ok(lib(), twin, 1, 8, 16)
    assert not ops.stem_sx_ok(lib(), twin, 1, 9, 14)             # 126 cells
    assert not ops.stem_sx_ok(lib(), None, 80, 400, 400)
    assert not ops.stem_sx_ok(lib(), ops.PackedConv(T, None, None, 64, 192, 1, 1, Cin=192, dtype=ops.SX6), 80, 400, 400)
    ops.SXPC = False
    assert not ops.stem_sx_ok(lib(), twin, 80, 400, 400)


def test_split_classes_and_twins():
    import torch
    from seam_match_rcnn_amd.models import detection as det
    src = open(os.path.join(ROOT, "seam-match-rcnn_amd", "models", "detection.py")).read()
    default = re.search(r'"SEAM_SPLIT_CLASSES",\s*"([^"]*)"', src).group(1).split(",")
    assert "stem" in default and det.ResNet50Body.SPLIT_TWINS[-1] == "stem"
    m = torch.nn.Module()
    saved = det.SPLIT_CLASSES, det.SPLIT_F32, det.SPLIT_DTYPE
    try:
        det.SPLIT_F32, det.SPLIT_DTYPE = True, det.ops.SX6
        det.SPLIT_CLASSES = frozenset({"stem"})
        assert det.split_twin(m, "stem") is True
        det.SPLIT_DTYPE = det.ops.SX9                    # the stem has the six-term form only
        assert det.split_twin(m, "stem") is False
        det.SPLIT_DTYPE, det.SPLIT_CLASSES = det.ops.SX6, frozenset({"c1"})
        assert det.split_twin(m, "stem") is False
    finally:
        det.SPLIT_CLASSES, det.SPLIT_F32, det.SPLIT_DTYPE = saved
