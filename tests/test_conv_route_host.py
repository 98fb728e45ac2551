"""The routing rules of ``ops.conv2d`` (``ops._conv_route``) and the Winograd-form rule it shares with ``match_trunk``
(``ops._wino_form``), on the host: the route is a function of integers, flags, which pack fields exist, the module knobs and the
library's host predicates, so the packs here carry sentinels where the tensors would be.  No GPU.

Every expected route below is written down from the rules as ``ops.py`` documents them (the knob comments and ``_conv_route``), not
produced by calling the function.  Where a rule hands the decision to a library predicate, the case states the predicate's value as a
precondition."""
import pytest

T = object()        # stands for a packed tensor: any use of it as one raises

KNOBS = dict(WINOGRAD=True, WINOGRAD24=1, WINO_MIN_FILL=55, WINO24_MARGIN=0.95, NARROW=True, SW=True, SW_MIN_HW=196, PWPC=True,
             PWPC_MIN_HW=2500, F16PC=True, F16PC64=True, F16PC_RULE=True, SWH=True, PWHPC=True, PWHPC_MIN_C=1024, SXPC=True,
             SXPC_MIN_TILES=196, SXPC_RULE=True)


@pytest.fixture()
def ops():
    """The module with every knob at its documented default (whatever the environment set); all of them are put back afterwards."""
    import seam_match_rcnn_amd.ops as ops
    saved = {k: getattr(ops, k) for k in KNOBS}
    caches = dict(ops._WINO24), dict(ops._WINO_FILL)
    for k, v in KNOBS.items():
        setattr(ops, k, v)
    ops._WINO24.clear()         # (the F(2x4,3x3) decision is cached with the margin it was taken under)
    yield ops
    for k, v in saved.items():
        setattr(ops, k, v)
    for cache, old in zip((ops._WINO24, ops._WINO_FILL), caches):
        cache.clear()
        cache.update(old)


def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def pack(ops, dtype, c, k, r=1, stride=1, pad=0, **fields):
    dt = {"f32": ops.F32, "f16": ops.F16, "bx3": ops.BX3, "sx6": ops.SX6, "sx9": ops.SX9}[dtype]
    return ops.PackedConv(T, None, None, k, c, r, r, stride=stride, pad=pad, Cin=c, dtype=dt, **{f: T for f in fields})


def route(ops, pc, n=1, h=14, w=14, relu=0, res=False, crop=False, f32=False):
    return ops._conv_route(lib(), pc, n, h, w, relu, res, crop, f32)


# (name, dtype, C, K, conv kwargs, pack fields, call kwargs, knobs set for the case, expected route)
CASES = [
    # ---- SW_MIN_HW = 196 pixels: 14 x 14 = 196 takes the weights-stationary kernel, 13 x 14 = 182 does not
    ("sw at the threshold", "f32", 64, 64, {}, ("ws",), dict(h=14, w=14), {}, "sw"),
    ("sw below the threshold", "f32", 64, 64, {}, ("ws",), dict(h=13, w=14), {}, "igemm"),
    ("sw any batch: the rule is the map's", "f32", 64, 64, {}, ("ws",), dict(n=80, h=13, w=14), {}, "igemm"),
    ("sw with a residual (its epilogue adds it)", "f32", 64, 64, {}, ("ws",), dict(res=True), {}, "sw"),
    ("sw is no producer / consumer route: relu = 2 stays", "f32", 64, 64, {}, ("ws",), dict(relu=2), {}, "sw"),
    ("SW off", "f32", 64, 64, {}, ("ws",), {}, dict(SW=False), "igemm"),
    # ---- PWPC_MIN_HW = 2500 pixels: 50 x 50 against 49 x 50 = 2450 (C = 512, K = 128: seam_conv1x1_pc_supported)
    ("pwpc at the threshold", "f32", 512, 128, {}, ("wq",), dict(h=50, w=50), {}, "pwpc"),
    ("pwpc below the threshold", "f32", 512, 128, {}, ("wq",), dict(h=49, w=50), {}, "igemm"),
    ("pwpc with a residual", "f32", 512, 128, {}, ("wq",), dict(h=50, w=50, res=True), {}, "pwpc"),
    ("PWPC off", "f32", 512, 128, {}, ("wq",), dict(h=50, w=50), dict(PWPC=False), "igemm"),
    ("PWPC_MIN_HW lowered at run time", "f32", 512, 128, {}, ("wq",), dict(h=49, w=50), dict(PWPC_MIN_HW=2450), "pwpc"),
    # ---- SXPC_MIN_TILES = 196 tiles of 128 pixels x 128 channels: K = 128 is one column of tiles, so M = 24961 = 109 x 229 pixels are
    #      ceil(24961 / 128) = 196 tiles and M = 24960 = 156 x 160 are 195
    ("sxpc at the tile rule", "sx6", 256, 128, {}, ("wx",), dict(h=109, w=229), {}, "sxpc"),
    ("sxpc below the tile rule: the split GEMM", "sx6", 256, 128, {}, ("wx",), dict(h=156, w=160), {}, "igemm"),
    ("sxpc below the tile rule, SXPC_RULE off", "sx6", 256, 128, {}, ("wx",), dict(h=156, w=160), dict(SXPC_RULE=False), "sxpc"),
    ("sxpc counts the batch: 2 x 24960 pixels", "sx6", 256, 128, {}, ("wx",), dict(n=2, h=156, w=160), {}, "sxpc"),
    ("sxpc with a residual", "sx6", 256, 128, {}, ("wx",), dict(h=109, w=229, res=True), {}, "sxpc"),
    ("sxpc relu = 2: a flag is all the kernel takes", "sx6", 256, 128, {}, ("wx",), dict(h=109, w=229, relu=2), {}, "igemm"),
    ("SXPC off", "sx6", 256, 128, {}, ("wx",), dict(h=109, w=229), dict(SXPC=False), "igemm"),
    ("nine-term packs never take sxpc", "sx9", 256, 128, {}, ("wx",), dict(h=109, w=229), {}, "igemm"),
    # ---- PWHPC_MIN_C = 1024: reductions from this length on (maps of >= SW_MIN_HW pixels)
    ("pwhpc at C = 1024", "f16", 1024, 256, {}, ("wph",), {}, {}, "pwhpc"),
    ("pwhpc not at C = 512", "f16", 512, 256, {}, ("wph",), {}, {}, "igemm"),
    ("C = 512 stays on swh", "f16", 512, 256, {}, ("wph", "wsh"), {}, {}, "swh"),
    ("PWHPC_MIN_C lowered at run time", "f16", 512, 256, {}, ("wph", "wsh"), {}, dict(PWHPC_MIN_C=512), "pwhpc"),
    ("pwhpc needs the map too", "f16", 1024, 256, {}, ("wph",), dict(h=13, w=14), {}, "igemm"),
    ("pwhpc and swh both eligible: pwhpc", "f16", 1024, 256, {}, ("wph", "wsh"), {}, {}, "pwhpc"),
    ("a residual knocks pwhpc off (swh adds it)", "f16", 1024, 256, {}, ("wph", "wsh"), dict(res=True), {}, "swh"),
    ("a residual knocks pwhpc off", "f16", 1024, 256, {}, ("wph",), dict(res=True), {}, "igemm"),
    ("out_f32 knocks pwhpc and swh off", "f16", 1024, 256, {}, ("wph", "wsh"), dict(f32=True), {}, "igemm"),
    ("relu = 2 keeps pwhpc and swh off", "f16", 1024, 256, {}, ("wph", "wsh"), dict(relu=2), {}, "igemm"),
    ("PWHPC off", "f16", 1024, 256, {}, ("wph", "wsh"), {}, dict(PWHPC=False), "swh"),
    # ---- swh: the fp16 twin of sw, the same map rule
    ("swh at the threshold", "f16", 256, 256, {}, ("wsh",), dict(h=14, w=14), {}, "swh"),
    ("swh below the threshold", "f16", 256, 256, {}, ("wsh",), dict(h=13, w=14), {}, "igemm"),
    ("swh keeps a residual", "f16", 256, 256, {}, ("wsh",), dict(res=True), {}, "swh"),
    ("out_f32 knocks swh off", "f16", 256, 256, {}, ("wsh",), dict(f32=True), {}, "igemm"),
    ("relu = True is a flag", "f16", 256, 256, {}, ("wsh",), dict(relu=True), {}, "swh"),
    ("SWH off", "f16", 256, 256, {}, ("wsh",), {}, dict(SWH=False), "igemm"),
    # ---- f16pc: 3x3, C = K = 128, pad 1.  seam_conv3x3_f16pc_pays is 1 on 28 x 28 and 0 on 50 x 50, where _supported is 1
    ("f16pc where it pays", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=28, w=28), {}, "f16pc"),
    ("f16pc where it does not pay", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=50, w=50), {}, "igemm"),
    ("f16pc, F16PC_RULE off: every supported shape", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=50, w=50), dict(F16PC_RULE=False), "f16pc"),
    ("a residual knocks f16pc off", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=28, w=28, res=True), {}, "igemm"),
    ("out_f32 knocks f16pc off", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=28, w=28, f32=True), {}, "igemm"),
    ("relu = 2 keeps f16pc off", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=28, w=28, relu=2), {}, "igemm"),
    ("F16PC off", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=28, w=28), dict(F16PC=False), "igemm"),
    # ---- narrow: <= 16 outputs, any map, no residual; it goes before sw
    ("narrow", "f32", 256, 12, {}, ("wn",), dict(h=3, w=5), {}, "narrow"),
    ("narrow and sw both eligible: narrow", "f32", 256, 12, {}, ("wn", "ws"), {}, {}, "narrow"),
    ("narrow loses to a residual", "f32", 256, 12, {}, ("wn",), dict(res=True), {}, "igemm"),
    ("narrow loses to a residual: sw where eligible", "f32", 256, 12, {}, ("wn", "ws"), dict(res=True), {}, "sw"),
    ("NARROW off", "f32", 256, 12, {}, ("wn",), {}, dict(NARROW=False), "igemm"),
    ("NARROW off: sw where eligible", "f32", 256, 12, {}, ("wn", "ws"), {}, dict(NARROW=False), "sw"),
    # ---- a cropped output grid is the crop kernel's, whatever else the pack holds
    ("crop over sw", "f32", 64, 64, {}, ("ws",), dict(crop=True), {}, "crop"),
    ("crop over narrow", "f32", 256, 12, {}, ("wn",), dict(crop=True), {}, "crop"),
    ("crop over pwpc", "f32", 512, 128, {}, ("wq",), dict(h=50, w=50, crop=True), {}, "crop"),
    ("crop over wino", "f32", 256, 256, dict(r=3, pad=1), ("u", "u24"), dict(crop=True), dict(WINO_MIN_FILL=0), "crop"),
    ("crop over swh", "f16", 256, 256, {}, ("wsh",), dict(crop=True), {}, "crop"),
    ("crop over pwhpc", "f16", 1024, 256, {}, ("wph",), dict(crop=True), {}, "crop"),
    ("crop over f16pc", "f16", 128, 128, dict(r=3, pad=1), ("wh",), dict(n=2, h=28, w=28, crop=True), {}, "crop"),
    ("crop, plain packs", "f16", 16, 64, dict(r=4), (), dict(h=30, w=30, crop=True), {}, "crop"),
    # ---- Winograd: WINO_MIN_FILL = 0 / 101 % switch the fill rule on / off for any map (a fill is 0 .. 100)
    ("wino24 forced", "f32", 256, 256, dict(r=3), ("u", "u24"), {}, dict(WINO_MIN_FILL=0, WINOGRAD24=2), "wino24"),
    ("WINOGRAD24 off", "f32", 256, 256, dict(r=3), ("u", "u24"), {}, dict(WINO_MIN_FILL=0, WINOGRAD24=0), "wino"),
    ("no F(2x4,3x3) weights", "f32", 256, 256, dict(r=3), ("u",), {}, dict(WINO_MIN_FILL=0, WINOGRAD24=2), "wino"),
    ("the fill rule refuses", "f32", 256, 256, dict(r=3), ("u", "u24"), {}, dict(WINO_MIN_FILL=101, WINOGRAD24=2), "igemm"),
    ("WINOGRAD off", "f32", 256, 256, dict(r=3), ("u", "u24"), {}, dict(WINO_MIN_FILL=0, WINOGRAD24=2, WINOGRAD=False), "igemm"),
    ("wino with a residual", "f32", 256, 256, dict(r=3, pad=1), ("u",), dict(res=True), dict(WINO_MIN_FILL=0), "wino"),
    # ---- nothing optional packed: the implicit GEMM of the pack's dtype
    ("plain fp32", "f32", 64, 64, dict(r=3, stride=2, pad=1), (), {}, {}, "igemm"),
    ("plain fp16", "f16", 64, 64, {}, (), dict(f32=True), {}, "igemm"),
    ("plain bf16x3", "bx3", 256, 256, {}, (), {}, {}, "igemm"),
    ("plain bf16x6", "sx6", 64, 256, {}, (), dict(h=200, w=200), {}, "igemm"),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_route_table(ops, case):
    _, dtype, c, k, conv, fields, call, knobs, expected = case
    for name, v in knobs.items():
        setattr(ops, name, v)
    assert route(ops, pack(ops, dtype, c, k, **conv, **dict.fromkeys(fields, T)), **call) == expected


def test_the_table_s_preconditions_hold():
    """What the cases above take from the library's predicates."""
    l = lib()
    assert l.seam_conv1x1_pc_supported(2500, 512, 128) == 1 and l.seam_conv1x1_pc_supported(2450, 512, 128) == 1
    assert l.seam_conv1x1_sxpc_supported(24961, 256, 128) == 1 and l.seam_conv1x1_sxpc_supported(24960, 256, 128) == 1
    assert l.seam_conv1x1_f16pc_supported(196, 1024, 256) == 1 and l.seam_conv1x1_f16pc_supported(196, 512, 256) == 1
    assert l.seam_conv3x3_f16pc_pays(2, 28, 28, 128, 128, 1) == 1
    assert l.seam_conv3x3_f16pc_pays(2, 50, 50, 128, 128, 1) == 0 and l.seam_conv3x3_f16pc_supported(2, 50, 50, 128, 128, 1) == 1
    assert 109 * 229 == 24961 and 156 * 160 == 24960 and -(-24961 // 128) == 196 and -(-24960 // 128) == 195


def test_knobs_are_read_at_call_time_and_restored(ops):
    pc = pack(ops, "f32", 64, 64, ws=T)
    assert route(ops, pc) == "sw"
    ops.SW_MIN_HW = 197
    assert route(ops, pc) == "igemm"
    ops.SW_MIN_HW = 196
    assert route(ops, pc) == "sw"


def test_fixed_labels_and_igemm_labels(ops):
    l = lib()
    for r, label in (("sxpc", "conv1x1_sxpc"), ("pwhpc", "conv1x1_f16pc"), ("narrow", "linear_narrow"), ("pwpc", "conv1x1_pc"),
                     ("f16pc", "conv3x3_f16pc")):
        assert ops._conv_variant(l, r, pack(ops, "f32", 256, 128), 1, 14, 14, 14, 14) == label
    tile = l.seam_conv_tile_taps(0, 196, 128, 1)
    for r in ("igemm", "crop"):
        assert ops._conv_variant(l, r, pack(ops, "f32", 256, 128), 1, 14, 14, 14, 14) == f"conv_igemm<float,{tile // 1000},{tile % 1000}>"
    tile = l.seam_conv_tile_taps(3, 196, 128, 1)
    assert ops._conv_variant(l, "igemm", pack(ops, "sx6", 256, 128), 1, 14, 14, 14, 14) == f"conv_igemm_sx<{tile // 1000},{tile % 1000},6>"
    tile = l.seam_conv_tile_taps(2, 196, 128, 1)
    assert ops._conv_variant(l, "igemm", pack(ops, "bx3", 256, 128), 1, 14, 14, 14, 14) == f"conv_igemm_bx3<{tile // 1000},{tile % 1000}>"
    tile = l.seam_conv_tile_taps(1, 4 * 26 * 26, 128, 9)
    assert (ops._conv_variant(l, "igemm", pack(ops, "f16", 128, 128, r=3), 4, 28, 28, 26, 26)
            == f"conv_igemm<_Float16,{tile // 1000},{tile % 1000}>")
    assert ops._conv_variant(l, "sw", pack(ops, "f32", 64, 64, ws=T), 1, 14, 14, 14, 14).startswith("conv1x1_sw<")
    assert ops._conv_variant(l, "swh", pack(ops, "f16", 256, 256, wsh=T), 1, 14, 14, 14, 14).startswith("conv1x1_swh<")


def test_wino_form(ops):
    l = lib()
    both, only22, none = (pack(ops, "f32", 256, 256, r=3, **f) for f in (dict(u=T, u24=T), dict(u=T), {}))
    ops.WINO_MIN_FILL, ops.WINOGRAD24 = 0, 2
    assert ops._wino_form(l, both, 1, 14, 14, 256, 0) == 2
    assert ops._wino_form(l, only22, 1, 14, 14, 256, 0) == 1 and ops._wino_form(l, none, 1, 14, 14, 256, 0) == 0
    ops.WINOGRAD24 = 0
    assert ops._wino_form(l, both, 1, 14, 14, 256, 0) == 1
    ops.WINOGRAD24, ops.WINO_MIN_FILL = 2, 101
    assert ops._wino_form(l, both, 1, 14, 14, 256, 0) == 0
    ops.WINO_MIN_FILL, ops.WINOGRAD = 0, False
    assert ops._wino_form(l, both, 1, 14, 14, 256, 0) == 0


def test_wino_form_is_the_rule_of_both_callers(ops):
    """``match_trunk`` hands ``_wino_form`` of its four maps (14, 12, 10, 8 at C = 256, valid 3x3) to the library; ``conv2d`` on the same
    layer and map must pick the same kernel, for any number of ROIs (the rule is the map's)."""
    l = lib()
    pc = pack(ops, "f32", 256, 256, r=3, u=T, u24=T)
    name = {0: "igemm", 1: "wino", 2: "wino24"}
    for knobs in ({}, dict(WINOGRAD24=0), dict(WINOGRAD24=2), dict(WINO_MIN_FILL=95), dict(WINOGRAD=False)):
        for k, v in dict(KNOBS, **knobs).items():
            setattr(ops, k, v)
        ops._WINO24.clear()
        for h in (14, 12, 10, 8):
            forms = {ops._wino_form(l, pc, k, h, h, 256, 0) for k in (1, 37, 300)}
            assert len(forms) == 1
            assert route(ops, pc, n=37, h=h, w=h, relu=1) == name[forms.pop()]
    # at the defaults the fill rule decides: seam_wino_slot_fill_pct against WINO_MIN_FILL
    for k, v in KNOBS.items():
        setattr(ops, k, v)
    for h in (14, 12, 10, 8):
        assert (ops._wino_form(l, pc, 5, h, h, 256, 0) > 0) == (l.seam_wino_slot_fill_pct(256, h, h, 256, 256, 0) >= 55)
