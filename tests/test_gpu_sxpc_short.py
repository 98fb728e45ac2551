"""The `short` entries (csrc/seam_pwsx.hip): conv1x1_sxpc and conv1x1_sxpc_dual on reductions of two chunks per tile, C == 128 and
C1 == C2 == 64.  ``seam_conv1x1_sxpc_short`` against ``seam_conv2d_sx(terms=6)``, the two-source form against the plain one on the
concatenated rows: the same bits, ``torch.equal``.  M = 1, one row into the second tile, and 38405 rows: 301 row tiles x 4 channel
tiles, more than four tiles per CU.  The two-source maps: (2, 9, 11) has tiles straddling the two images, (1, 20, 13) three tiles in
one image.  Outputs are written into poisoned, guarded buffers."""
import math

import pytest
import torch

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
GUARD = 1 << 20


def normal(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def guarded(m, k):
    raw = torch.full((2 * GUARD + m * k * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    y = raw[GUARD:GUARD + m * k * 4].view(torch.float32).view(m, k)
    y.fill_(float("nan"))
    return y, lambda: bool((raw[:GUARD] == 0x5A).all()) and bool((raw[GUARD + m * k * 4:] == 0x5A).all())


_PACKS = {}


def pack(k):
    from seam_match_rcnn_amd import ops
    if k not in _PACKS:
        wt = normal(3 + k, (k, 128)) / math.sqrt(128)
        pc = ops.pack_conv(wt.view(k, 128, 1, 1).to(DEV), dtype=ops.SX6)
        assert pc.wxs is not None and pc.wx is None
        _PACKS[k] = pc
    return _PACKS[k]


def short(x, pc, scale, shift, res, relu):
    from seam_match_rcnn_amd import _native, ops
    m = x.shape[0]
    y, intact = guarded(m, pc.K)
    _native.check(_native.lib().seam_conv1x1_sxpc_short(ops._ptr(x), ops._ptr(pc.wxs), ops._ptr(scale), ops._ptr(shift), ops._ptr(res),
                                                        ops._ptr(y), m, 128, pc.K, relu, ops._stream()), "seam_conv1x1_sxpc_short")
    torch.cuda.synchronize()
    assert intact(), "guard bytes around the output were written"
    return y


@pytest.mark.parametrize("m", [1, 129, 38405])
def test_plain_equals_the_split_gemm_with_a_residual(m):
    from seam_match_rcnn_amd import _native, ops
    k = 512
    pc = pack(k)
    x, res = normal(7, (m, 128)).to(DEV), normal(8, (m, k)).to(DEV)
    scale, shift = (normal(9, (k,)).abs() + 0.5).to(DEV), normal(10, (k,)).to(DEV)
    ref = torch.full((m, k), float("nan"), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().seam_conv2d_sx(ops._ptr(x), ops._ptr(pc.w), ops._ptr(scale), ops._ptr(shift), ops._ptr(res), ops._ptr(ref),
                                               1, m, 1, 128, k, 1, 1, 1, 0, 1, 6, ops._stream()), "seam_conv2d_sx")
    y = short(x, pc, scale, shift, res, 1)
    assert bool(torch.isfinite(ref).all()) and torch.equal(ref, y), (m, int((ref != y).sum()))


@pytest.mark.parametrize("shape", [(2, 9, 11), (1, 20, 13)], ids=lambda s: "x".join(map(str, s)))
def test_two_source_equals_the_plain_kernel_on_concatenated_rows(shape):
    from seam_match_rcnn_amd import _native, ops
    n, ho, wo = shape
    k, m = 256, n * ho * wo
    pc = pack(k)
    x1, x2 = normal(11, (n, ho, wo, 64)).to(DEV), normal(12, (n, ho, wo, 64)).to(DEV)
    shift = normal(13, (k,)).to(DEV)
    y, intact = guarded(m, k)
    _native.check(_native.lib().seam_conv1x1_sxpc_dual_short(ops._ptr(x1), ops._ptr(x2), ops._ptr(pc.wxs), None, ops._ptr(shift), ops._ptr(y),
                                                             n, ho, wo, 64, ho, wo, 64, k, 1, ops._stream()), "seam_conv1x1_sxpc_dual_short")
    torch.cuda.synchronize()
    assert intact()
    rows = torch.cat([x1, x2], -1).view(m, 128).contiguous()
    assert torch.equal(y, short(rows, pc, None, shift, None, 1))


def test_refusals_launch_nothing():
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    pc = pack(256)
    x = torch.zeros((64, 256), device=DEV)
    y, intact = guarded(64, 256)
    for m, c, k in ((64, 64, 256), (64, 192, 256), (64, 256, 256), (64, 128, 64), (0, 128, 256)):
        assert lib.seam_conv1x1_sxpc_short_supported(m, c, k) == 0
        assert lib.seam_conv1x1_sxpc_short(ops._ptr(x), ops._ptr(pc.wxs), None, None, None, ops._ptr(y), m, c, k, 0, ops._stream()) != 0
    for c1, c2 in ((128, 64), (64, 128), (32, 96)):
        assert lib.seam_conv1x1_sxpc_dual_short_supported(64, c1, c2, 256) == 0
        assert lib.seam_conv1x1_sxpc_dual_short(ops._ptr(x), ops._ptr(x), ops._ptr(pc.wxs), None, None, ops._ptr(y), 1, 8, 8, c1, 8, 8, c2, 256, 0,
                                                ops._stream()) != 0
    assert lib.seam_conv1x1_sxpc_dual_short(ops._ptr(x), None, ops._ptr(pc.wxs), None, None, ops._ptr(y), 1, 8, 8, 64, 8, 8, 64, 256, 0, ops._stream()) != 0
    torch.cuda.synchronize()
    assert intact() and bool(torch.isnan(y).all())


def test_the_body_picks_the_short_twins_by_the_map_and_the_knob():
    """Two 64 x 96 images (NHWC4): layer1.0's shortcut GEMM runs the two-source twin; layer2's expansions are 8 x 12 maps, below the
    map rule, and stay exact until the rule is lifted; with the knob off every launch is the one before the entries existed."""
    import numpy as np
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    pfx = "backbone.body."
    sd = {k[len(pfx):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items() if k.startswith(pfx)}
    body = det.ResNet50Body()
    body.load_state_dict(sd)
    body = body.to(DEV).eval()
    x = normal(91, (2, 64, 96, 4))
    x[..., 3] = 0
    x = x.to(DEV)

    def traced():
        ops.CONV_TRACE = []
        try:
            with torch.no_grad():
                return body(x), [t[0] for t in ops.CONV_TRACE]
        finally:
            ops.CONV_TRACE = None
    saved = ops.SXPC_SHORT, ops.SXPC_RULE, ops.SXPC
    try:
        pk = body.packed()
        assert "c3dsxs" in pk[(1, 0)] and [key for key in pk if isinstance(key, tuple) and "c3xs" in pk[key]] == [(2, 1), (2, 2), (2, 3)]
        on, names = traced()
        assert names.count("conv1x1_sxpc_dual_short") == 1 and "conv1x1_sxpc_short" not in names
        ops.SXPC = False                                    # the twins on the implicit GEMM: the same bits
        off, names2 = traced()
        assert not any(n.startswith("conv1x1_sxpc") for n in names2) and all(torch.equal(a, b) for a, b in zip(on, off))
        ops.SXPC, ops.SXPC_RULE = True, False
        lifted, names3 = traced()
        assert names3.count("conv1x1_sxpc_short") == 3
        ops.SXPC_RULE, ops.SXPC_SHORT = saved[1], False
        before, names4 = traced()
        assert not any(n.startswith(("conv1x1_sxpc_short", "conv1x1_sxpc_dual_short")) for n in names4)
        assert sum(n.startswith("conv1x1_sw") for n in names4) == sum(n.startswith("conv1x1_sw") for n in names) + 1
        assert any(not torch.equal(a, b) for a, b in zip(on, before))
        assert float((on[0] - before[0]).abs().max()) <= 1e-5 * float(before[0].abs().max())
    finally:
        ops.SXPC_SHORT, ops.SXPC_RULE, ops.SXPC = saved
