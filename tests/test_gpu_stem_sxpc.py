"""stem_sxpc (csrc/seam_pwsx.hip): the ResNet stem over the zero-padded space-to-depth frame as the gather form of conv1x1_sxpc64,
against ``seam_conv1x1_sxpc64`` on the rows gathered with torch -- the same bits, so ``torch.equal`` -- and against a float64 CPU
convolution under the accuracy gate of tests/test_gpu_split_f32.py.

Frames ``(N, Hs, Ws)``: (3, 3, 5) is M = 45, one tile over three images; (2, 9, 11) a tile that straddles two images and a ragged
last tile; (1, 16, 8) exactly one tile; (1, 7, 1) Ws = 1; (1, 20, 13) three tiles in one image; (4, 96, 100) 300 tiles, more than
the 256 CUs.  The unpadded frames have no zero anywhere (|x| >= 0.5), their border cells included, so a window that reads a frame
cell where a zero cell belongs -- a wrong pad -- changes the result.  Outputs are written into poisoned, guarded buffers."""
import math

import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
gpu = pytest.mark.gpu
GUARD = 1 << 20
FRAMES = [(3, 3, 5), (2, 9, 11), (1, 16, 8), (1, 7, 1), (1, 20, 13), (4, 96, 100)]


def normal(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def guarded(shape):
    n = math.prod(shape) * 4
    raw = torch.full((2 * GUARD + n,), 0x5A, dtype=torch.uint8, device=DEV)
    y = raw[GUARD:GUARD + n].view(torch.float32).view(shape)
    y.fill_(float("nan"))

    def intact():
        return bool((raw[:GUARD] == 0x5A).all()) and bool((raw[GUARD + n:] == 0x5A).all())
    return y, intact


def frame(n, hs, ws):
    """[n, hs, ws, 12] without a zero: N(0, 1) pushed away from 0 by half a unit"""
    x = normal(100 + n * hs * ws, (n, hs, ws, 12))
    return x + 0.5 * torch.sign(x)


def padded(x):
    return F.pad(x, (0, 0, 2, 1, 2, 1)).contiguous()


def gathered(xp):
    """[N, Hs + 3, Ws + 3, 12] -> [N Hs Ws, 192]: per output pixel its 4 x 4 cells in (r, s, c) order"""
    n, hp, wp, _ = xp.shape
    win = xp.unfold(1, 4, 1).unfold(2, 4, 1)                 # [N, Hs, Ws, 12, r, s]
    return win.permute(0, 1, 2, 4, 5, 3).reshape(n * (hp - 3) * (wp - 3), 192).contiguous()


_W = {}


def weights():
    """(rows [64, 192] on the host in (r, s, c) order, their SX6 pack, scale, shift), cached: read only"""
    from seam_match_rcnn_amd import ops
    if not _W:
        rows = normal(5, (64, 192)) / math.sqrt(147)
        pc = ops.pack_conv(rows.view(64, 192, 1, 1).to(DEV), dtype=ops.SX6)
        assert pc.wx64 is not None
        _W["w"] = (rows, pc, (normal(6, (64,)).abs() + 0.5).to(DEV), normal(7, (64,)).to(DEV))
    return _W["w"]


def stem(xp, pc, scale, shift, relu):
    from seam_match_rcnn_amd import _native, ops
    n, hp, wp, _ = xp.shape
    y, intact = guarded((n, hp - 3, wp - 3, 64))
    _native.check(_native.lib().seam_stem_sxpc(ops._ptr(xp), ops._ptr(pc.wx64), ops._ptr(scale), ops._ptr(shift), ops._ptr(y),
                                               n, hp - 3, wp - 3, relu, ops._stream()), "seam_stem_sxpc")
    torch.cuda.synchronize()
    assert intact(), "guard bytes around the output were written"
    return y


def rows_gemm(r, pc, scale, shift, relu):
    from seam_match_rcnn_amd import _native, ops
    y = torch.full((r.shape[0], 64), float("nan"), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().seam_conv1x1_sxpc64(ops._ptr(r), ops._ptr(pc.wx64), ops._ptr(scale), ops._ptr(shift), None, ops._ptr(y),
                                                    r.shape[0], 192, 64, relu, ops._stream()), "seam_conv1x1_sxpc64")
    return y


@gpu
@pytest.mark.parametrize("epilogue", ["plain", "bn_relu"])
@pytest.mark.parametrize("shape", FRAMES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_64_channel_form_on_gathered_rows(shape, epilogue):
    _, pc, scale, shift = weights()
    x = frame(*shape)
    assert bool((x.abs() >= 0.5).all())
    xp = padded(x).to(DEV)
    sc, sh, relu = (scale, shift, 1) if epilogue == "bn_relu" else (None, None, 0)
    y = stem(xp, pc, sc, sh, relu)
    ref = rows_gemm(gathered(xp), pc, sc, sh, relu).view(y.shape)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(y, ref), (shape, int((y != ref).sum()))


@gpu
def test_a_frame_alone_gives_the_bits_it_has_in_a_batch():
    _, pc, scale, shift = weights()
    xp = padded(frame(2, 9, 11)).to(DEV)
    y = stem(xp, pc, scale, shift, 1)
    assert torch.equal(stem(xp[1:].contiguous(), pc, scale, shift, 1), y[1:])


@gpu
def test_accuracy_gate_against_float64():
    """e = max|y - y64| / max|y64| against the float64 CPU convolution: e_split <= 2 e_exact + 1e-7, e_exact from the exact stem
    launch (the implicit GEMM over the unpadded frame, pad 2, cropped to the frame's grid) on the same input."""
    from seam_match_rcnn_amd import ops
    rows, pc, scale, shift = weights()
    x = frame(4, 96, 100)
    w4 = rows.view(64, 4, 4, 12).permute(0, 3, 1, 2).contiguous()                # OIHW of the 4x4 / stride-1 form
    y64 = F.conv2d(F.pad(x.double().permute(0, 3, 1, 2), (2, 1, 2, 1)), w4.double())
    y64 = torch.relu(y64 * scale.cpu().double()[None, :, None, None] + shift.cpu().double()[None, :, None, None]).permute(0, 2, 3, 1)
    ys = stem(padded(x).to(DEV), pc, scale, shift, 1)
    exact = ops.pack_conv(w4.to(DEV), stride=1, pad=2, cstore=12, wino=False)
    exact.scale, exact.shift = scale, shift
    ye = ops.conv2d(x.to(DEV), exact, relu=True, out_hw=(96, 100))
    top = float(y64.abs().max())
    e_split = float((ys.cpu().double() - y64).abs().max()) / top
    e_exact = float((ye.cpu().double() - y64).abs().max()) / top
    print(f"stem_sxpc gate (4, 96, 100): e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


@gpu
def test_refusals_launch_nothing():
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    _, pc, _, _ = weights()
    xp = torch.zeros((1, 10, 10, 12), device=DEV)
    y, intact = guarded((1, 7, 7, 64))
    for n, hs, ws in ((0, 7, 7), (1, 0, 7), (1, 7, -1), (1, 1 << 16, 1 << 16)):
        assert lib.seam_stem_sxpc_supported(n, hs, ws) == 0
        assert lib.seam_stem_sxpc(ops._ptr(xp), ops._ptr(pc.wx64), None, None, ops._ptr(y), n, hs, ws, 0, ops._stream()) != 0
    assert lib.seam_stem_sxpc_supported(1, 7, 7) == 1
    assert lib.seam_stem_sxpc(ops._ptr(xp), ops._ptr(pc.wx64), None, None, ops._ptr(y), 1, 7, 7, 2, ops._stream()) != 0       # relu 0 | 1
    assert lib.seam_stem_sxpc(None, ops._ptr(pc.wx64), None, None, ops._ptr(y), 1, 7, 7, 0, ops._stream()) != 0
    torch.cuda.synchronize()
    assert intact() and bool(torch.isnan(y).all())
