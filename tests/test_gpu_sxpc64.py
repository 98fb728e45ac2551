"""conv1x1_sxpc64 (csrc/seam_pwsx.hip): the 64-output-channel form of the split producer / consumer kernel, against
``seam_conv2d_sx(terms=6)`` on the same inputs -- the two entries compute the same bits, so every comparison is ``torch.equal``.

Tile geometry: 128 pixels x 64 output channels per tile, 64 channels per chunk, consumer wave w = channels 32 (w & 1) of pixels
64 (w >> 1).  M covers one row, a ragged half tile (63: the second pixel half of the only tile is empty), one full tile, one row
into the second tile, a ragged third tile and a persistent walk of 301 tiles (more than the 256 CUs); C covers two chunks (the
shortest the entry serves), three (the stem's), four and five.  Every output of the new entry is carved out of a larger allocation
with 1 MiB of guard bytes on both sides, checked after each launch."""
import math

import numpy as np
import pytest
import torch

DEV = "cuda:0"
gpu = pytest.mark.gpu
TILE = 128
GUARD = 1 << 20
K = 64
MS = [1, 63, TILE, TILE + 1, 300, TILE * 300 + 5]
CS = [128, 192, 256, 320]


def normal(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def guarded(m, k):
    """a poisoned [m, k] fp32 output between two guard regions of GUARD bytes; -> (tensor, check)"""
    raw = torch.full((2 * GUARD + m * k * 4,), 0x5A, dtype=torch.uint8, device=DEV)
    y = raw[GUARD:GUARD + m * k * 4].view(torch.float32).view(m, k)
    y.fill_(float("nan"))

    def intact():
        return bool((raw[:GUARD] == 0x5A).all()) and bool((raw[GUARD + m * k * 4:] == 0x5A).all())
    return y, intact


_PACKS, _X = {}, {}


def pack(c, seed=3):
    """(weight [64, c] on the host, its SX6 pack with ``wx64``), cached: packs are read only"""
    from seam_match_rcnn_amd import ops
    if (c, seed) not in _PACKS:
        wt = normal(seed, (K, c)) / math.sqrt(c)
        pc = ops.pack_conv(wt.view(K, c, 1, 1).to(DEV), dtype=ops.SX6)
        assert pc.wx64 is not None and pc.wx is None
        _PACKS[(c, seed)] = (wt, pc)
    return _PACKS[(c, seed)]


def rows(m, c):
    """the first m rows of one cached [max M, c] matrix (read only)"""
    if c not in _X:
        _X[c] = normal(7 + c, (max(MS), c)).to(DEV)
    return _X[c][:m]


def both(x, pc, scale=None, shift=None, res=None, relu=0):
    """-> (seam_conv2d_sx terms 6, seam_conv1x1_sxpc64) on x [M, C]; the guards of the second output are asserted"""
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    m, c = x.shape
    ref = torch.full((m, K), float("nan"), dtype=torch.float32, device=DEV)
    _native.check(lib.seam_conv2d_sx(ops._ptr(x), ops._ptr(pc.w), ops._ptr(scale), ops._ptr(shift), ops._ptr(res), ops._ptr(ref),
                                     1, m, 1, c, K, 1, 1, 1, 0, relu, 6, ops._stream()), "seam_conv2d_sx")
    y, intact = guarded(m, K)
    _native.check(lib.seam_conv1x1_sxpc64(ops._ptr(x), ops._ptr(pc.wx64), ops._ptr(scale), ops._ptr(shift), ops._ptr(res), ops._ptr(y),
                                          m, c, K, relu, ops._stream()), "seam_conv1x1_sxpc64")
    torch.cuda.synchronize()
    assert intact(), "guard bytes around the output were written"
    return ref, y


@gpu
@pytest.mark.parametrize("c", CS)
@pytest.mark.parametrize("m", MS)
def test_equals_the_split_gemm(m, c):
    _, pc = pack(c)
    ref, y = both(rows(m, c), pc)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(ref, y), (m, c, int((ref != y).sum()))


@gpu
@pytest.mark.parametrize("mode", ["shift", "scale_shift", "residual", "relu", "all"])
def test_epilogue_modes(mode):
    m, c = 300, 192
    _, pc = pack(c)
    scale = (normal(41, (K,)).abs() + 0.5).to(DEV) if mode in ("scale_shift", "all") else None
    shift = normal(42, (K,)).to(DEV) if mode in ("shift", "scale_shift", "all") else None
    res = normal(43, (m, K)).to(DEV) if mode in ("residual", "all") else None
    ref, y = both(rows(m, c), pc, scale=scale, shift=shift, res=res, relu=1 if mode in ("relu", "all") else 0)
    assert torch.equal(ref, y), (mode, int((ref != y).sum()))


@gpu
def test_launch_to_launch_and_batch_invariance():
    m, c = 3 * 50, 256
    _, pc = pack(c)
    x, shift = rows(m, c), normal(63, (K,)).to(DEV)
    _, first = both(x, pc, shift=shift, relu=1)
    for _ in range(20):
        assert torch.equal(both(x, pc, shift=shift, relu=1)[1], first)
    assert torch.equal(both(x[:50], pc, shift=shift, relu=1)[1], first[:50])       # one image of 50 pixels alone


@gpu
@pytest.mark.parametrize("m,c,k", [(64, 64, 64), (64, 96, 64), (64, 256, 128), (64, 256, 32), (0, 256, 64)])
def test_refusals_launch_nothing(m, c, k):
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    assert lib.seam_conv1x1_sxpc64_supported(m, c, k) == 0
    x = torch.zeros((64, 320), device=DEV)
    w = torch.zeros((128 * 320 * 6,), dtype=torch.uint8, device=DEV)
    y, intact = guarded(64, 128)
    assert lib.seam_conv1x1_sxpc64(ops._ptr(x), ops._ptr(w), None, None, None, ops._ptr(y), m, c, k, 0, ops._stream()) != 0
    if lib.seam_conv1x1_sxpc64_supported(1, c, k) == 0:         # the pack entry follows the kernel's rule for (C, K)
        assert lib.seam_pack_conv1x1_weight_sxpc64(ops._ptr(x), ops._ptr(y), k, c, ops._stream()) != 0
    torch.cuda.synchronize()
    assert intact() and bool(torch.isnan(y).all())
    assert lib.seam_conv1x1_sxpc64_supported(64, 256, 64) == 1
    assert lib.seam_conv1x1_sxpc64(ops._ptr(x), ops._ptr(w), None, None, None, ops._ptr(y), 64, 256, 64, 2, ops._stream()) != 0     # relu 0 | 1
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


def pieces_np(w):
    """the three truncation pieces of fp32 values, in numpy"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    p0 = (w.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = w - p0
    p1 = (r.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    return p0, p1, r - p1


def unpack_planes(wx, k, c):
    """[3][k][c] fp32 out of the fragment-order pack [k/32][c/16][3 planes][64 lanes = (k-half, row)][8 bf16]"""
    t = wx.view(torch.bfloat16).view(k // 32, c // 16, 3, 2, 32, 8).float()
    return t.permute(2, 0, 4, 1, 3, 5).reshape(3, k, c).cpu().numpy()


@gpu
def test_pack_and_repack_write_the_three_pieces_in_fragment_order():
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    c = 192
    wt, pc = pack(c, seed=5)
    assert pc.wx64.numel() == 6 * K * c
    got, want = unpack_planes(pc.wx64, K, c), pieces_np(wt.numpy())
    for p in range(3):
        assert np.array_equal(got[p].view(np.uint32), want[p].view(np.uint32)), p
    w = wt.to(DEV)
    b = torch.full((6 * K * c,), 0xEE, dtype=torch.uint8, device=DEV)
    job = _native.RepackJob(src=w.data_ptr(), dst=b.data_ptr(), scale=None, form=_native.REPACK_SXPC64, K=K, Cin=c, R=1, S=1, Cstore=c, mode=0)
    arr = (_native.RepackJob * 1)(job)
    blocks = int(lib.seam_repack_layout(arr, 1))
    assert blocks > 0
    table = ops._upload(arr, torch.device(DEV))
    _native.check(lib.seam_repack_many_f32(ops._ptr(table), 1, blocks, ops._stream()), "seam_repack_many_f32")
    torch.cuda.synchronize()
    assert torch.equal(pc.wx64, b)


@gpu
def test_conv2d_route_gives_the_bits_of_the_split_gemm():
    """``ops.conv2d`` on an SX6 pack with ``wx64``: route ``sxpc64`` (the knob on, the tile rule off) and the implicit GEMM agree."""
    from seam_match_rcnn_amd import ops
    _, pc = pack(256)
    x = rows(2 * 9 * 11, 256).view(2, 9, 11, 256)
    res = normal(44, (2, 9, 11, K)).to(DEV)
    saved = ops.SXPC64, ops.SXPC_RULE
    try:
        ops.SXPC64, ops.SXPC_RULE, ops.CONV_TRACE = True, False, []
        on = ops.conv2d(x, pc, relu=True, residual=res)
        assert [t[0] for t in ops.CONV_TRACE] == ["conv1x1_sxpc64"]
        ops.SXPC64, ops.CONV_TRACE = False, []
        off = ops.conv2d(x, pc, relu=True, residual=res)
        assert ops.CONV_TRACE[0][0].startswith("conv_igemm_sx<")
    finally:
        (ops.SXPC64, ops.SXPC_RULE), ops.CONV_TRACE = saved, None
    assert torch.equal(on, off)
