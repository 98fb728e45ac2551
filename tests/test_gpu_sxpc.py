"""conv1x1_sxpc (csrc/seam_pwsx.hip): the six-term split-bf16 1x1 convolution on a producer / consumer block, against
``seam_conv2d_sx(terms=6)`` on the same inputs -- the two entries compute the same bits, so every comparison is ``torch.equal``.

Tile geometry of the kernel: 128 pixels x 128 output channels per tile, 64 channels per chunk.  The shapes below are the smallest
that reach each mechanism: ragged and tiny M, the shortest and a long reduction, an odd number of chunks, one / three / eight
n-tiles, a persistent walk of more than three tiles per CU, fewer tiles than CUs, every epilogue mode.  Every output of the new
entry is carved out of a larger allocation with 1 MiB of guard bytes on both sides, checked after each launch."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu
TILE = 128
CHUNK = 64
GUARD = 1 << 20


def bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


# all-ones mantissas, alternating bits, the neighbours of +-FLT_MAX, 2^-120, zeros, mixed signs (the values of
# tests/test_gpu_split_f32.py)
SPECIAL = bits([0x3fffffff, 0xbfffffff, 0x7f7fffff, 0xff7fffff, 0x7f7ffffe, 0xff7ffffe, 0x7f7f0001, 0x7f000001,
                0x55555555, 0xaaaaaaaa, 0x2aaaaaaa, 0xd5555555, 0x3faaaaaa, 0xbf555555, 0x03800000, 0x83800000,
                0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x3f80ffff, 0x3f8000ff, 0x3fff00ff, 0xbf80ff01,
                0x4b7fffff, 0xcb7fffff, 0x3effffff, 0x3f000001, 0x40490fdb, 0xc02df854, 0x0dffffff, 0x7effffff])


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


_PACKS = {}


def pack(c, k, seed=3):
    """(weight [k, c] on the host, the SX6 pack with both weight forms), cached: packs are read only"""
    from seam_match_rcnn_amd import ops
    key = (c, k, seed)
    if key not in _PACKS:
        wt = normal(seed, (k, c)) / math.sqrt(c)
        pc = ops.pack_conv(wt.view(k, c, 1, 1).to(DEV), dtype=ops.SX6)
        assert pc.wx is not None
        _PACKS[key] = (wt, pc)
    return _PACKS[key]


def both(x, pc, scale=None, shift=None, res=None, relu=0):
    """-> (seam_conv2d_sx terms 6, seam_conv1x1_sxpc) on x [M, C]; the guards of the second output are asserted"""
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    m, c = x.shape
    k = pc.K
    ref = torch.full((m, k), float("nan"), dtype=torch.float32, device=DEV)
    _native.check(lib.seam_conv2d_sx(ops._ptr(x), ops._ptr(pc.w), ops._ptr(scale), ops._ptr(shift), ops._ptr(res), ops._ptr(ref),
                                     1, m, 1, c, k, 1, 1, 1, 0, relu, 6, ops._stream()), "seam_conv2d_sx")
    y, intact = guarded(m, k)
    _native.check(lib.seam_conv1x1_sxpc(ops._ptr(x), ops._ptr(pc.wx), ops._ptr(scale), ops._ptr(shift), ops._ptr(res), ops._ptr(y),
                                        m, c, k, relu, ops._stream()), "seam_conv1x1_sxpc")
    torch.cuda.synchronize()
    assert intact(), "guard bytes around the output were written"
    return ref, y


def check_equal(m, c, k, seed=7, **kw):
    _, pc = pack(c, k)
    x = normal(seed, (m, c)).to(DEV)
    ref, y = both(x, pc, **kw)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(ref, y), (m, c, k, int((ref != y).sum()))


@gpu
@pytest.mark.parametrize("m", [1, 37, TILE - 1, TILE + 1, 3 * TILE + 5])
def test_ragged_and_tiny_m(m):
    check_equal(m, 256, 128)


@gpu
@pytest.mark.parametrize("c", [256, 256 + CHUNK, 1024])
def test_reduction_lengths(c):
    check_equal(TILE + 1, c, 128)


@gpu
@pytest.mark.parametrize("k", [128, 384, 1024])
def test_output_widths(k):
    check_equal(TILE + 1, 256, k)


@gpu
def test_persistent_walk_of_more_than_three_tiles_per_cu():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    m, k = 50_000, 256
    tiles = -(-m // TILE) * (k // 128)
    assert tiles > 3 * cus and tiles % cus != 0, (tiles, cus)
    check_equal(m, 256, k)


@gpu
def test_fewer_tiles_than_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * 3 < cus
    check_equal(TILE + 9, 320, 384)             # six tiles, an odd number of chunks: the buffers' roles differ from tile to tile


@gpu
@pytest.mark.parametrize("mode", ["none", "shift", "scale_shift", "residual", "relu", "all"])
def test_epilogue_modes(mode):
    m, c, k = 3 * TILE + 5, 256, 384
    scale = (normal(41, (k,)).abs() + 0.5).to(DEV) if mode in ("scale_shift", "all") else None
    shift = normal(42, (k,)).to(DEV) if mode in ("shift", "scale_shift", "all") else None
    res = normal(43, (m, k)).to(DEV) if mode in ("residual", "all") else None
    check_equal(m, c, k, scale=scale, shift=shift, res=res, relu=1 if mode in ("relu", "all") else 0)


@gpu
def test_piece_identity():
    """SPECIAL tiled to 256 channels through a 256 x 256 identity weight: all values in one pixel, and one value per pixel;
    the outputs are the inputs (the case that caught the v_pk_add_f32 fold in the split)."""
    from seam_match_rcnn_amd import _native, ops
    assert bool(torch.isfinite(SPECIAL).all())
    vals = SPECIAL.repeat(8)
    pc = ops.pack_conv(torch.eye(256).view(256, 256, 1, 1).to(DEV), dtype=ops.SX6)
    assert pc.wx is not None
    lib = _native.lib()
    for x in (vals.view(1, 256), torch.diag(vals)):
        y, intact = guarded(x.shape[0], 256)
        _native.check(lib.seam_conv1x1_sxpc(ops._ptr(x.to(DEV)), ops._ptr(pc.wx), None, None, None, ops._ptr(y), x.shape[0], 256, 256, 0,
                                            ops._stream()), "seam_conv1x1_sxpc")
        torch.cuda.synchronize()
        assert intact()
        wrong = (y.cpu().double() != x.double()).nonzero().tolist()
        print(f"sxpc identity {tuple(x.shape)}: wrong at {wrong[:8]}")
        assert torch.equal(y.cpu().double(), x.double())


@gpu
def test_accuracy_gate_long_reduction_with_residual():
    """The project's gate, explicit on one case: e <= 2 e_exact + 1e-7, e = max|y - y64| / max|y64|, e_exact from seam_conv2d_f32."""
    from seam_match_rcnn_amd import _native, ops
    m, c, k = 200, 1024, 256
    wt, pc = pack(c, k)
    x, res, bias = normal(51, (m, c)), normal(52, (m, k)), normal(53, (k,)) * 0.1
    ref = F.linear(x.double(), wt.double(), bias.double()) + res.double()
    xd, rd, bd = x.to(DEV), res.to(DEV), bias.to(DEV)
    _, y = both(xd, pc, shift=bd, res=rd)
    pe = ops.pack_conv(wt.view(k, c, 1, 1).to(DEV), wino=False)
    ye = torch.empty((m, k), dtype=torch.float32, device=DEV)
    _native.check(_native.lib().seam_conv2d_f32(ops._ptr(xd), ops._ptr(pe.w), None, ops._ptr(bd), ops._ptr(rd), ops._ptr(ye),
                                                1, m, 1, c, k, 1, 1, 1, 0, 0, ops._stream()), "seam_conv2d_f32")
    scale = float(ref.abs().max())
    e = float((y.cpu().double() - ref).abs().max()) / scale
    e_exact = float((ye.cpu().double() - ref).abs().max()) / scale
    print(f"sxpc gate {(m, c, k)}: e {e:.3e} e_exact {e_exact:.3e}")
    assert e <= 2 * e_exact + 1e-7, (e, e_exact)


@gpu
def test_launch_to_launch_and_batch_invariance():
    m, c, k = 3 * 50, 512, 256
    _, pc = pack(c, k)
    x, res, shift = normal(61, (m, c)).to(DEV), normal(62, (m, k)).to(DEV), normal(63, (k,)).to(DEV)
    ref, first = both(x, pc, shift=shift, res=res, relu=1)
    assert torch.equal(ref, first)
    for _ in range(49):
        assert torch.equal(launch(x, pc, shift, res), first)
    alone = launch(x[:50].contiguous(), pc, shift, res[:50].contiguous())       # one image of 50 pixels alone
    assert torch.equal(alone, first[:50])


def launch(x, pc, shift, res):
    from seam_match_rcnn_amd import _native, ops
    y, intact = guarded(x.shape[0], pc.K)
    _native.check(_native.lib().seam_conv1x1_sxpc(ops._ptr(x), ops._ptr(pc.wx), None, ops._ptr(shift), ops._ptr(res), ops._ptr(y),
                                                  x.shape[0], x.shape[1], pc.K, 1, ops._stream()), "seam_conv1x1_sxpc")
    torch.cuda.synchronize()
    assert intact()
    return y


@gpu
@pytest.mark.parametrize("m,c,k", [(64, 64, 128), (64, 288, 128), (64, 256, 96), (0, 256, 128)])
def test_refusals(m, c, k):
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    assert lib.seam_conv1x1_sxpc_supported(m, c, k) == 0
    x = torch.zeros((64, 320), device=DEV)
    w = torch.zeros((128 * 320 * 6,), dtype=torch.uint8, device=DEV)
    y, intact = guarded(64, 128)
    assert lib.seam_conv1x1_sxpc(ops._ptr(x), ops._ptr(w), None, None, None, ops._ptr(y), m, c, k, 0, ops._stream()) != 0
    torch.cuda.synchronize()
    assert intact() and bool(torch.isnan(y).all())
    assert lib.seam_conv1x1_sxpc_supported(64, 256, 128) == 1
    assert lib.seam_conv1x1_sxpc(ops._ptr(x), ops._ptr(w), None, None, None, ops._ptr(y), 64, 256, 128, 2, ops._stream()) != 0     # relu 0 | 1


def pieces_np(w):
    """the three truncation pieces of fp32 values, in numpy"""
    w = np.ascontiguousarray(w, dtype=np.float32)
    p0 = (w.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    r = w - p0
    p1 = (r.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    p2 = r - p1
    return p0, p1, p2


def unpack_planes(wx, k, c):
    """[3][k][c] fp32 out of the fragment-order pack [k/32][c/16][3 planes][64 lanes = (k-half, row)][8 bf16]"""
    t = wx.view(torch.bfloat16).view(k // 32, c // 16, 3, 2, 32, 8).float()
    return t.permute(2, 0, 4, 1, 3, 5).reshape(3, k, c).cpu().numpy()


@gpu
def test_pack_is_the_three_pieces_in_fragment_order():
    k, c = 256, 320
    wt = normal(71, (k, c)) / math.sqrt(c)
    wt[0, :32] = SPECIAL
    from seam_match_rcnn_amd import ops
    pc = ops.pack_conv(wt.view(k, c, 1, 1).to(DEV), dtype=ops.SX6)
    got = unpack_planes(pc.wx, k, c)
    want = pieces_np(wt.numpy())
    for p in range(3):
        assert np.array_equal(got[p].view(np.uint32), want[p].view(np.uint32)), p
    assert np.array_equal(got.astype(np.float64).sum(0), wt.numpy().astype(np.float64))


@gpu
def test_repack_many_writes_the_bytes_of_the_per_layer_entry():
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    k, c = 384, 320
    w = (normal(81, (k, c, 1, 1)) / math.sqrt(c)).to(DEV)
    nbytes = int(lib.seam_conv1x1_sxpc_weight_bytes(k, c))
    assert nbytes == 6 * k * c
    a = torch.zeros((nbytes,), dtype=torch.uint8, device=DEV)
    b = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=DEV)
    w.mul_(1.25).add_(0.001)                                # the source changed in place, as after an optimizer step
    _native.check(lib.seam_pack_conv1x1_weight_sxpc(ops._ptr(w), ops._ptr(a), k, c, ops._stream()), "seam_pack_conv1x1_weight_sxpc")
    job = _native.RepackJob(src=w.data_ptr(), dst=b.data_ptr(), scale=None, form=_native.REPACK_SXPC, K=k, Cin=c, R=1, S=1, Cstore=c, mode=0)
    arr = (_native.RepackJob * 1)(job)
    blocks = int(lib.seam_repack_layout(arr, 1))
    assert blocks > 0
    table = ops._upload(arr, torch.device(DEV))
    _native.check(lib.seam_repack_many_f32(ops._ptr(table), 1, blocks, ops._stream()), "seam_repack_many_f32")
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert np.array_equal(unpack_planes(b, k, c)[0].view(np.uint32), pieces_np(w.view(k, c).cpu().numpy())[0].view(np.uint32))


@gpu
def test_model_level_switches():
    """A body forward on two 64 x 96 images: the new kernel on (every supported shape, the rule's override) and off give the same
    bits; set_split_f32(False) equals the process switch SPLIT_F32 = False bit for bit."""
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
    rule, on_flag, split = ops.SXPC_RULE, ops.SXPC, det.SPLIT_F32
    try:
        with torch.no_grad():
            ops.SXPC_RULE, ops.SXPC = False, True
            ops.CONV_TRACE = []
            on = body(x)
            names = [t[0] for t in ops.CONV_TRACE]
            ops.CONV_TRACE = None
            assert names.count("conv1x1_sxpc") >= 10, names
            ops.SXPC = False
            ops.CONV_TRACE = []
            off = body(x)
            assert "conv1x1_sxpc" not in [t[0] for t in ops.CONV_TRACE]
            ops.CONV_TRACE = None
            ops.SXPC = True
            for a, b in zip(on, off):
                assert torch.equal(a, b)
            det.set_split_f32(body, False)
            by_attr = body(x)
            det.set_split_f32(body, True)
            det.SPLIT_F32 = False
            by_switch = body(x)
            for a, b in zip(by_attr, by_switch):
                assert torch.equal(a, b)
            assert any(not torch.equal(a, b) for a, b in zip(on, by_attr))
    finally:
        ops.SXPC_RULE, ops.SXPC, det.SPLIT_F32, ops.CONV_TRACE = rule, on_flag, split, None
