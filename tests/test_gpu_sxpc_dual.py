"""conv1x1_sxpc_dual (csrc/seam_pwsx.hip): the two-source form of the split-bf16 producer / consumer kernel -- a projection-shortcut
block, ``bn3(conv3(h)) + bn_d(conv_d(x))``, as ONE reduction over ``[x1 | x2 sampled at stride2]``.  Its contract is the bits of
``seam_conv1x1_sxpc`` on the materialised concatenation (itself the bits of ``seam_conv2d_sx`` with six terms:
tests/test_gpu_sxpc.py), so every comparison is ``torch.equal``.

Only the producers know the two sources, so the shapes below aim at them: odd and even x2 maps, stride 1 and 2, a 1 x 1 map (one
image per output row), maps of fewer than 128 pixels (a tile spans several images: the multiply-high division) and of more (at most
two: the compare), ragged M, both orders of a long and a short source, a persistent walk, an x2 beyond 4 GiB.  Every x2 is NaN at
the pixels the stride skips, and every output of the new entry lies between two guard regions checked after each launch."""
import math

import numpy as np
import pytest
import torch

from test_gpu_sxpc import DEV, SPECIAL, TILE, guarded, normal

gpu = pytest.mark.gpu
_PACKS = {}


def pack(c, k, seed=3):
    """(weight [k, c] on the host, its SX6 pack), cached: packs are read only"""
    from seam_match_rcnn_amd import ops
    if (c, k, seed) not in _PACKS:
        wt = normal(seed, (k, c)) / math.sqrt(c)
        pc = ops.pack_conv(wt.view(k, c, 1, 1).to(DEV), dtype=ops.SX6)
        assert pc.wx is not None
        _PACKS[(c, k, seed)] = (wt, pc)
    return _PACKS[(c, k, seed)]


def sources(n, ho, wo, h2, w2, c1, c2, s, seed=7):
    """x1 [n, ho, wo, c1] and x2 [n, h2, w2, c2] on the device; x2 is NaN wherever the stride does not sample it"""
    x1 = normal(seed, (n, ho, wo, c1)).to(DEV)
    x2 = torch.full((n, h2, w2, c2), float("nan"), device=DEV)
    x2[:, :(ho - 1) * s + 1:s, :(wo - 1) * s + 1:s] = normal(seed + 1, (n, ho, wo, c2)).to(DEV)
    return x1, x2


def cat_rows(x1, x2, s):
    n, ho, wo, _ = x1.shape
    return torch.cat([x1, x2[:, :(ho - 1) * s + 1:s, :(wo - 1) * s + 1:s]], -1).reshape(n * ho * wo, -1).contiguous()


def plain(rows, pc, scale=None, shift=None, relu=0):
    """seam_conv1x1_sxpc on materialised rows [M, C]: the reference"""
    from seam_match_rcnn_amd import _native, ops
    y = torch.full((rows.shape[0], pc.K), float("nan"), device=DEV)
    _native.check(_native.lib().seam_conv1x1_sxpc(ops._ptr(rows), ops._ptr(pc.wx), ops._ptr(scale), ops._ptr(shift), None, ops._ptr(y),
                                                  rows.shape[0], rows.shape[1], pc.K, relu, ops._stream()), "seam_conv1x1_sxpc")
    return y


def dual(x1, x2, pc, s, scale=None, shift=None, relu=0):
    """seam_conv1x1_sxpc_dual -> [M, K]; the guards around the output are asserted"""
    from seam_match_rcnn_amd import _native, ops
    n, ho, wo, c1 = x1.shape
    _, h2, w2, c2 = x2.shape
    y, intact = guarded(n * ho * wo, pc.K)
    _native.check(_native.lib().seam_conv1x1_sxpc_dual(ops._ptr(x1), ops._ptr(x2), ops._ptr(pc.wx), ops._ptr(scale), ops._ptr(shift), ops._ptr(y),
                                                       n, ho, wo, c1, h2, w2, c2, s, pc.K, relu, ops._stream()), "seam_conv1x1_sxpc_dual")
    torch.cuda.synchronize()
    assert intact(), "guard bytes around the output were written"
    return y


def check_equal(n, ho, wo, h2, w2, s, c1=64, c2=192, k=128, **kw):
    _, pc = pack(c1 + c2, k)
    x1, x2 = sources(n, ho, wo, h2, w2, c1, c2, s)
    ref = plain(cat_rows(x1, x2, s), pc, **kw)
    y = dual(x1, x2, pc, s, **kw)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(ref, y), ((n, ho, wo, h2, w2, s, c1, c2, k), int((ref != y).sum()))


@gpu
@pytest.mark.parametrize("geo", [(2, 5, 7, 10, 13), (3, 9, 9, 17, 18), (1, 1, 1, 1, 1)])
def test_stride_two_on_odd_and_even_maps(geo):
    check_equal(*geo, 2)


@gpu
@pytest.mark.parametrize("geo", [(2, 5, 7, 5, 7), (3, 9, 9, 9, 9), (1, 1, 1, 1, 1), (2, 12, 13, 12, 13)])
def test_stride_one_on_the_same_map(geo):
    check_equal(*geo, 1)


@gpu
@pytest.mark.parametrize("k", [128, 384])
@pytest.mark.parametrize("c1,c2", [(64, 192), (192, 64), (128, 256), (256, 64)])
def test_source_widths_and_output_widths(c1, c2, k):
    check_equal(2, 5, 7, 10, 13, 2, c1=c1, c2=c2, k=k)
    check_equal(2, 12, 13, 24, 25, 2, c1=c1, c2=c2, k=k)        # 156 pixels per image: the two-images-per-tile path, two tiles


@gpu
@pytest.mark.parametrize("geo", [
    (1, 1, 1, 1, 1, 1),             # M = 1
    (127, 1, 1, 2, 3, 2),           # M = 127: one image per row (HoWo = 1)
    (129, 1, 1, 1, 1, 1),           # M = 129: the same, two tiles
    (1, 127, 1, 253, 2, 2),         # M = 127 in one image, Wo = 1
    (3, 43, 1, 86, 1, 2),           # M = 129 over three images
    (5, 6, 6, 11, 12, 2),           # a tile that spans more than three images
    (1, 10, 13, 20, 26, 2),         # M = 130 in one image: HoWo >= 128
])
def test_ragged_m_and_tiles_across_images(geo):
    n, ho, wo, h2, w2, s = geo
    check_equal(n, ho, wo, h2, w2, s)


@gpu
def test_persistent_walk_of_more_than_three_tiles_per_cu():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n, ho, wo, k = 10, 41, 41, 1024
    tiles = -(-(n * ho * wo) // TILE) * (k // 128)
    assert tiles > 3 * cus and tiles % cus != 0, (tiles, cus)
    check_equal(n, ho, wo, 82, 81, 2, k=k)


@gpu
def test_fewer_tiles_than_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 2 * 3 < cus
    check_equal(1, 11, 13, 21, 26, 2, c1=128, c2=192, k=384)        # 143 rows: six tiles, an odd number of chunks


@gpu
@pytest.mark.parametrize("mode", ["none", "shift", "scale_shift", "relu", "all"])
def test_epilogue_modes(mode):
    k = 384
    scale = (normal(41, (k,)).abs() + 0.5).to(DEV) if mode in ("scale_shift", "all") else None
    shift = normal(42, (k,)).to(DEV) if mode in ("shift", "scale_shift", "all") else None
    check_equal(3, 9, 9, 17, 18, 2, k=k, scale=scale, shift=shift, relu=1 if mode in ("relu", "all") else 0)


@gpu
def test_piece_identity():
    """The special values of tests/test_gpu_sxpc.py through a 256 x 256 identity, 64 channels from x1 and 192 from x2: all values in
    one pixel, and one value per pixel of a 16 x 16 map sampled from 31 x 31; the outputs are the inputs."""
    from seam_match_rcnn_amd import ops
    vals = SPECIAL.repeat(8)
    pc = ops.pack_conv(torch.eye(256).view(256, 256, 1, 1).to(DEV), dtype=ops.SX6)
    for rows, (ho, wo, h2, w2, s) in ((vals.view(1, 256), (1, 1, 1, 1, 1)), (torch.diag(vals), (16, 16, 31, 31, 2))):
        x1 = rows[:, :64].reshape(1, ho, wo, 64).contiguous().to(DEV)
        x2 = torch.full((1, h2, w2, 192), float("nan"), device=DEV)
        x2[:, ::s, ::s] = rows[:, 64:].reshape(1, ho, wo, 192).to(DEV)
        y = dual(x1, x2, pc, s)
        wrong = (y.cpu().double() != rows.double()).nonzero().tolist()
        print(f"sxpc dual identity {tuple(rows.shape)}: wrong at {wrong[:8]}")
        assert torch.equal(y.cpu().double(), rows.double())


@gpu
def test_launch_to_launch_and_batch_invariance():
    _, pc = pack(256, 128)
    x1, x2 = sources(3, 7, 9, 14, 17, 64, 192, 2, seed=61)
    shift = normal(63, (128,)).to(DEV)
    first = dual(x1, x2, pc, 2, shift=shift, relu=1)
    assert torch.equal(first, plain(cat_rows(x1, x2, 2), pc, shift=shift, relu=1))
    for _ in range(49):
        assert torch.equal(dual(x1, x2, pc, 2, shift=shift, relu=1), first)
    alone = dual(x1[1:2].contiguous(), x2[1:2].contiguous(), pc, 2, shift=shift, relu=1)       # the middle image alone
    assert torch.equal(alone, first[63:126])


@gpu
def test_x2_beyond_four_gib():
    """18 images of 250 x 250 x 1024 fp32 are 4.6 GB: the second source's descriptor is rebased per tile, lane offsets stay 32-bit.
    The last two images (their x2 pixels lie past 4 GiB) against the reference on their slice."""
    n, ho, wo, h2, w2, c1, c2, k, s = 18, 125, 125, 250, 250, 64, 1024, 128, 2
    _, pc = pack(c1 + c2, k)
    x2 = torch.empty((n, h2, w2, c2), device=DEV)
    assert x2.numel() * 4 > 1 << 32
    x2.normal_(generator=torch.Generator(device=DEV).manual_seed(5))
    x1 = torch.empty((n, ho, wo, c1), device=DEV).normal_(generator=torch.Generator(device=DEV).manual_seed(6))
    y = dual(x1, x2, pc, s)
    ref = plain(cat_rows(x1[16:], x2[16:], s), pc)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(y[16 * ho * wo:], ref)
    assert bool(torch.isfinite(y).all())


@gpu
@pytest.mark.parametrize("name,args", [
    ("C1=32", (2, 5, 7, 32, 10, 13, 256, 2, 128, 0)),
    ("C1+C2=192", (2, 5, 7, 64, 10, 13, 128, 2, 128, 0)),
    ("K=96", (2, 5, 7, 64, 10, 13, 192, 2, 96, 0)),
    ("(Ho-1)*s == H2", (2, 5, 7, 64, 8, 13, 192, 2, 128, 0)),
    ("(Wo-1)*s == W2", (2, 5, 7, 64, 10, 12, 192, 2, 128, 0)),
    ("stride2=0", (2, 5, 7, 64, 10, 13, 192, 0, 128, 0)),
    ("relu=2", (2, 5, 7, 64, 10, 13, 192, 2, 128, 2)),
])
def test_refusals(name, args):
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    x1 = torch.zeros((2, 5, 7, 64), device=DEV)
    x2 = torch.zeros((2, 10, 13, 256), device=DEV)
    w = torch.zeros((128 * 320 * 6,), dtype=torch.uint8, device=DEV)
    y, intact = guarded(70, 128)
    n, ho, wo, c1, h2, w2, c2, s, k, relu = args
    assert lib.seam_conv1x1_sxpc_dual(ops._ptr(x1), ops._ptr(x2), ops._ptr(w), None, None, ops._ptr(y), n, ho, wo, c1, h2, w2, c2, s, k, relu,
                                      ops._stream()) != 0, name
    torch.cuda.synchronize()
    assert intact() and bool(torch.isnan(y).all()), name
    # the accepted neighbour of every refusal
    assert lib.seam_conv1x1_sxpc_dual(ops._ptr(x1), ops._ptr(x2), ops._ptr(w), None, None, ops._ptr(y), 2, 5, 7, 64, 10, 13, 192, 2, 128, 0,
                                      ops._stream()) == 0
    torch.cuda.synchronize()
    assert intact() and bool((y == 0).all())


def gate_errors(x1, x2, wt, shift, s):
    """(e_split, e_exact): e = max|y - y64| / max|y64| against the float64 folded two-source product; e_exact from
    seam_conv2d_dual_f32 on the same operands"""
    from seam_match_rcnn_amd import _native, ops
    n, ho, wo, c1 = x1.shape
    _, h2, w2, c2 = x2.shape
    k = wt.shape[0]
    ref = cat_rows(x1, x2, s).cpu().double() @ wt.double().t() + shift.double()
    ps = ops.pack_conv(wt.view(k, c1 + c2, 1, 1).to(DEV), shift.to(DEV), dtype=ops.SX6)
    pe = ops.pack_conv(wt.view(k, c1 + c2, 1, 1).to(DEV), shift.to(DEV), wino=False)
    ys = dual(x1, x2, ps, s, shift=ps.shift)
    ye = torch.empty((n * ho * wo, k), device=DEV)
    _native.check(_native.lib().seam_conv2d_dual_f32(ops._ptr(x1), ops._ptr(x2), ops._ptr(pe.w), None, ops._ptr(pe.shift), ops._ptr(ye),
                                                     n, ho, wo, c1, h2, w2, c2, s, k, 0, ops._stream()), "seam_conv2d_dual_f32")
    scale = float(ref.abs().max())
    return float((ys.cpu().double() - ref).abs().max()) / scale, float((ye.cpu().double() - ref).abs().max()) / scale


GATE_SHAPES = [(2, 10, 10, 20, 20, 128, 256, 512), (2, 4, 4, 7, 7, 512, 1024, 2048)]


@gpu
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_accuracy_gate(shape):
    """The rule of tests/test_gpu_split_f32.py: e_split <= 2 e_exact + 1e-7."""
    n, ho, wo, h2, w2, c1, c2, k = shape
    x1, x2 = sources(n, ho, wo, h2, w2, c1, c2, 2, seed=11)
    wt = normal(13, (k, c1 + c2)) / math.sqrt(c1 + c2)
    e_split, e_exact = gate_errors(x1, x2, wt, normal(14, (k,)) * 0.1, 2)
    print(f"sxpc dual gate {shape}: e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


@gpu
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_accuracy_gate_on_cancelling_input(shape):
    """Channel pairs (v, -v (1 + 2^-12)) against equal weights in both sources: the leading terms of each pair vanish."""
    n, ho, wo, h2, w2, c1, c2, k = shape

    def pairs(seed, c):
        v = normal(seed, (n, ho, wo, c // 2))
        return torch.stack([v, -v * (1.0 + 2.0 ** -12)], -1).reshape(n, ho, wo, c)
    x1 = pairs(21, c1).to(DEV)
    x2 = torch.full((n, h2, w2, c2), float("nan"), device=DEV)
    x2[:, ::2, ::2] = pairs(22, c2).to(DEV)
    wh = normal(23, (k, (c1 + c2) // 2)) / math.sqrt(c1 + c2)
    wt = torch.stack([wh, wh], -1).reshape(k, c1 + c2)
    e_split, e_exact = gate_errors(x1, x2, wt, torch.zeros(k), 2)
    print(f"sxpc dual gate cancelling {shape}: e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


@gpu
def test_ops_route_and_fallback_give_the_same_bits():
    """ops.conv2d_dual on an SX6 pack: the kernel (trace label conv1x1_sxpc_dual) and, with ops.SXPC off, gather + concatenate +
    conv_igemm_sx on the same pack."""
    from seam_match_rcnn_amd import ops
    bn = lambda seed, k: (normal(seed, (k,)).abs() + 0.5, normal(seed + 1, (k,)), normal(seed + 2, (k,)), normal(seed + 3, (k,)).abs() + 0.5)
    k, c1, c2 = 256, 64, 192
    w1, w2 = (normal(31, (k, c1, 1, 1)) / 8).to(DEV), (normal(32, (k, c2, 1, 1)) / 14).to(DEV)
    b1, b2 = tuple(t.to(DEV) for t in bn(33, k)), tuple(t.to(DEV) for t in bn(37, k))
    exact, split = ops.pack_conv_dual(w1, b1, w2, b2, dtype=(torch.float32, ops.SX6))
    assert split.dtype == ops.SX6 and split.w is not None and split.wx is not None and exact.dtype == torch.float32
    assert split.shift.data_ptr() == exact.shift.data_ptr()
    alone = ops.pack_conv_dual(w1, b1, w2, b2, dtype=ops.SX6)
    assert torch.equal(alone.wx, split.wx) and torch.equal(alone.w, split.w)
    x1, x2 = sources(2, 9, 11, 18, 21, c1, c2, 2, seed=35)
    x2 = torch.nan_to_num(x2, nan=1e30)             # (the fallback's gather never reads them either)
    flag = ops.SXPC
    try:
        ops.CONV_TRACE = []
        on = ops.conv2d_dual(x1, x2, split, 2, relu=True)
        names = [t[0] for t in ops.CONV_TRACE]
        assert names == ["conv1x1_sxpc_dual"], names
        ops.SXPC = False
        ops.CONV_TRACE = []
        off = ops.conv2d_dual(x1, x2, split, 2, relu=True)
        names = [t[0] for t in ops.CONV_TRACE]
        assert len(names) == 1 and names[0].startswith("conv_igemm_sx<"), names
    finally:
        ops.SXPC, ops.CONV_TRACE = flag, None
    assert torch.equal(on, off)
    ye = ops.conv2d_dual(x1, x2, exact, 2, relu=True)
    assert float((on - ye).abs().max()) <= 1e-5 * float(ye.abs().max())


def make_body():
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models import detection as det
    pfx = "backbone.body."
    sd = {k[len(pfx):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items() if k.startswith(pfx)}
    body = det.ResNet50Body()
    body.load_state_dict(sd)
    return body.to(DEV).eval()


def frames():
    x = normal(91, (2, 64, 96, 4))
    x[..., 3] = 0
    return x.to(DEV)


def traced(body, x):
    from seam_match_rcnn_amd import ops
    ops.CONV_TRACE = []
    try:
        out = body(x)
        return out, list(ops.CONV_TRACE)
    finally:
        ops.CONV_TRACE = None


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@gpu
def test_model_level_switches():
    """The body on two 64 x 96 images.  The served blocks are layer2.0 / layer3.0 / layer4.0, at any batch; ops.SXPC off gives the same
    bits through the fallback; without the class c3ds the walk is the one before the class existed (the split twins of c1 / c2s2 /
    c3 and the exact dual GEMM); set_split_f32(False) is the exact kernels."""
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    body, x = make_body(), frames()
    classes, flag = det.SPLIT_CLASSES, ops.SXPC
    assert "c3ds" in classes

    def walk(split):
        """ResNet50Body._run with the dual blocks on their exact packs (split: the other classes' twins)"""
        pk = body.packed()
        t = body._stem(x, pk)
        outs = []
        for li, bi, b in body.blocks():
            e = pk[(li, bi)]
            if not split:
                t = det.body_block(t, e, b.stride)[0]
            else:
                o = ops.conv2d(t, e.get("c1x", e["c1"]), relu=True)
                o = ops.conv2d(o, e.get("c2x", e["c2"]), relu=True)
                if "c3ds" in e:
                    t = ops.conv2d_dual(o, t, e["c3ds"], b.stride, relu=True)
                else:
                    t = ops.conv2d(o, e.get("c3x", e["c3"]), relu=True, residual=t)
            if bi == len(getattr(body, f"layer{li}")) - 1:
                outs.append(t)
        return outs
    try:
        with torch.no_grad():
            on, trace = traced(body, x)
            pk = body.packed()
            assert [key for key in pk if isinstance(key, tuple) and "c3dsx" in pk[key]] == [(2, 0), (3, 0), (4, 0)]
            served = [t[4] for t in trace if t[0] == "conv1x1_sxpc_dual"]
            assert served == [(2, 8, 12, 384, 512, 1, 1), (2, 4, 6, 768, 1024, 1, 1), (2, 2, 3, 1536, 2048, 1, 1)], served
            before = walk(split=True)
            assert any(not torch.equal(a, b) for a, b in zip(on, before))
            ops.SXPC = False
            off, trace = traced(body, x)
            assert not any(t[0].startswith("conv1x1_sxpc") for t in trace)
            ops.SXPC = flag
            assert same(on, off)
            det.SPLIT_CLASSES = classes - {"c3ds"}
            without, trace = traced(body, x)
            assert not any("c3dsx" in e for key, e in body.packed().items() if isinstance(key, tuple))
            assert not any(t[0] == "conv1x1_sxpc_dual" for t in trace)
            assert sum(t[0].startswith("conv_igemm<float") and t[4][3] in (384, 768, 1536) for t in trace) == 3
            assert same(without, before)
            det.SPLIT_CLASSES = classes
            det.set_split_f32(body, False)
            exact, trace = traced(body, x)
            assert not any(t[0].startswith(("conv1x1_sxpc", "conv_igemm_sx")) for t in trace)
            assert same(exact, walk(split=False))
            det.set_split_f32(body, True)
            assert same(body(x), on)
    finally:
        det.SPLIT_CLASSES, ops.SXPC = classes, flag


@gpu
def test_an_image_alone_equals_the_image_in_a_batch_through_the_body():
    body, x = make_body(), frames()
    with torch.no_grad():
        both = body(x)
        alone = body(x[1:2].contiguous())
    assert all(torch.equal(a[1:2], b) for a, b in zip(both, alone))


@gpu
def test_pack_plan_refreshes_the_split_twin_in_place():
    """One optim.SGD step on the body's layer2..layer4: the plan needs no new job form (SPLIT3 + SXPC jobs on the folded matrix, a
    derived source it shares with the exact pack): refresh() is in place and the forward equals a freshly packed body's."""
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    from seam_match_rcnn_amd.optim import SGD

    class Holder(torch.nn.Module):
        def __init__(self, body):
            super().__init__()
            self.backbone = torch.nn.Module()
            self.backbone.body = body
    body, x = make_body(), frames()
    for name, p in body.named_parameters():
        p.requires_grad_(name.startswith(("layer2", "layer3", "layer4")))
    params = [p for p in body.parameters() if p.requires_grad]
    opt = SGD(params, lr=0.01, momentum=0.9, model=Holder(body))
    plan = opt.plan
    twins = [body.packed()[key]["c3dsx"] for key in ((2, 0), (3, 0), (4, 0))]
    old = [(t.w.clone(), t.wx.clone()) for t in twins]
    n_derived = sum(any(d.requires_grad for d in deps) for _, _, deps in plan._derived)
    for i, p in enumerate(params):
        p.grad = (normal(100 + i, tuple(p.shape)) * 0.1).to(DEV)
    opt.step()
    assert (plan.refreshes, plan.rebuilds, plan.launches_per_refresh) == (1, 0, 1)
    assert plan.fallback_calls == n_derived == 3            # one folded matrix per shortcut block, whatever the number of its packs
    assert all(body.packed()[key]["c3dsx"] is t for key, t in zip(((2, 0), (3, 0), (4, 0)), twins))
    assert all(not torch.equal(t.w, w) and not torch.equal(t.wx, wx) for t, (w, wx) in zip(twins, old))
    fresh = det.ResNet50Body()
    fresh.load_state_dict(body.state_dict())
    fresh = fresh.to(DEV).eval()
    with torch.no_grad():
        got, trace = traced(body, x)
        want = fresh(x)
    assert sum(t[0] == "conv1x1_sxpc_dual" for t in trace) == 3
    assert same(got, want)
    for key, t in zip(((2, 0), (3, 0), (4, 0)), twins):
        f = fresh.packed()[key]["c3dsx"]
        assert torch.equal(f.w, t.w) and torch.equal(f.wx, t.wx) and torch.equal(f.shift, t.shift)
    # a second refresh through the plan's own entry returns True
    for p in params:
        with torch.no_grad():
            p.add_(0.001)
    assert plan.refresh(params) is True
    with torch.no_grad():
        fresh2 = det.ResNet50Body()
        fresh2.load_state_dict(body.state_dict())
        assert same(body(x), fresh2.to(DEV).eval()(x))
