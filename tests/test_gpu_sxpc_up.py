"""conv1x1_sxpc_up (csrc/seam_pwsx.hip): the split-bf16 producer / consumer 1x1 kernel with a nearest-upsampled coarse map as its
residual -- the FPN lateral plus the top-down merge in one launch.  Its contract is the bits of ``seam_conv1x1_sxpc`` (scale, shift,
no residual, no ReLU) followed by ``ops.upsample_add_`` and ReLU, so every kernel comparison is ``torch.equal``.

Only the epilogue's residual addresses differ from the plain kernel: the producers compute one coarse-map offset per tile pixel and
hand the table over through LDS.  The shapes aim at that table: an exact 2x ratio, non-integer ratios on both axes, the FPN's odd
level, tiles across several images (the multiply-high image rule), 1 x 1 maps (a tile of 128 images) and ``Wo == 1`` (both are
served), ragged M, three n-tiles, and a walk of more tiles than CUs (the table's two parities).  Every output lies between two
NaN-free guard regions checked after each launch; the coarse map has no rows the nearest rule does not reach, so it needs no poison."""
import math

import pytest
import torch

from test_gpu_sxpc import DEV, guarded, normal
from test_gpu_sxpc_dual import pack, plain

gpu = pytest.mark.gpu


def up(x, top, pc, scale=None, shift=None, relu=0):
    """seam_conv1x1_sxpc_up on x [N, Ho, Wo, C], top [N, rH, rW, K] -> [M, K]; the guards around the output are asserted"""
    from seam_match_rcnn_amd import _native, ops
    n, ho, wo, c = x.shape
    y, intact = guarded(n * ho * wo, pc.K)
    _native.check(_native.lib().seam_conv1x1_sxpc_up(ops._ptr(x), ops._ptr(pc.wx), ops._ptr(scale), ops._ptr(shift), ops._ptr(top), ops._ptr(y),
                                                     n, ho, wo, c, pc.K, top.shape[1], top.shape[2], relu, ops._stream()), "seam_conv1x1_sxpc_up")
    torch.cuda.synchronize()
    assert intact(), "guard bytes around the output were written"
    return y


def unfused(x, top, pc, scale=None, shift=None, relu=0):
    """the reference: seam_conv1x1_sxpc (scale, shift), then ops.upsample_add_, then ReLU"""
    from seam_match_rcnn_amd import ops
    n, ho, wo, c = x.shape
    y = plain(x.reshape(n * ho * wo, c), pc, scale=scale, shift=shift)
    ops.upsample_add_(y.view(n, ho, wo, pc.K), top)
    return torch.relu(y) if relu else y


def maps(n, ho, wo, rh, rw, c, k, seed=7):
    return normal(seed, (n, ho, wo, c)).to(DEV), normal(seed + 1, (n, rh, rw, k)).to(DEV)


def check_equal(n, ho, wo, rh, rw, c=256, k=128, **kw):
    _, pc = pack(c, k)
    x, top = maps(n, ho, wo, rh, rw, c, k)
    ref = unfused(x, top, pc, **kw)
    y = up(x, top, pc, **kw)
    assert bool(torch.isfinite(ref).all())
    assert torch.equal(ref, y), ((n, ho, wo, rh, rw, c, k), int((ref != y).sum()))


@gpu
@pytest.mark.parametrize("geo", [
    (1, 16, 16, 8, 8, 256, 128),        # exact 2x, two tiles
    (3, 5, 7, 3, 4, 320, 256),          # an odd chunk count, M = 105 ragged, a tile across (more than) three images
    (2, 25, 25, 13, 13, 256, 128),      # the FPN's odd level
    (1, 13, 9, 5, 4, 256, 128),         # non-integer ratios on both axes
    (300, 1, 1, 1, 1, 256, 128),        # 1 x 1 maps: a tile of 128 images (served)
    (130, 3, 1, 2, 1, 256, 128),        # Wo == 1 (served)
    (1, 43, 3, 22, 2, 256, 384),        # three n-tiles, M = 129: one row past a tile
    (2, 7, 9, 7, 9, 256, 128),          # the same grid: ratio one
    (2, 4, 4, 9, 9, 256, 128),          # a coarse map LARGER than the output (the rule is ATen's for any ratio)
])
def test_equals_the_unfused_form(geo):
    n, ho, wo, rh, rw, c, k = geo
    check_equal(n, ho, wo, rh, rw, c, k)


@gpu
def test_a_walk_of_more_tiles_than_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert -(-(4 * 100 * 100) // 128) * 2 > 2 * cus
    check_equal(4, 100, 100, 50, 50, 256, 256, relu=1)


@gpu
@pytest.mark.parametrize("has_scale", [False, True])
@pytest.mark.parametrize("has_shift", [False, True])
@pytest.mark.parametrize("relu", [0, 1])
def test_epilogue_modes(has_scale, has_shift, relu):
    k = 256
    scale = (normal(41, (k,)).abs() + 0.5).to(DEV) if has_scale else None
    shift = normal(42, (k,)).to(DEV) if has_shift else None
    check_equal(3, 5, 7, 3, 4, 320, k, scale=scale, shift=shift, relu=relu)


@gpu
def test_launch_to_launch_and_batch_invariance():
    _, pc = pack(256, 128)
    x, top = maps(3, 7, 9, 4, 5, 256, 128, seed=61)
    shift = normal(63, (128,)).to(DEV)
    first = up(x, top, pc, shift=shift, relu=1)
    assert torch.equal(first, unfused(x, top, pc, shift=shift, relu=1))
    assert torch.equal(up(x, top, pc, shift=shift, relu=1), first)
    alone = up(x[1:2].contiguous(), top[1:2].contiguous(), pc, shift=shift, relu=1)      # the middle image alone
    assert torch.equal(alone, first[63:126])


@gpu
@pytest.mark.parametrize("name,args", [
    ("C=192", (2, 5, 7, 192, 128, 3, 4, 0)),
    ("K=192", (2, 5, 7, 256, 192, 3, 4, 0)),
    ("rH=0", (2, 5, 7, 256, 128, 0, 4, 0)),
    ("relu=2", (2, 5, 7, 256, 128, 3, 4, 2)),
    ("null top", (2, 5, 7, 256, 128, 3, 4, 0)),
    ("three coarse images of 2.2 GB under one tile", (3, 8, 8, 256, 128, 1200, 1200, 0)),
])
def test_refusals(name, args):
    """Refused on the host, nothing launched: the output keeps its sentinel.  (M != N Ho Wo cannot be said to the launch, which
    takes the grid; the predicate refuses it: tests/test_sxpc_up_host.py.)"""
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    x = torch.zeros((2, 5, 7, 256), device=DEV)
    top = torch.zeros((2, 3, 4, 128), device=DEV)
    w = torch.zeros((128 * 256 * 6,), dtype=torch.uint8, device=DEV)
    y, intact = guarded(70, 128)
    n, ho, wo, c, k, rh, rw, relu = args
    assert lib.seam_conv1x1_sxpc_up(ops._ptr(x), ops._ptr(w), None, None, None if name == "null top" else ops._ptr(top), ops._ptr(y),
                                    n, ho, wo, c, k, rh, rw, relu, ops._stream()) != 0, name
    torch.cuda.synchronize()
    assert intact() and bool(torch.isnan(y).all()), name
    # the accepted neighbour of every refusal
    assert lib.seam_conv1x1_sxpc_up(ops._ptr(x), ops._ptr(w), None, None, ops._ptr(top), ops._ptr(y), 2, 5, 7, 256, 128, 3, 4, 0, ops._stream()) == 0
    torch.cuda.synchronize()
    assert intact() and bool((y == 0).all())


def gate_errors(x, top, wt, shift):
    """(e_split, e_exact): e = max|y - y64| / max|y64| against the float64 lateral + merge; e_exact from the exact conv2d_topdown"""
    from seam_match_rcnn_amd import ops
    n, ho, wo, c = x.shape
    k = wt.shape[0]
    rh, rw = top.shape[1], top.shape[2]
    ih = torch.clamp(torch.floor(torch.arange(ho, dtype=torch.float32) * (torch.tensor(float(rh)) / torch.tensor(float(ho)))).long(), max=rh - 1)
    iw = torch.clamp(torch.floor(torch.arange(wo, dtype=torch.float32) * (torch.tensor(float(rw)) / torch.tensor(float(wo)))).long(), max=rw - 1)
    ref = (x.cpu().double().reshape(-1, c) @ wt.double().t() + shift.double()).view(n, ho, wo, k) + top.cpu().double()[:, ih][:, :, iw]
    ps = ops.pack_conv(wt.view(k, c, 1, 1).to(DEV), shift.to(DEV), dtype=ops.SX6)
    pe = ops.pack_conv(wt.view(k, c, 1, 1).to(DEV), shift.to(DEV), wino=False)
    ys = up(x, top, ps, shift=ps.shift).view(n, ho, wo, k)
    ye = ops.conv2d_topdown(x, pe, top)
    scale = float(ref.abs().max())
    return float((ys.cpu().double() - ref).abs().max()) / scale, float((ye.cpu().double() - ref).abs().max()) / scale


GATE_SHAPES = [(2, 10, 10, 5, 5, 256, 128), (2, 4, 4, 2, 2, 1024, 256)]


@gpu
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_accuracy_gate(shape):
    """The rule of tests/test_gpu_split_f32.py: e_split <= 2 e_exact + 1e-7."""
    n, ho, wo, rh, rw, c, k = shape
    x, top = maps(n, ho, wo, rh, rw, c, k, seed=11)
    e_split, e_exact = gate_errors(x, top, normal(13, (k, c)) / math.sqrt(c), normal(14, (k,)) * 0.1)
    print(f"sxpc up gate {shape}: e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


@gpu
@pytest.mark.parametrize("shape", GATE_SHAPES)
def test_accuracy_gate_on_cancelling_input(shape):
    """Channel pairs (v, -v (1 + 2^-12)) against equal weights: the leading terms of each pair vanish."""
    n, ho, wo, rh, rw, c, k = shape
    v = normal(21, (n, ho, wo, c // 2))
    x = torch.stack([v, -v * (1.0 + 2.0 ** -12)], -1).reshape(n, ho, wo, c).to(DEV)
    wh = normal(23, (k, c // 2)) / math.sqrt(c)
    wt = torch.stack([wh, wh], -1).reshape(k, c)
    top = (normal(24, (n, rh, rw, k)) * 2.0 ** -10).to(DEV)       # (small: the cancelled products stay visible beside it)
    e_split, e_exact = gate_errors(x, top, wt, torch.zeros(k))
    print(f"sxpc up gate cancelling {shape}: e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


# ------------------------------------------------------------------------------------------------ ops and model level
class knobs:
    """ops.SXPC_RULE off (the tiny shapes below are under the tile rule) and whatever the block changes restored"""

    def __enter__(self):
        from seam_match_rcnn_amd import ops
        from seam_match_rcnn_amd.models import detection as det
        self.saved = (ops.SXPC_RULE, ops.SXPC, det.SPLIT_CLASSES)
        ops.SXPC_RULE = False
        return self

    def __exit__(self, *exc):
        from seam_match_rcnn_amd import ops
        from seam_match_rcnn_amd.models import detection as det
        ops.SXPC_RULE, ops.SXPC, det.SPLIT_CLASSES = self.saved
        ops.CONV_TRACE = None
        return False


def traced(fn):
    from seam_match_rcnn_amd import ops
    ops.CONV_TRACE = []
    try:
        out = fn()
        return out, [t[0] for t in ops.CONV_TRACE]
    finally:
        ops.CONV_TRACE = None


@gpu
def test_ops_route_and_fallbacks_give_the_same_bits():
    """ops.conv2d_topdown on an SX6 pack: the kernel (trace label conv1x1_sxpc_up); under the tile rule and with ops.SXPC off,
    conv2d + upsample_add_ on the same pack."""
    from seam_match_rcnn_amd import ops
    wt = (normal(31, (256, 512, 1, 1)) / 22).to(DEV)
    bias = normal(32, (256,)).to(DEV)
    exact, split = ops.pack_conv(wt, bias, dtype=(torch.float32, ops.SX6))
    assert exact.dtype == torch.float32 and split.dtype == ops.SX6 and split.wx is not None
    assert split.shift.data_ptr() == exact.shift.data_ptr() == bias.data_ptr()
    x, top = maps(2, 9, 11, 5, 6, 512, 256, seed=35)
    with knobs():
        on, names = traced(lambda: ops.conv2d_topdown(x, split, top))
        assert names == ["conv1x1_sxpc_up"], names
        ops.SXPC_RULE = True                    # 2 x 99 rows: two tiles, far below SXPC_MIN_TILES
        ruled, names = traced(lambda: ops.conv2d_topdown(x, split, top))
        assert len(names) == 1 and names[0].startswith("conv_igemm_sx<"), names
        ops.SXPC_RULE, ops.SXPC = False, False
        off, names = traced(lambda: ops.conv2d_topdown(x, split, top))
        assert len(names) == 1 and names[0].startswith("conv_igemm_sx<"), names
    assert torch.equal(on, ruled) and torch.equal(on, off)
    ye = ops.conv2d_topdown(x, exact, top)
    assert float((on - ye).abs().max()) <= 1e-5 * float(ye.abs().max())


def make_fpn():
    from seam_match_rcnn_amd.models import detection as det
    torch.manual_seed(5)
    return det.FeaturePyramidNetwork().to(DEV).eval()


def pyramid():
    """the body's four maps of two 64 x 64 frames"""
    return [normal(70 + i, (2, 16 >> i, 16 >> i, 256 << i)).to(DEV) for i in range(4)]


def fpn_by_hand(fpn, feats, inner):
    """the single-stream walk of FeaturePyramidNetwork.forward with the lateral packs ``inner``, the merge un-fused for SX6 packs"""
    from seam_match_rcnn_amd import ops
    layer = fpn.packed()[1]
    merge = lambda x, pc, top: (ops.upsample_add_(ops.conv2d(x, pc), top) if pc.dtype == ops.SX6 else ops.conv2d_topdown(x, pc, top))
    last = ops.conv2d(feats[3], inner[3])
    outs = [None, None, None, ops.conv2d(last, layer[3])]
    for i in (2, 1, 0):
        last = merge(feats[i], inner[i], last)
        outs[i] = ops.conv2d(last, layer[i])
    return outs


def same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@gpu
def test_fpn_switches():
    from seam_match_rcnn_amd.models import detection as det
    assert "lat" in det.SPLIT_CLASSES
    fpn, feats = make_fpn(), pyramid()
    run = lambda: [v for k, v in fpn(feats).items() if k != "pool"]
    with knobs():
        with torch.no_grad():
            on, names = traced(run)
            exact_packs, _, twins = fpn.packed()
            assert twins is not None and all(t.dtype == "bf16x6" and t.wx is not None for t in twins)
            assert sorted(n for n in names if n.startswith("conv1x1_sxpc")) == ["conv1x1_sxpc", "conv1x1_sxpc_up", "conv1x1_sxpc_up", "conv1x1_sxpc_up"], names
            assert same(on, fpn_by_hand(fpn, feats, twins))
            today = fpn_by_hand(fpn, feats, exact_packs)
            assert any(not torch.equal(a, b) for a, b in zip(on, today))
            det.SPLIT_CLASSES = det.SPLIT_CLASSES - {"lat"}
            without, names = traced(run)
            assert fpn.packed()[2] is None and not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names), names
            assert same(without, today)
            det.SPLIT_CLASSES = det.SPLIT_CLASSES | {"lat"}
            det.set_split_f32(fpn, False)
            off, names = traced(run)
            assert not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names), names
            assert same(off, today)
            det.set_split_f32(fpn, True)
            fpn.train()
            training, names = traced(run)
            assert not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names), names
            assert same(training, today)
            fpn.eval()
        graded, names = traced(run)             # under grad: the exact kernels
        assert not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names), names
        assert same(graded, today)
        with torch.no_grad():
            assert same(run(), on)


@gpu
def test_mask_predictor_switches():
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    assert "mdeconv" in det.SPLIT_CLASSES
    torch.manual_seed(6)
    mp = det.MaskRCNNPredictor(256, 256, 14).to(DEV).eval()
    x = normal(80, (3, 14, 14, 256)).to(DEV)
    run = lambda: mp(x)

    def by_hand(up_pack):
        y = ops.conv2d(x, up_pack, relu=True)
        return ops.linear(y.view(3 * 14 * 14 * 4, -1), mp._pk[1]).view(3, 14, 14, 4 * 14)
    with knobs():
        with torch.no_grad():
            on, names = traced(run)
            ups = mp._pk[0]
            assert len(ups) == 2 and ups[1].dtype == ops.SX6 and ups[1].w is not None and ups[1].wx is not None
            assert names[0] == "conv1x1_sxpc", names
            today = by_hand(ups[0])
            assert torch.equal(on, by_hand(ups[1])) and not torch.equal(on, today)
            assert float((on - today).abs().max()) <= 1e-5 * float(today.abs().max())
            det.SPLIT_CLASSES = det.SPLIT_CLASSES - {"mdeconv"}
            without, names = traced(run)
            assert len(mp._pk[0]) == 1 and not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names), names
            assert torch.equal(without, today)
            det.SPLIT_CLASSES = det.SPLIT_CLASSES | {"mdeconv"}
            det.set_split_f32(mp, False)
            off, names = traced(run)
            assert not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names) and torch.equal(off, today), names
            det.set_split_f32(mp, True)
            mp.train()
            training, names = traced(run)
            assert not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names) and torch.equal(training, today), names
            mp.eval()
        graded, names = traced(run)
        assert not any(n.startswith(("conv1x1_sxpc", "conv_igemm_sx")) for n in names) and torch.equal(graded, today), names
        with torch.no_grad():
            assert torch.equal(run(), on)
            # the kernel and the implicit GEMM on the twin give the same bits (the route may look at the batch)
            ops.SXPC = False
            assert torch.equal(run(), on)


@gpu
def test_pack_plan_refreshes_the_lateral_twins_in_place():
    """One optim.SGD step on the FPN: the plan refreshes the twins with its SPLIT3 and SXPC jobs; their bytes equal a fresh pack's."""
    from seam_match_rcnn_amd.models import detection as det
    from seam_match_rcnn_amd.optim import SGD

    class Holder(torch.nn.Module):
        def __init__(self, fpn):
            super().__init__()
            self.backbone = torch.nn.Module()
            self.backbone.fpn = fpn
    fpn, feats = make_fpn(), pyramid()
    params = list(fpn.parameters())
    opt = SGD(params, lr=0.01, momentum=0.9, model=Holder(fpn))
    plan = opt.plan
    twins = fpn.packed()[2]
    old = [(t.w.clone(), t.wx.clone()) for t in twins]
    for i, p in enumerate(params):
        p.grad = (normal(100 + i, tuple(p.shape)) * 0.1).to(DEV)
    opt.step()
    assert (plan.refreshes, plan.rebuilds, plan.launches_per_refresh) == (1, 0, 1)
    assert fpn.packed()[2] is twins
    assert all(not torch.equal(t.w, w) and not torch.equal(t.wx, wx) for t, (w, wx) in zip(twins, old))
    fresh = det.FeaturePyramidNetwork()
    fresh.load_state_dict(fpn.state_dict())
    fresh = fresh.to(DEV).eval()
    for f, t in zip(fresh.packed()[2], twins):
        assert torch.equal(f.w, t.w) and torch.equal(f.wx, t.wx) and torch.equal(f.shift, t.shift)
    with knobs(), torch.no_grad():
        assert same(list(fpn(feats).values()), list(fresh(feats).values()))
