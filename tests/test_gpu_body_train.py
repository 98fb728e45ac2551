"""GPU: training the ResNet body -- the two kernels of ``csrc/seam_body_train.hip`` and ``ResNet50Body.forward_taped`` /
``autograd.BodyFunction`` on the module alone.

References: ``F.conv2d(...).backward`` in float64 on the CPU for the stride-2 input gradient (tolerance: ``close`` of
tests/test_gpu_train.py, rtol 2e-4 and atol 2e-5 of the largest reference element), the torch expression itself for
``relu_mask_add`` (bit for bit), ``ResNet50Body.forward`` for the taped forward (bit for bit) and float64 autograd through
``oracle.detection.resnet50_body`` for the body's 52 weight gradients (``fpn_train_refs.compare_grads`` at its own 2e-3).
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_train_refs as FR
from oracle import detection as OD

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (N, H, W, C, K): odd x odd | even x even (the last row / column reach a tap that does not exist) | mixed | Ho = Wo = 1 twice |
# wider than one 128-pixel tile in every class | the layer's real channel count over three images
SHAPES = [(2, 7, 9, 32, 32), (1, 8, 10, 64, 32), (2, 13, 6, 32, 64), (1, 1, 1, 32, 32), (1, 2, 2, 32, 32), (1, 3, 70, 32, 32),
          (3, 25, 34, 128, 128)]


def close(got, want, rtol=2e-4, atol_frac=2e-5, msg=""):
    """``close`` of tests/test_gpu_train.py."""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    assert got.shape == want.shape, (got.shape, want.shape, msg)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_frac * (float(np.abs(want).max()) + 1e-30) + 1e-9, err_msg=msg)


@functools.lru_cache(maxsize=None)
def case(shape):
    """Operands of one shape and the float64 input gradients (without / with the scale), computed once and shared."""
    n, h, w, c, k = shape
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(shape, (1, 3, 5, 7, 11))))
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = torch.randn((n, ho, wo, k), generator=g)
    wt = torch.randn((k, c, 3, 3), generator=g) * 0.1
    scale = torch.rand((k,), generator=g) + 0.5
    mask = torch.randn((n, h, w, c), generator=g)
    flat = mask.view(-1)
    flat[::7] = 0.0                                              # y == 0 and the negative zero count as "not positive"
    flat[3::11] = -0.0
    refs = {}
    for with_scale in (False, True):
        x = torch.zeros((n, c, h, w), dtype=torch.float64, requires_grad=True)
        y = F.conv2d(x, wt.double(), None, 2, 1)
        assert tuple(y.shape[2:]) == (ho, wo)
        if with_scale:
            y = y * scale.double().view(1, -1, 1, 1)
        y.backward(dy.double().permute(0, 3, 1, 2))
        refs[with_scale] = x.grad.permute(0, 2, 3, 1).contiguous()
    return dict(dy=dy, w=wt, scale=scale, mask=mask, refs=refs)


@pytest.fixture(params=[1, 0], ids=["kernel", "composition"])
def selector(request):
    from seam_match_rcnn_amd import _native
    before = _native.get_option("SEAM_S2_DGRAD")
    _native.set_option("SEAM_S2_DGRAD", request.param)
    yield request.param
    _native.set_option("SEAM_S2_DGRAD", before)


@pytest.mark.parametrize("with_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("with_scale", [False, True], ids=["noscale", "scale"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_conv3x3s2_dgrad_vs_float64(shape, with_scale, with_mask, selector):
    from seam_match_rcnn_amd import ops
    n, h, w, c, k = shape
    cs = case(shape)
    want = cs["refs"][with_scale]
    if with_mask:
        want = torch.where(cs["mask"] > 0, want, torch.zeros_like(want))
    pk = ops.pack_conv3x3s2_dgrad(cs["w"].to(DEV), cs["scale"].to(DEV) if with_scale else None)
    dy, mask = cs["dy"].to(DEV), (cs["mask"].to(DEV) if with_mask else None)
    outs = []
    for _ in range(2):
        out = torch.full((n, h, w, c), float("nan"), device=DEV)           # an element nobody writes fails the comparison
        assert ops.conv3x3s2_dgrad(dy, pk, (h, w), mask=mask, out=out) is out
        outs.append(out)
    fresh = ops.conv3x3s2_dgrad(dy, pk, (h, w), mask=mask)
    err = float((outs[0].cpu().double() - want).abs().max())
    print(f"{shape} scale={with_scale} mask={with_mask} selector={selector}: max err {err:.3e} of {float(want.abs().max()):.3e}")
    close(outs[0], want.float(), msg=str(shape))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], fresh)          # a fixed summation order
    if with_mask:
        assert bool((outs[0][mask <= 0] == 0).all())


def test_conv3x3s2_dgrad_splits_a_large_batch_over_images(monkeypatch):
    from seam_match_rcnn_amd import ops, ops_train
    shape = SHAPES[0]
    n, h, w, c, k = shape
    cs = case(shape)
    pk = ops.pack_conv3x3s2_dgrad(cs["w"].to(DEV), cs["scale"].to(DEV))
    whole = ops.conv3x3s2_dgrad(cs["dy"].to(DEV), pk, (h, w), mask=cs["mask"].to(DEV))
    monkeypatch.setattr(ops_train, "WGRAD_MAX_OPERAND_BYTES", h * w * c * 4)                  # one image per launch
    parts = ops.conv3x3s2_dgrad(cs["dy"].to(DEV), pk, (h, w), mask=cs["mask"].to(DEV))
    assert torch.equal(whole, parts)
    monkeypatch.setattr(ops_train, "WGRAD_MAX_OPERAND_BYTES", h * w * c * 4 - 1)
    with pytest.raises(ValueError):
        ops.conv3x3s2_dgrad(cs["dy"].to(DEV), pk, (h, w))


def test_conv3x3s2_dgrad_refusals_write_nothing():
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    dy, wp, dx = torch.zeros((1, 2, 2, 32), device=DEV), torch.zeros((9, 32, 32), device=DEV), nan(1, 4, 4, 32)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    bad = [(0, 4, 4, 32, 32), (-1, 4, 4, 32, 32), (1, 0, 4, 32, 32), (1, 4, 0, 32, 32), (1, 4, 4, 48, 32), (1, 4, 4, 32, 40),
           (1, 4, 4, 0, 32), (1, 4, 4, 32, 0),
           (4096, 64, 64, 32, 32),                 # dx of exactly 2^31 bytes
           (1, 1, 1, 32, 32 << 24)]                # dy of 2^31 bytes
    for dims in bad:
        assert lib.seam_conv3x3s2_dgrad_f32(p(dy), p(wp), None, p(dx), *dims, st) != 0, dims
    assert lib.seam_conv3x3s2_dgrad_f32(None, p(wp), None, p(dx), 1, 4, 4, 32, 32, st) != 0
    assert lib.seam_conv3x3s2_dgrad_f32(p(dy), None, None, p(dx), 1, 4, 4, 32, 32, st) != 0
    assert lib.seam_conv3x3s2_dgrad_f32(p(dy), p(wp), None, None, 1, 4, 4, 32, 32, st) != 0
    wout = nan(9 * 32 * 32)
    assert lib.seam_pack_conv3x3s2_dgrad_f32(p(wp), None, p(wout), 40, 32, st) != 0
    assert lib.seam_pack_conv3x3s2_dgrad_f32(p(wp), None, p(wout), 32, 48, st) != 0
    assert lib.seam_pack_conv3x3s2_dgrad_f32(None, None, p(wout), 32, 32, st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dx).all()) and bool(torch.isnan(wout).all())
    # the wrapper: a dy that does not belong to the input size, a mask of another shape
    pk = ops.pack_conv3x3s2_dgrad(torch.zeros((32, 32, 3, 3), device=DEV))
    with pytest.raises(ValueError):
        ops.conv3x3s2_dgrad(dy, pk, (6, 4))
    with pytest.raises(ValueError):
        ops.conv3x3s2_dgrad(dy, pk, (4, 4), mask=torch.zeros((1, 4, 4, 64), device=DEV))
    with pytest.raises(_native.SeamNativeError):
        ops.pack_conv3x3s2_dgrad(torch.zeros((40, 32, 3, 3), device=DEV))


@pytest.mark.parametrize("shape", [(2, 33, 17, 64), (1, 1, 1, 4), (3, 129, 36)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("with_b", [False, True], ids=["a", "a+b"])
def test_relu_mask_add_bit_for_bit(shape, with_b):
    from seam_match_rcnn_amd import _native, ops
    g = torch.Generator().manual_seed(len(shape) * 100 + shape[-1])
    y, a, b = (torch.randn(shape, generator=g) for _ in range(3))
    y.view(-1)[::3] = 0.0
    y.view(-1)[1::5] = -0.0
    a.view(-1)[::4] = -0.0                                       # (-0) + (-0) stays a negative zero where y > 0
    b.view(-1)[::2] = -0.0
    want = torch.where(y > 0, a + b if with_b else a, torch.zeros(()))
    out = ops.relu_mask_add(y.to(DEV), a.to(DEV), b.to(DEV) if with_b else None)
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
    untouched = torch.full((8, 4), float("nan"), device=DEV)
    lib, p = _native.lib(), (lambda t: C.c_void_p(t.data_ptr()))
    st = torch.cuda.current_stream().cuda_stream
    z = torch.zeros((8, 4), device=DEV)
    assert lib.seam_relu_mask_add_f32(p(z), p(z), None, p(untouched), 0, 4, st) != 0
    assert lib.seam_relu_mask_add_f32(p(z), p(z), None, p(untouched), 8, 6, st) != 0
    assert lib.seam_relu_mask_add_f32(p(z), None, None, p(untouched), 8, 4, st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(untouched).all())


# ------------------------------------------------------------------------------ the module
H, W = 72, 104        # C2 18 x 26, C3 9 x 13, C4 5 x 7, C5 3 x 4: every stride-2 layer sees an odd and an even extent
PFX = "backbone.body."


def body_state():
    import seam_match_rcnn_amd.synth as synth
    return {k[len(PFX):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items()
            if k.startswith(PFX)}


def make_body(trainable=("layer1", "layer2", "layer3", "layer4")):
    from seam_match_rcnn_amd.models import detection as det
    body = det.ResNet50Body()
    body.load_state_dict(body_state())
    for name, p in body.named_parameters():
        p.requires_grad_(any(name.startswith(t) for t in trainable))
    return body.to(DEV)


def frames(n):
    g = torch.Generator().manual_seed(40 + n)
    x = torch.randn((n, H, W, 4), generator=g)
    x[..., 3] = 0                                                # NHWC4: the fourth channel is padding
    return x


def grads_of(body, x, ups):
    body.zero_grad(set_to_none=True)
    feats = body.forward_taped(x.to(DEV))
    sum((f * u.to(DEV)).sum() for f, u in zip(feats, ups)).backward()
    return feats, {k: p.grad.detach().clone() for k, p in body.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def body_runs():
    x = frames(2)
    body = make_body()
    with torch.no_grad():
        plain = body(x.to(DEV))
    g = torch.Generator().manual_seed(9)
    ups = [torch.randn(tuple(f.shape), generator=g) for f in plain]
    feats, first = grads_of(body, x, ups)
    _, second = grads_of(body, x, ups)
    return dict(x=x, ups=ups, plain=plain, feats=feats, first=first, second=second)


@pytest.mark.parametrize("n", [1, 4])
def test_forward_taped_equals_forward(n):
    body = make_body()
    x = frames(n).to(DEV)
    with torch.no_grad():
        plain = body(x)                                           # 4 images: two batch slices on two streams
    taped = body.forward_taped(x)
    via_call = body(x, taped=True)
    assert [tuple(t.shape[1:]) for t in taped] == [(18, 26, 256), (9, 13, 512), (5, 7, 1024), (3, 4, 2048)]
    for a, b, c in zip(plain, taped, via_call):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert all(t.requires_grad for t in taped) and not any(t.requires_grad for t in plain)


def test_body_gradients_vs_float64(body_runs):
    sd = body_state()
    first, second = body_runs["first"], body_runs["second"]
    keys = sorted(k for k in sd if k.startswith("layer") and k.endswith("weight") and sd[k].dim() == 4)
    assert len(keys) == 52 and sorted(first) == keys
    assert all(torch.equal(first[k], second[k]) for k in keys)                       # two backward passes, the same bits
    assert all(first[k].shape == sd[k].shape for k in keys)                          # ordinary OIHW .grad tensors
    P = {PFX + k: v.double() for k, v in sd.items()}
    for k in keys:
        P[PFX + k].requires_grad_(True)
    x64 = body_runs["x"][..., :3].double().permute(0, 3, 1, 2).contiguous()
    ref = OD.resnet50_body(x64, P)
    for f, r in zip(body_runs["plain"], ref):
        r = r.detach().permute(0, 2, 3, 1)
        assert float((f.cpu().double() - r).abs().max()) <= 1e-3 * float(r.abs().max())      # the bound of smoke()
    sum((r * u.double().permute(0, 3, 1, 2)).sum() for r, u in zip(ref, body_runs["ups"])).backward()
    FR.compare_grads(first, {k: P[PFX + k].grad for k in keys}, keys)


def test_only_layer4_trainable(body_runs):
    body = make_body(("layer4",))
    feats, got = grads_of(body, body_runs["x"], body_runs["ups"])
    assert sorted(got) == sorted(k for k in body_runs["first"] if k.startswith("layer4."))
    assert len(got) == 10
    for k in got:
        assert torch.equal(got[k], body_runs["first"][k]), k
    assert all(p.grad is None for k, p in body.named_parameters() if not k.startswith("layer4."))
    for a, b in zip(feats, body_runs["plain"]):
        assert torch.equal(a, b)
    # the tape starts at layer4.0: three blocks are kept, C2..C4 carry no tape, so no gradient can run below layer4.0
    assert feats[3].grad_fn.n_blocks == 3
    assert all(f.grad_fn is None and not f.requires_grad for f in feats[:3])
    assert body_runs["feats"][3].grad_fn.n_blocks == 16 and body_runs["feats"][0].grad_fn is not None


def test_frozen_body_has_no_tape_and_the_stem_is_refused(body_runs):
    body = make_body(())
    feats = body.forward_taped(body_runs["x"].to(DEV))
    assert all(f.grad_fn is None for f in feats) and all(torch.equal(a, b) for a, b in zip(feats, body_runs["plain"]))
    body = make_body(("conv1", "layer4"))
    with pytest.raises(NotImplementedError, match="backbone"):
        body.forward_taped(body_runs["x"].to(DEV))
    from seam_match_rcnn_amd.models import detection as det
    body = det.set_compute_dtype(make_body(), torch.float16)
    with pytest.raises(NotImplementedError, match="fp32 only"):
        body.forward_taped(body_runs["x"].to(DEV))
