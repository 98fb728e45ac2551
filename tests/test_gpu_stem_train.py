"""GPU: training the ResNet stem (opt-in, ``train_stem``) -- ``seam_maxpool3s2_relu_bwd_f32``, the cropped weight gradient
``seam_conv_wgrad_crop_f32``, ``autograd.BodyFunction`` with the stem in front on the module alone, and the model.

References and bounds
  pool adjoint     ``F.max_pool2d(torch.relu(z), 3, 2, 1).backward(dpool)`` on the CPU, ``torch.equal``: y lies on the grid k/4
                   and dpool on k/64 with |k| <= 256, so every sum of up to four terms is exact in fp32 and no tolerance is needed.
  cropped wgrad    float64 ``F.conv2d(...)[..., :Ho, :Wo].backward`` on the CPU under ``fpn_train_refs.wgrad_close``.
  module           ``ResNet50Body.forward`` for the taped forward (bit for bit); float64 autograd through
                   ``oracle.detection.resnet50_body`` for all 53 weight gradients under ``fpn_train_refs.compare_grads`` at its own
                   2e-3 (fp32 and float64 CPU autograd of stem + ReLU + pool differ by 3e-7 relative Frobenius in conv1's
                   gradient at this size, so ReLU and argmax flips do not threaten the bound); the two input forms of the frame
                   against each other under ``fpn_train_refs.wgrad_close``; a stem-frozen run for the 52 bottleneck gradients
                   (bit for bit).
The helpers of tests/test_gpu_body_train.py and tests/test_gpu_body_train_model.py are restated here.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fpn_train_refs as FR
import rpn_train_refs as PR
from oracle import detection as OD

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

# (N, H, W, C): a single cell | even x even | odd x even over two images | even x odd | a row wider than one 256-lane chunk
# (35 pooled columns x 2 channel vectors are 70 lanes, 36 x 16 = 576 at the real channel count below) | the real channel count,
# three images, three chunks per pooled row
POOL_SHAPES = [(1, 1, 1, 4), (1, 2, 2, 4), (2, 7, 10, 64), (1, 8, 9, 64), (1, 3, 70, 8), (3, 36, 52, 64)]


@functools.lru_cache(maxsize=None)
def pool_case(shape):
    """y on the grid k/4, k in [-4, 8], with negative zeros planted (about half the cells are not positive, most windows hold
    a positive tie), dpool on the grid k/64, and torch's gradient on the CPU -- computed once per shape and shared."""
    n, h, w, c = shape
    g = torch.Generator().manual_seed(sum(p * q for p, q in zip(shape, (1, 3, 5, 7))))
    y = torch.randint(-4, 9, shape, generator=g).float() / 4
    y.view(-1)[1::7] = -0.0
    ho, wo = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dpool = torch.randint(-256, 257, (n, ho, wo, c), generator=g).float() / 64
    z = y.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    out = F.max_pool2d(torch.relu(z), 3, 2, 1)
    assert tuple(out.shape[2:]) == (ho, wo)
    out.backward(dpool.permute(0, 3, 1, 2).contiguous())
    return dict(y=y, dpool=dpool, want=z.grad.permute(0, 2, 3, 1).contiguous())


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pool_adjoint_equals_torch(shape):
    from seam_match_rcnn_amd import ops
    cs = pool_case(shape)
    y, dpool = cs["y"].to(DEV), cs["dpool"].to(DEV)
    first = ops.maxpool3s2_relu_bwd(y, dpool)
    second = ops.maxpool3s2_relu_bwd(y, dpool)
    frac = float((cs["y"] <= 0).float().mean())
    print(f"{shape}: {frac:.2f} of y not positive, |want| max {float(cs['want'].abs().max()):.3f}, "
          f"mismatches {int((first.cpu() != cs['want']).sum())}")
    assert first.shape == y.shape and first.dtype == torch.float32
    assert torch.equal(first.cpu(), cs["want"])
    assert torch.equal(first, second)                              # two launches, the same bits
    assert bool((first[y <= 0] == 0).all())                         # the negative zero counts as not positive


def test_pool_adjoint_splits_a_large_batch_over_images(monkeypatch):
    from seam_match_rcnn_amd import ops, ops_train
    shape = POOL_SHAPES[-1]
    n, h, w, c = shape
    cs = pool_case(shape)
    y, dpool = cs["y"].to(DEV), cs["dpool"].to(DEV)
    whole = ops.maxpool3s2_relu_bwd(y, dpool)
    monkeypatch.setattr(ops_train, "WGRAD_MAX_OPERAND_BYTES", h * w * c * 4)                  # one image per launch
    assert torch.equal(ops.maxpool3s2_relu_bwd(y, dpool), whole)
    monkeypatch.setattr(ops_train, "WGRAD_MAX_OPERAND_BYTES", 2 * h * w * c * 4 + 5)          # two images, then one
    assert torch.equal(ops.maxpool3s2_relu_bwd(y, dpool), whole)
    assert torch.equal(whole.cpu(), cs["want"])
    monkeypatch.setattr(ops_train, "WGRAD_MAX_OPERAND_BYTES", h * w * c * 4 - 1)
    with pytest.raises(ValueError):
        ops.maxpool3s2_relu_bwd(y, dpool)


def test_pool_adjoint_refusals_write_nothing():
    from seam_match_rcnn_amd import _native, ops
    lib = _native.lib()
    dy = torch.full((1, 4, 4, 8), float("nan"), device=DEV)
    y, dpool = torch.ones((1, 4, 4, 8), device=DEV), torch.ones((1, 2, 2, 8), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    bad = [(1, 4, 4, 6), (0, 4, 4, 8), (-1, 4, 4, 8), (1, 0, 4, 8), (1, 4, 0, 8), (1, 4, 4, 0),
           (4096, 64, 64, 32)]                    # y of exactly 2^31 bytes
    for dims in bad:
        assert lib.seam_maxpool3s2_relu_bwd_f32(p(y), p(dpool), p(dy), *dims, st) != 0, dims
    assert lib.seam_maxpool3s2_relu_bwd_f32(p(y), None, p(dy), 1, 4, 4, 8, st) != 0
    assert lib.seam_maxpool3s2_relu_bwd_f32(None, p(dpool), p(dy), 1, 4, 4, 8, st) != 0
    assert lib.seam_maxpool3s2_relu_bwd_f32(p(y), p(dpool), None, 1, 4, 4, 8, st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dy).all())
    assert lib.seam_maxpool3s2_relu_bwd_f32(p(y), p(dpool), p(dy), 1, 4, 4, 8, st) == 0       # the same operands, accepted
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dy).any())
    # the wrapper: shapes that do not belong together, a channel count that is no multiple of 4
    with pytest.raises(ValueError):
        ops.maxpool3s2_relu_bwd(y, torch.ones((1, 3, 2, 8), device=DEV))
    with pytest.raises(ValueError):
        ops.maxpool3s2_relu_bwd(y, torch.ones((2, 2, 2, 8), device=DEV))
    with pytest.raises(ValueError):
        ops.maxpool3s2_relu_bwd(torch.ones((1, 4, 4, 6), device=DEV), torch.ones((1, 2, 2, 6), device=DEV))
    with pytest.raises(ValueError):
        ops.maxpool3s2_relu_bwd(torch.ones((4, 4, 8), device=DEV), torch.ones((2, 2, 8), device=DEV))


# ------------------------------------------------------------------------------ the cropped weight gradient
@pytest.mark.parametrize("shape", [(2, 9, 13, 12, 64), (1, 1, 1, 12, 64), (3, 36, 52, 12, 64)], ids=lambda s: "x".join(map(str, s)))
def test_cropped_wgrad_vs_float64(shape):
    """The stem's space-to-depth form: 4x4 / stride 1 / pad 2 cropped to the input grid -- the conv's own grid has one more row
    and one more column, which dy does not hold."""
    from seam_match_rcnn_amd import ops
    n, h, w, c, k = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn((n, h, w, c), generator=g)
    dy = torch.randn((n, h, w, k), generator=g)
    wt = torch.zeros((k, c, 4, 4), dtype=torch.float64, requires_grad=True)
    full = F.conv2d(x.double().permute(0, 3, 1, 2), wt, None, 1, 2)
    assert tuple(full.shape[2:]) == (h + 1, w + 1)
    full[:, :, :h, :w].backward(dy.double().permute(0, 3, 1, 2))
    got = ops.conv_wgrad_chunked(x.to(DEV), dy.to(DEV), 4, 4, 1, 2, out_hw=(h, w))
    again = ops.conv_wgrad_chunked(x.to(DEV), dy.to(DEV), 4, 4, 1, 2, out_hw=(h, w))
    print(f"{shape}: max err {float((got.cpu().double() - wt.grad).abs().max()):.3e} of {float(wt.grad.abs().max()):.3e}")
    assert got.shape == (k, c, 4, 4) and torch.equal(got, again)
    FR.wgrad_close(got, wt.grad.float())


def test_cropped_wgrad_on_the_full_grid_is_conv_wgrad_and_refusals_write_nothing():
    from seam_match_rcnn_amd import _native, ops
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 8, 6, 12), generator=g).to(DEV)
    dy = torch.randn((2, 9, 7, 64), generator=g).to(DEV)
    assert torch.equal(ops.conv_wgrad(x, dy, 4, 4, 1, 2, out_hw=(9, 7)), ops.conv_wgrad(x, dy, 4, 4, 1, 2))
    with pytest.raises(ValueError):
        ops.conv_wgrad(x, dy, 4, 4, 1, 2, out_hw=(8, 6))           # dy is not [2,8,6,K]
    with pytest.raises(ValueError):
        ops.conv_wgrad(x, torch.zeros((2, 10, 7, 64), device=DEV), 4, 4, 1, 2, out_hw=(10, 7))        # beyond the conv's own grid
    lib = _native.lib()
    p = lambda t: C.c_void_p(t.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    dw = torch.full((64, 12, 4, 4), float("nan"), device=DEV)
    ws = torch.zeros((int(lib.seam_conv_wgrad_workspace_floats(2 * 9 * 7, 12, 64, 4, 4)),), device=DEV)
    for ho, wo in ((10, 7), (9, 8), (0, 7), (9, -1)):
        assert lib.seam_conv_wgrad_crop_f32(p(x), p(dy), p(dw), 2, 8, 6, 12, 64, 4, 4, 1, 2, ho, wo, p(ws), st) != 0, (ho, wo)
    assert lib.seam_conv_wgrad_crop_f32(p(x), None, p(dw), 2, 8, 6, 12, 64, 4, 4, 1, 2, 8, 6, p(ws), st) != 0
    assert lib.seam_conv_wgrad_crop_f32(p(x), p(dy), p(dw), 2, 8, 6, 10, 64, 4, 4, 1, 2, 8, 6, p(ws), st) != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(dw).all())


# ------------------------------------------------------------------------------ the module
H, W = 72, 104        # stem output 36 x 52, pooled 18 x 26
PFX = "backbone.body."
ALL = ("conv1", "layer1", "layer2", "layer3", "layer4")


def body_state():
    import seam_match_rcnn_amd.synth as synth
    return {k[len(PFX):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items()
            if k.startswith(PFX)}


def make_body(trainable=ALL, train_stem=True):
    from seam_match_rcnn_amd.models import detection as det
    body = det.ResNet50Body()
    body.load_state_dict(body_state())
    for name, p in body.named_parameters():
        p.requires_grad_(any(name.startswith(t) for t in trainable))
    body.train_stem = train_stem
    return body.to(DEV)


def frames(n):
    g = torch.Generator().manual_seed(40 + n)
    x = torch.randn((n, H, W, 4), generator=g)
    x[..., 3] = 0                                                # NHWC4: the fourth channel is padding
    return x


def space_to_depth(x):
    """NHWC4 [N,H,W,4] -> the frame ``MatchRCNN.forward`` feeds, [N,H/2,W/2,12]: channel (dy*2+dx)*3 + c of cell (i, j) is
    colour c of pixel (2i+dy, 2j+dx)."""
    n, h, w, _ = x.shape
    return x[..., :3].reshape(n, h // 2, 2, w // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, h // 2, w // 2, 12).contiguous()


def grads_of(body, x, ups):
    body.zero_grad(set_to_none=True)
    feats = body.forward_taped(x.to(DEV))
    sum((f * u.to(DEV)).sum() for f, u in zip(feats, ups)).backward()
    return feats, {k: p.grad.detach().clone() for k, p in body.named_parameters() if p.grad is not None}


@pytest.fixture(scope="module")
def stem_runs():
    x4 = frames(2)
    forms = {"nhwc4": x4, "s2d": space_to_depth(x4)}
    body = make_body()
    out = dict(x4=x4, forms=forms)
    g = torch.Generator().manual_seed(9)
    for name, x in forms.items():
        with torch.no_grad():
            plain = body(x.to(DEV))
        if "ups" not in out:
            out["ups"] = [torch.randn(tuple(f.shape), generator=g) for f in plain]
        feats, first = grads_of(body, x, out["ups"])
        _, second = grads_of(body, x, out["ups"])
        out[name] = dict(plain=plain, feats=feats, first=first, second=second)
    return out


@pytest.mark.parametrize("form", ["nhwc4", "s2d"])
def test_taped_forward_with_the_stem_equals_forward(stem_runs, form):
    r = stem_runs[form]
    assert [tuple(t.shape[1:]) for t in r["feats"]] == [(18, 26, 256), (9, 13, 512), (5, 7, 1024), (3, 4, 2048)]
    for a, b in zip(r["plain"], r["feats"]):
        assert torch.equal(a, b)
    assert all(t.requires_grad for t in r["feats"])
    assert r["feats"][0].grad_fn.n_blocks == 16


@pytest.mark.parametrize("form", ["nhwc4", "s2d"])
def test_all_53_gradients_vs_float64(stem_runs, form):
    sd = body_state()
    first, second = stem_runs[form]["first"], stem_runs[form]["second"]
    keys = sorted(k for k in sd if k.endswith("weight") and sd[k].dim() == 4)
    assert len(keys) == 53 and "conv1.weight" in keys and sorted(first) == keys
    assert all(torch.equal(first[k], second[k]) for k in keys)                       # two backward passes, the same bits
    assert all(first[k].shape == sd[k].shape for k in keys)                          # ordinary OIHW .grad tensors
    assert first["conv1.weight"].shape == (64, 3, 7, 7) and first["conv1.weight"].is_contiguous()
    P = {PFX + k: v.double() for k, v in sd.items()}
    for k in keys:
        P[PFX + k].requires_grad_(True)
    x64 = stem_runs["x4"][..., :3].double().permute(0, 3, 1, 2).contiguous()
    ref = OD.resnet50_body(x64, P)
    for f, r in zip(stem_runs[form]["plain"], ref):
        r = r.detach().permute(0, 2, 3, 1)
        assert float((f.cpu().double() - r).abs().max()) <= 1e-3 * float(r.abs().max())      # the bound of smoke()
    sum((r * u.double().permute(0, 3, 1, 2)).sum() for r, u in zip(ref, stem_runs["ups"])).backward()
    FR.compare_grads(first, {k: P[PFX + k].grad for k in keys}, keys)


def test_the_two_input_forms_agree_on_conv1(stem_runs):
    a, b = stem_runs["nhwc4"]["first"]["conv1.weight"], stem_runs["s2d"]["first"]["conv1.weight"]
    print(f"conv1.weight.grad: NHWC4 vs space-to-depth, max diff {float((a - b).abs().max()):.3e} of {float(a.abs().max()):.3e}")
    FR.wgrad_close(b, a)


@pytest.mark.parametrize("form", ["nhwc4", "s2d"])
def test_bottleneck_gradients_equal_a_stem_frozen_run(stem_runs, form):
    for train_stem in (True, False):                   # conv1 frozen: the switch changes nothing, no stem tape
        body = make_body(ALL[1:], train_stem=train_stem)
        feats, got = grads_of(body, stem_runs["forms"][form], stem_runs["ups"])
        first = stem_runs[form]["first"]
        assert len(got) == 52 and sorted(got) == sorted(k for k in first if k != "conv1.weight")
        for k in got:
            assert torch.equal(got[k], first[k]), k
        assert body.conv1.weight.grad is None
        for a, b in zip(feats, stem_runs[form]["plain"]):
            assert torch.equal(a, b)


@pytest.mark.parametrize("form", ["nhwc4", "s2d"])
def test_only_conv1_trainable(stem_runs, form):
    body = make_body(("conv1",))
    feats, got = grads_of(body, stem_runs["forms"][form], stem_runs["ups"])
    assert sorted(got) == ["conv1.weight"]
    assert torch.equal(got["conv1.weight"], stem_runs[form]["first"]["conv1.weight"])
    assert all(p.grad is None for k, p in body.named_parameters() if k != "conv1.weight")
    assert feats[0].grad_fn.n_blocks == 16                        # the gradient passes through every frozen block
    for a, b in zip(feats, stem_runs[form]["plain"]):
        assert torch.equal(a, b)


def test_the_switch_off_and_fp16_are_still_refused(stem_runs):
    x = stem_runs["x4"].to(DEV)
    with pytest.raises(NotImplementedError, match="backbone"):
        make_body(train_stem=False).forward_taped(x)
    from seam_match_rcnn_amd.models import detection as det
    with pytest.raises(NotImplementedError, match="fp32 only"):
        det.set_compute_dtype(make_body(), torch.float16).forward_taped(x)


# ------------------------------------------------------------------------------ the model
NCLS = 14
ROI_BATCH = 64
SIX = ["loss_classifier", "loss_box_reg", "loss_mask", "loss_match", "loss_objectness", "loss_rpn_box_reg"]


def make_model(layers=5, train_stem=True):
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=NCLS, min_size=256, max_size=320,
                               trainable_backbone_layers=layers, train_stem=train_stem, **params)
    sd = synth.detector_state(5, NCLS)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, strict=False)
    m.roi_heads.batch_size_per_image = ROI_BATCH
    return m.to(DEV).train()


def make_model_batch(seed=0):
    """The 256 x 320 two-image batch of tests/test_gpu_rpn_train.py::make_model_batch."""
    import seam_match_rcnn_amd.synth as synth
    g = torch.Generator().manual_seed(seed)
    images, targets = [], []
    for i, (h, w) in enumerate(((200, 250), (192, 240))):
        images.append(torch.from_numpy(synth.frames(50 + i, 1, h, w)[0]).to(DEV))
        ng = 2 + i
        gt = PR.random_gt(g, ng, h, w, 30, 120)
        masks = torch.zeros((ng, h, w), dtype=torch.uint8)
        for j, b in enumerate(gt.round().to(torch.int64).tolist()):
            masks[j, b[1]:b[3], b[0]:b[2]] = 1
        targets.append(dict(boxes=gt.to(DEV), labels=torch.randint(1, NCLS, (ng,), generator=g).to(DEV), masks=masks.to(DEV),
                            pair_ids=torch.randint(0, 3, (ng,), generator=g), styles=torch.randint(1, 3, (ng,), generator=g),
                            sources=torch.tensor([i])))
    return images, targets


def stem_output(m, images):
    with torch.no_grad():
        x = m.transform([i.detach() for i in images])[0]
        body = m.backbone.body
        return body._stem(x, body.packed())


def test_the_model_trains_its_stem():
    images, targets = make_model_batch()
    m = make_model()
    m.rpn.sample_generator = torch.Generator(device=DEV).manual_seed(1)
    m.roi_heads.sample_generator = torch.Generator(device=DEV).manual_seed(2)
    losses = m(images, targets)
    assert list(losses) == SIX
    sum(v for v in losses.values() if bool(torch.isfinite(v))).backward()
    body = dict(m.backbone.body.named_parameters())
    assert len(body) == 53
    for k, p in body.items():
        assert p.grad is not None and p.grad.shape == p.shape, k
        assert bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    assert body["conv1.weight"].grad.shape == (64, 3, 7, 7)
    # one SGD step moves conv1 and the stem's output with it: the packed weights follow the parameter
    w0, s0 = body["conv1.weight"].detach().clone(), stem_output(m, images)
    torch.optim.SGD([p for p in m.parameters() if p.requires_grad], lr=0.01).step()
    s1 = stem_output(m, images)
    assert not torch.equal(body["conv1.weight"].detach(), w0) and not torch.equal(s0, s1)
    fresh = make_model()
    fresh.load_state_dict(m.state_dict())
    assert torch.equal(stem_output(fresh, images), s1)             # ... and is what a fresh model computes from them
    with pytest.raises(NotImplementedError, match="backbone"):      # without the switch the same model still raises
        make_model(train_stem=False)(images, targets)
