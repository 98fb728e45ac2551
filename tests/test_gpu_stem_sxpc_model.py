"""The split class ``stem`` in the ResNet body (models/detection.py): which calls run ``stem_sxpc``, and that every other call
gives the exact kernels' bytes whether the fp32 space-to-depth frame came padded (2 + 1 zero cells) or not.

"The exact bytes" are written down here as the body computed its stem before the class existed: the implicit GEMM over the
unpadded frame with pad 2, cropped to the frame's grid, FrozenBN + ReLU, then the 3x3 / stride-2 max-pool."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
PFX = "backbone.body."


def normal(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


_BODY = {}


def body():
    """one eval-mode body for the file: tests move only switches and put them back"""
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models import detection as det
    if not _BODY:
        sd = {k[len(PFX):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items() if k.startswith(PFX)}
        b = det.ResNet50Body()
        b.load_state_dict(sd)
        for p in b.parameters():
            p.requires_grad_(False)
        _BODY["b"] = b.to(DEV).eval()
    return _BODY["b"]


def frame(n=2, hs=16, ws=24, seed=11):
    x = normal(seed, (n, hs, ws, 12))
    return (x + 0.5 * torch.sign(x)).to(DEV)            # no zero anywhere: the border cells are not zeros


def padded(x):
    return F.pad(x, (0, 0, 2, 1, 2, 1)).contiguous()


def exact_stem(b, x, pool=True):
    from seam_match_rcnn_amd import ops
    y = ops.conv2d(x, b.packed()["stem_s2d"], relu=True, out_hw=(x.shape[1], x.shape[2]))
    return ops.maxpool2d(y, 3, 2, 1) if pool else y


def traced(fn):
    from seam_match_rcnn_amd import ops
    ops.CONV_TRACE = []
    try:
        out = fn()
        return out, [t[0] for t in ops.CONV_TRACE]
    finally:
        ops.CONV_TRACE = None


def same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


class knobs:
    def __enter__(self):
        from seam_match_rcnn_amd import ops
        from seam_match_rcnn_amd.models import detection as det
        self.saved = (ops.SXPC, det.SPLIT_CLASSES, det.SPLIT_F32, det.BODY_STREAMS)
        return self

    def __exit__(self, *exc):
        from seam_match_rcnn_amd import ops
        from seam_match_rcnn_amd.models import detection as det
        ops.SXPC, det.SPLIT_CLASSES, det.SPLIT_F32, det.BODY_STREAMS = self.saved
        det.set_split_f32(body(), True)
        body().eval()
        return False


def test_the_split_stem_runs_and_is_the_kernel_on_the_twin():
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    assert "stem" in det.SPLIT_CLASSES
    b, x = body(), frame()
    with knobs(), torch.no_grad():
        det.BODY_STREAMS = 1
        on, names = traced(lambda: b(x))
        assert names[0] == "stem_sxpc" and names.count("stem_sxpc") == 1, names[:3]
        on_p, names = traced(lambda: b(padded(x), True))
        assert names[0] == "stem_sxpc" and same(on, on_p)
        twin = b.packed()["stem_x"]
        by_hand = ops.maxpool2d(ops.stem_s2d_sx(padded(x), twin, relu=True, padded=True), 3, 2, 1)
        assert torch.equal(b._stem(x, b.packed()), by_hand)
        today = exact_stem(b, x)
        assert not torch.equal(by_hand, today)
        assert float((by_hand - today).abs().max()) <= 1e-5 * float(today.abs().max())
        det.BODY_STREAMS = 2                               # two batch slices on two streams: the same bits
        assert same(b(frame(4)), [torch.cat([u, v]) for u, v in zip(b(frame(4)[:2]), b(frame(4)[2:]))])


@pytest.mark.parametrize("how", ["class_off", "split_f32_off", "process_switch", "sxpc_off"])
def test_switched_off_the_body_gives_the_exact_stems_bytes(how):
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    b, x = body(), frame()
    with knobs(), torch.no_grad():
        det.BODY_STREAMS = 1
        if how == "class_off":
            det.SPLIT_CLASSES = det.SPLIT_CLASSES - {"stem"}
        elif how == "split_f32_off":
            det.set_split_f32(b, False)
        elif how == "process_switch":
            det.SPLIT_F32 = False
        else:
            ops.SXPC = False
        off, names = traced(lambda: b(x))
        assert "stem_sxpc" not in names and names[0].startswith("conv_igemm<float"), names[:3]
        if how == "class_off":
            assert "stem_x" not in b.packed()
        assert torch.equal(b._stem(x, b.packed()), exact_stem(b, x))
        off_p, names = traced(lambda: b(padded(x), True))          # a padded frame all the same: the valid convolution over it
        assert "stem_sxpc" not in names and names[0].startswith("conv_igemm<float"), names[:3]
        assert same(off, off_p)


def test_class_off_leaves_the_rest_of_the_body_as_it_is():
    """without ``stem`` the body is the stem's exact bytes followed by the walk it has with the class on"""
    from seam_match_rcnn_amd.models import detection as det
    b, x = body(), frame()
    with knobs(), torch.no_grad():
        det.BODY_STREAMS = 1
        det.SPLIT_CLASSES = det.SPLIT_CLASSES - {"stem"}
        off, names_off = traced(lambda: b(x))
        det.SPLIT_CLASSES = det.SPLIT_CLASSES | {"stem"}
        _, names_on = traced(lambda: b(x))
        assert names_on[1:] == names_off[1:]


@pytest.mark.parametrize("pad", [False, True], ids=["unpadded", "padded"])
def test_grad_training_mode_and_the_taped_forward_stay_exact(pad):
    b, x = body(), frame()
    xin = padded(x) if pad else x
    want = exact_stem(b, x)
    with knobs():
        with torch.enable_grad():
            got, names = traced(lambda: b._stem(xin, b.packed(), pad))
        assert "stem_sxpc" not in names and torch.equal(got, want)
        b.train()
        with torch.no_grad():
            got, names = traced(lambda: b._stem(xin, b.packed(), pad))
        assert "stem_sxpc" not in names and torch.equal(got, want)
        b.eval()
        with torch.no_grad():
            ref = b(x)
        from seam_match_rcnn_amd.models import detection as det
        feats, names = traced(lambda: b.forward_taped(xin, pad))
        assert "stem_sxpc" not in names
        det.set_split_f32(b, False)
        with torch.no_grad():
            exact = b(x)
        assert same(feats, exact) and not same(feats, ref)


def test_a_frame_under_128_cells_takes_the_exact_kernel():
    b = body()
    x = frame(2, 9, 14)                                    # 126 cells
    with knobs(), torch.no_grad():
        got, names = traced(lambda: b._stem(x, b.packed()))
        assert len(names) == 1 and names[0].startswith("conv_igemm<float"), names
        assert torch.equal(got, exact_stem(b, x))
        got, names = traced(lambda: b._stem(padded(x), b.packed(), True))
        assert len(names) == 1 and names[0].startswith("conv_igemm<float") and torch.equal(got, exact_stem(b, x))
        _, names = traced(lambda: b._stem(frame(1, 8, 16), b.packed()))       # 128 cells: served
        assert names == ["stem_sxpc"]


def test_the_transform_pads_only_when_the_split_stem_will_run():
    from seam_match_rcnn_amd.models import detection as det
    tf = det.GeneralizedRCNNTransform(64, 96).to(DEV).eval()
    imgs = [torch.rand((3, 64, 96), generator=torch.Generator().manual_seed(i)).to(DEV) for i in range(2)]
    with knobs():
        with torch.no_grad():
            xp, sizes, _, (hp, wp) = tf(imgs)
            assert tuple(xp.shape) == (2, hp // 2 + 3, wp // 2 + 3, 12)
            det.SPLIT_CLASSES = det.SPLIT_CLASSES - {"stem"}
            x, _, _, _ = tf(imgs)
            det.SPLIT_CLASSES = det.SPLIT_CLASSES | {"stem"}
        assert tuple(x.shape) == (2, hp // 2, wp // 2, 12)
        assert torch.equal(xp[:, 2:-1, 2:-1], x)            # the interior is the unpadded frame, the cells around it are zeros
        ring = xp.clone()
        ring[:, 2:-1, 2:-1] = 0
        assert not bool(ring.any())
        with torch.enable_grad():
            assert tuple(tf(imgs)[0].shape) == tuple(x.shape)
        tf.train()
        with torch.no_grad():
            assert tuple(tf(imgs)[0].shape) == tuple(x.shape)
        tf.eval()
        det.set_split_f32(tf, False)
        with torch.no_grad():
            assert tuple(tf(imgs)[0].shape) == tuple(x.shape)
        det.set_split_f32(tf, True)
        small = det.GeneralizedRCNNTransform(16, 28).to(DEV).eval()           # 32 x 32 padded: 16 x 16 cells ... served; 8 x 14: not
        with torch.no_grad():
            t = small([torch.rand((3, 16, 28)).to(DEV)])
        assert t[0].shape[1] == t[3][0] // 2 + (3 if (t[3][0] // 2) * (t[3][1] // 2) >= 128 else 0)


def test_after_an_sgd_step_with_train_stem_the_twin_equals_a_fresh_pack():
    """``optim.SGD(..., model=)`` refreshes the body's packs in place: the stem's twin (a derived source of conv1.weight and its
    SEAM_REPACK_SXPC64 job) follows the parameter."""
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    from seam_match_rcnn_amd.optim import SGD

    class Holder(torch.nn.Module):
        def __init__(self, b):
            super().__init__()
            self.backbone = torch.nn.Module()
            self.backbone.body = b

    sd = {k[len(PFX):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items() if k.startswith(PFX)}
    b = det.ResNet50Body()
    b.load_state_dict(sd)
    for name, p in b.named_parameters():
        p.requires_grad_(name == "conv1.weight")
    b.train_stem = True
    m = Holder(b).to(DEV)
    opt = SGD([b.conv1.weight], lr=0.05, momentum=0.9, model=m)
    twin = b.packed()["stem_x"]
    before = twin.wx64.clone()
    b.conv1.weight.grad = normal(3, tuple(b.conv1.weight.shape)).to(DEV)
    opt.step()
    assert opt.plan.refreshes == 1 and opt.plan.rebuilds == 0
    assert b.packed()["stem_x"] is twin and not torch.equal(twin.wx64, before)
    fresh = det.ResNet50Body()
    fresh.load_state_dict(b.state_dict())
    ft = fresh.to(DEV).packed()["stem_x"]
    assert torch.equal(ft.wx64, twin.wx64) and torch.equal(ft.w, twin.w)
    assert torch.equal(ft.scale, twin.scale) and torch.equal(ft.shift, twin.shift)
    x = frame()
    with torch.no_grad():
        assert torch.equal(ops.stem_s2d_sx(x, twin), ops.stem_s2d_sx(x, ft))
