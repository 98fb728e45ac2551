"""Three-plane split-bf16 convolution (ops.SX6 / ops.SX9, csrc/seam_conv.hip conv_igemm_sx): the fp32 product as six or nine
exact bf16 piece products in one fp32 accumulator.

The gate: on every shape the split result is as close to the float64 convolution as the exact fp32 kernel
(``seam_conv2d_f32``) is -- e_split <= 2 e_exact + 1e-7, e = max|y - y64| / max|y64| (the factor 2: the summation order alone
moves this figure by that much between two exact fp32 kernels; the floor: shapes where e_exact happens to be 0).  The
two-source and upsampled-residual forms are not served by the split kernel (those layers stay on their fp32 kernels), so they
have no case here."""
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
gpu = pytest.mark.gpu


def bits(words):
    return torch.from_numpy(np.array(words, dtype=np.uint32).view(np.float32).copy())


# all-ones mantissas, alternating bits, the neighbours of +-FLT_MAX, 2^-120, zeros, mixed signs: 32 values = one chunk
SPECIAL = bits([0x3fffffff, 0xbfffffff, 0x7f7fffff, 0xff7fffff, 0x7f7ffffe, 0xff7ffffe, 0x7f7f0001, 0x7f000001,
                0x55555555, 0xaaaaaaaa, 0x2aaaaaaa, 0xd5555555, 0x3faaaaaa, 0xbf555555, 0x03800000, 0x83800000,
                0x00000000, 0x80000000, 0x3f800000, 0xbf800000, 0x3f80ffff, 0x3f8000ff, 0x3fff00ff, 0xbf80ff01,
                0x4b7fffff, 0xcb7fffff, 0x3effffff, 0x3f000001, 0x40490fdb, 0xc02df854, 0x0dffffff, 0x7effffff])


def planes_of(pc, rows, nk):
    """[plane 3][rows][nk * 32] float64 out of a three-plane pack (layout: [slab][chunk][plane][slab rows][32 bf16])."""
    slab = 128 if rows % 128 == 0 else 64
    p = pc.w.view(-1).view(rows // slab, nk, 3, slab, 32).float().cpu().double()
    return p.permute(2, 0, 3, 1, 4).reshape(3, rows, nk * 32)


def conv_igemm_f32(x, pc, relu, res):
    """``seam_conv2d_f32`` itself (ops.conv2d may hand an fp32 pack to another exact kernel)."""
    from seam_match_rcnn_amd import _native, ops
    n, h, w, c = x.shape
    ho, wo = (h + 2 * pc.pad - pc.R) // pc.stride + 1, (w + 2 * pc.pad - pc.S) // pc.stride + 1
    y = torch.empty((n, ho, wo, pc.K), dtype=torch.float32, device=x.device)
    _native.check(_native.lib().seam_conv2d_f32(ops._ptr(x), ops._ptr(pc.w), ops._ptr(pc.scale), ops._ptr(pc.shift), ops._ptr(res),
                                                ops._ptr(y), n, h, w, c, pc.K, pc.R, pc.S, pc.stride, pc.pad, int(relu),
                                                ops._stream()), "seam_conv2d_f32")
    return y


@gpu
@pytest.mark.parametrize("terms", [6, 9])
def test_split_identity(terms):
    from seam_match_rcnn_amd import ops
    dt = {6: ops.SX6, 9: ops.SX9}[terms]
    assert bool(torch.isfinite(SPECIAL).all())
    # weights: row 0 holds the values, row 1 their reverse
    wt = torch.zeros(64, 32, 1, 1)
    wt[0, :, 0, 0] = SPECIAL
    wt[1, :, 0, 0] = SPECIAL.flip(0)
    pl = planes_of(ops.pack_conv(wt.to(DEV), dtype=dt), 64, 1)
    assert torch.equal(pl.sum(0)[:, :32], wt[:, :, 0, 0].double())
    assert bool((pl[0, 0].abs() <= SPECIAL.double().abs()).all())          # truncation: the top piece never rounds away from zero
    # activations: an identity weight hands each value's pieces back through the accumulator, smallest first
    eye = torch.zeros(32, 32, 1, 1)
    eye[torch.arange(32), torch.arange(32)] = 1.0
    pe = ops.pack_conv(eye.to(DEV), dtype=dt)
    benign = normal(5, (32,))
    yb = ops.conv2d(benign.view(1, 1, 1, 32).to(DEV), pe).cpu().view(32)
    alone = ops.conv2d(torch.diag(SPECIAL).view(32, 1, 1, 32).to(DEV), pe).cpu().view(32, 32)      # one value per pixel, the rest zeros
    y = ops.conv2d(SPECIAL.view(1, 1, 1, 32).to(DEV), pe).cpu().view(32)
    print(f"split identity terms {terms}: benign ok {torch.equal(yb, benign)}, alone wrong at {(alone.diagonal() != SPECIAL).nonzero().view(-1).tolist()}, "
          f"non-finite pixels {(~torch.isfinite(alone)).any(1).nonzero().view(-1).tolist()}, together wrong at {(y != SPECIAL).nonzero().view(-1).tolist()}")
    assert torch.equal(yb, benign)
    assert torch.equal(alone.double(), torch.diag(SPECIAL).double())
    assert torch.equal(y.double(), SPECIAL.double()), (y, SPECIAL)


def normal(seed, shape):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed))


def make_case(n, c, h, w, k, r, stride, pad, relu, res, seed):
    x = normal(seed, (n, c, h, w))
    wt = normal(seed + 1, (k, c, r, r)) / math.sqrt(c * r * r)
    bias = normal(seed + 2, (k,)) * 0.1
    return x, wt, bias


def errors(x, wt, bias, stride, pad, relu, res, dt):
    from seam_match_rcnn_amd import ops
    ref = F.conv2d(x.double(), wt.double(), bias.double(), stride, pad)
    resid = normal(77, tuple(ref.shape)) if res else None
    if res:
        ref = ref + resid.double()
    if relu:
        ref = F.relu(ref)
    xin = x.permute(0, 2, 3, 1).contiguous().to(DEV)
    rd = None if resid is None else resid.permute(0, 2, 3, 1).contiguous().to(DEV)
    ys = ops.conv2d(xin, ops.pack_conv(wt.to(DEV), bias.to(DEV), stride=stride, pad=pad, dtype=dt), relu, rd)
    ye = conv_igemm_f32(xin, ops.pack_conv(wt.to(DEV), bias.to(DEV), stride=stride, pad=pad, wino=False), relu, rd)
    ref = ref.permute(0, 2, 3, 1)
    scale = float(ref.abs().max())
    return (float((ys.cpu().double() - ref).abs().max()) / scale, float((ye.cpu().double() - ref).abs().max()) / scale)


GATE_CASES = [
    # N, C, H, W, K, R, stride, pad, relu, res
    (1, 32, 8, 8, 32, 1, 1, 0, False, False),            # one chunk
    (2, 96, 5, 7, 64, 1, 1, 0, False, False),            # three chunks, ragged M
    (1, 256, 14, 14, 1024, 1, 1, 0, True, False),
    (1, 128, 9, 9, 128, 3, 2, 1, False, False),          # 3x3 stride 2 pad 1
    (2, 1024, 10, 10, 256, 1, 1, 0, False, True),        # + residual
]


@gpu
@pytest.mark.parametrize("terms", [6, 9])
@pytest.mark.parametrize("case", GATE_CASES)
def test_accuracy_gate(case, terms):
    from seam_match_rcnn_amd import ops
    n, c, h, w, k, r, stride, pad, relu, res = case
    x, wt, bias = make_case(n, c, h, w, k, r, stride, pad, relu, res, 11)
    e_split, e_exact = errors(x, wt, bias, stride, pad, relu, res, {6: ops.SX6, 9: ops.SX9}[terms])
    print(f"split gate {case} terms {terms}: e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


@gpu
@pytest.mark.parametrize("terms", [6, 9])
def test_accuracy_gate_on_cancelling_input(terms):
    """Channel pairs (v, -v (1 + 2^-12)) against equal weights: the leading terms of each pair vanish, what is left is made of
    the low-order pieces -- the dropped ones show here if they show anywhere."""
    from seam_match_rcnn_amd import ops
    c, k = 256, 64
    v = normal(21, (2, c // 2, 6, 6))
    x = torch.stack([v, -v * (1.0 + 2.0 ** -12)], 2).reshape(2, c, 6, 6)
    wh = normal(22, (k, c // 2, 1, 1)) / math.sqrt(c)
    wt = torch.stack([wh, wh], 2).reshape(k, c, 1, 1)
    e_split, e_exact = errors(x, wt, torch.zeros(k), 1, 0, False, False, {6: ops.SX6, 9: ops.SX9}[terms])
    print(f"split gate cancelling terms {terms}: e_split {e_split:.3e} e_exact {e_exact:.3e}")
    assert e_split <= 2 * e_exact + 1e-7, (e_split, e_exact)


@gpu
@pytest.mark.parametrize("terms", [6, 9])
def test_deterministic_and_batch_invariant(terms):
    from seam_match_rcnn_amd import ops
    dt = {6: ops.SX6, 9: ops.SX9}[terms]
    x = normal(31, (3, 5, 7, 96)).to(DEV)
    res = normal(32, (3, 5, 7, 64)).to(DEV)
    pc = ops.pack_conv((normal(33, (64, 96, 1, 1)) * 0.1).to(DEV), normal(34, (64,)).to(DEV), dtype=dt)
    a = ops.conv2d(x, pc, True, res)
    b = ops.conv2d(x, pc, True, res)
    assert torch.equal(a, b)
    alone = ops.conv2d(x[:1].contiguous(), pc, True, res[:1].contiguous())
    assert torch.equal(alone[0], a[0])
    # a map big enough for the 128-row tile, and its first image alone (another tile shape: the same bits)
    x = normal(35, (3, 40, 40, 64)).to(DEV)
    pc = ops.pack_conv((normal(36, (256, 64, 1, 1)) * 0.1).to(DEV), None, dtype=dt)
    a = ops.conv2d(x, pc)
    assert torch.equal(ops.conv2d(x[:1].contiguous(), pc)[0], a[0])


@gpu
def test_switch_restores_the_exact_kernels():
    """``split_f32`` off: a body forward is the launches of ops.conv2d on the fp32 packs, bit for bit; on (an eval-mode module,
    no gradient tape) the split kernels serve their classes; a training-mode module or an enabled tape keeps the exact kernels."""
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd import ops
    from seam_match_rcnn_amd.models import detection as det
    pfx = "backbone.body."
    sd = {k[len(pfx):]: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.detector_state(5, 14).items() if k.startswith(pfx)}
    body = det.ResNet50Body()
    body.load_state_dict(sd)
    body = body.to(DEV).eval()
    x = normal(41, (1, 64, 64, 4))
    x[..., 3] = 0
    x = x.to(DEV)

    def exact_chain():
        pk = body.packed()
        h, feats = body._stem(x, pk), []
        for li, bi, b in body.blocks():
            h = det.body_block(h, pk[(li, bi)], b.stride)[0]
            if bi == len(getattr(body, f"layer{li}")) - 1:
                feats.append(h)
        return feats

    with torch.no_grad():
        on = body(x)
        assert any(k in e for e in body.packed().values() if isinstance(e, dict) for k in ("c1x", "c2x", "c3x"))
        det.set_split_f32(body, False)
        off = body(x)
        assert all(e.dtype == torch.float32 for v in body.packed().values() if isinstance(v, dict) for e in v.values())
        want = exact_chain()
        det.set_split_f32(body, True)
    for a, b in zip(off, want):
        assert torch.equal(a, b)
    assert any(not torch.equal(a, b) for a, b in zip(on, want))                 # the switch switches something
    for a, b in zip(on, want):
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
    grad_on = body(x)                                                            # grad enabled: the exact kernels
    body.train()
    with torch.no_grad():
        training = body(x)                                                       # training mode: its no-grad forward equals its taped one
    for a, b, c in zip(grad_on, training, want):
        assert torch.equal(a, c) and torch.equal(b, c)


@gpu
def test_the_body_repacks_when_a_pack_time_knob_moves():
    """Packs only, no forward: ``packed()`` follows SPLIT_CLASSES and FUSE_SHORTCUT by its key, nobody drops ``_pk`` by hand."""
    from seam_match_rcnn_amd.models import detection as det
    body = det.ResNet50Body().to(DEV).eval()
    blocks = lambda pk: {key: e for key, e in pk.items() if isinstance(key, tuple)}
    having = lambda pk, name: [key for key, e in blocks(pk).items() if name in e]
    classes, fuse = det.SPLIT_CLASSES, det.FUSE_SHORTCUT
    assert {"c1", "c2s2", "c3", "c3ds"} <= classes and fuse
    try:
        first = body.packed()
        assert "c1x" in first[(2, 1)] and "c3ds" in first[(2, 0)] and "c3dsx" in first[(2, 0)]
        c3x, c2x = having(first, "c3x"), having(first, "c2x")
        assert c3x and c2x
        det.SPLIT_CLASSES = classes - {"c1"}
        without = body.packed()
        assert without is not first and not having(without, "c1x")
        assert having(without, "c3x") == c3x and having(without, "c2x") == c2x
        det.SPLIT_CLASSES = classes
        again = body.packed()
        assert again is not without and "c1x" in again[(2, 1)] and len(having(again, "c1x")) == 16
        det.FUSE_SHORTCUT = False
        unfused = body.packed()
        assert unfused is not again and not having(unfused, "c3ds") and not having(unfused, "c3dsx")
        assert "ds" in unfused[(2, 0)] and "c1x" in unfused[(2, 1)]
        det.FUSE_SHORTCUT = fuse
        fused = body.packed()
        assert fused is not unfused and "c3ds" in fused[(2, 0)] and "c3dsx" in fused[(2, 0)]
        assert body.packed() is fused
    finally:
        det.SPLIT_CLASSES, det.FUSE_SHORTCUT = classes, fuse


def test_header_exports_and_signatures_agree():
    from seam_match_rcnn_amd import _native
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "seam_hip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(seam_[a-z0-9_]+)\s*\(", txt)))
    assert sorted(_native.SIGNATURES) == declared
    for name in ("seam_pack_conv_weight_sx", "seam_conv2d_sx"):
        assert name in declared and hasattr(_native.lib(), name)
    assert len(_native.SIGNATURES["seam_conv2d_sx"][1]) == len(_native.SIGNATURES["seam_conv2d_bx3"][1]) + 1      # + terms
