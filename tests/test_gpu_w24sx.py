"""GPU: conv3x3_wino24sx (csrc/seam_wino24sx.hip) -- the F(2x4,3x3) Winograd convolution with its position GEMMs as six-term
split-bf16 products -- through the C ABI, against a float64 direct convolution y64 with e = max|y - y64| / max|y64|.

Gates on every case:
  * e_new <= 3 * e_w24 + 1e-7, e_w24 = seam_conv3x3_wino24_f32's error on the same inputs.  The 3: the CPU emulation (fp32 transforms,
    bf16-plane products accumulated in fp32 per 16-channel step, six terms) gave ratios of 1.2-2.4 over six shapes, six and nine
    terms alike -- the added error is accumulation length, not the dropped terms; the margin over 2.4 is for the MFMA's internal
    summation, which the emulation cannot reproduce.  (tools/w24sx_noise_probe.py, which sums a k-step's products one after the
    other in fp32, reads 1.9-3.4; measured on the GPU: 0.63-0.91 on these cases)
  * |y_new - y_exact| <= 2e-5 * scale against seam_conv2d_f32, the bound of every Winograd kernel in tests/test_gpu_wino.py.
Every output is carved out of a larger allocation whose guard bytes, before and behind it, are checked after the launch."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import seam_match_rcnn_amd.synth as synth

pytestmark = pytest.mark.gpu

GUARD = 1 << 16          # bytes before and behind every output that must stay untouched


def rnd(seed, shape, name="x"):
    return torch.from_numpy(synth.normal(synth.stream_id(seed, name), shape))


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


@pytest.fixture(scope="module")
def env():
    import seam_match_rcnn_amd.ops as ops
    from seam_match_rcnn_amd import _native
    return ops, _native.lib(), torch.device("cuda:0")


class Out:
    """An fp32 output filled with NaN between two guard zones of 0x5A."""

    def __init__(self, shape, dev):
        n = math.prod(shape) * 4
        self.raw = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device=dev)
        self.raw.fill_(0x5A)
        self.y = self.raw[GUARD:GUARD + n].view(torch.float32).view(shape)
        self.y.fill_(float("nan"))
        self.n = n

    def intact(self):
        return bool((self.raw[:GUARD] == 0x5A).all()) and bool((self.raw[GUARD + self.n:] == 0x5A).all())


def pack_sx(lib, wt, dev):
    k, c = wt.shape[:2]
    u = torch.empty((int(lib.seam_wino24sx_weight_bytes(k, c)),), dtype=torch.uint8, device=dev)
    assert lib.seam_pack_conv_weight_wino24_sx(ptr(wt), ptr(u), k, c, c, 0, None) == 0
    return u


def pack_w24(lib, wt, dev):
    k, c = wt.shape[:2]
    u = torch.empty((int(lib.seam_wino24_weight_floats(k, c)),), dtype=torch.float32, device=dev)
    assert lib.seam_pack_conv_weight_wino24_f32(ptr(wt), ptr(u), k, c, c, 0, None) == 0
    return u


def run_sx(lib, dev, x, u, sc, sh, res, k, pad, relu):
    n, h, w, c = x.shape
    o = Out((n, h + 2 * pad - 2, w + 2 * pad - 2, k), dev)
    rc = lib.seam_conv3x3_wino24sx_f32(ptr(x), ptr(u), ptr(sc), ptr(sh), ptr(res), ptr(o.y), n, h, w, c, k, pad, 1, relu, None)
    torch.cuda.synchronize()
    assert rc == 0 and o.intact(), f"rc {rc}, guards intact: {o.intact()}"
    return o.y


_cache = {}


def problem(env, n, h, w, c, k, pad):
    """Inputs, the float64 reference of the plain convolution and the two existing kernels' outputs, computed once per shape."""
    key = (n, h, w, c, k, pad)
    if key not in _cache:
        ops, lib, dev = env
        x = rnd(71, (n, c, h, w))
        wt = rnd(72, (k, c, 3, 3), "w") * (1.0 / math.sqrt(c * 9))
        y64 = F.conv2d(x.double(), wt.double(), None, 1, pad).permute(0, 2, 3, 1).contiguous()
        xd, wd = nhwc(x).to(dev), wt.to(dev)
        ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
        y24 = torch.empty((n, ho, wo, k), dtype=torch.float32, device=dev)
        assert lib.seam_conv3x3_wino24_f32(ptr(xd), ptr(pack_w24(lib, wd, dev)), None, None, None, ptr(y24), n, h, w, c, k, pad, 0, None) == 0
        pc = ops.pack_conv(wd, None, stride=1, pad=pad)
        yex = torch.empty_like(y24)
        assert lib.seam_conv2d_f32(ptr(xd), ptr(pc.w), None, None, None, ptr(yex), n, h, w, c, k, 3, 3, 1, pad, 0, None) == 0
        torch.cuda.synchronize()
        _cache[key] = dict(x=xd, w=wd, u=pack_sx(lib, wd, dev), y64=y64, y24=y24.cpu(), yex=yex.cpu())
    return _cache[key]


def gates(tag, y, ref64, y24, yex):
    """The two gates; ref64 / y24 / yex already carry the case's epilogue."""
    scale = float(ref64.abs().max())
    e_new = float((y.double() - ref64).abs().max()) / scale
    e_w24 = float((y24.double() - ref64).abs().max()) / scale
    d_ex = float((y - yex).abs().max())
    print(f"{tag}: e_new {e_new:.3e} e_w24 {e_w24:.3e} ratio {e_new / max(e_w24, 1e-30):.2f} |new-exact|/scale {d_ex / scale:.3e}")
    assert e_new <= 3 * e_w24 + 1e-7, f"{tag}: e_new {e_new:.3e} > 3 * {e_w24:.3e} + 1e-7"
    assert d_ex <= 2e-5 * scale, f"{tag}: |new - exact| {d_ex:.3e} > 2e-5 * {scale:.3e}"


def test_one_block(env):
    """1 x 8x8, 64 -> 64, pad 1: one block, 8 of 32 tile slots, 4 k-steps."""
    _, lib, dev = env
    p = problem(env, 1, 8, 8, 64, 64, 1)
    y = run_sx(lib, dev, p["x"], p["u"], None, None, None, 64, 1, 0).cpu()
    gates("1x8x8 64->64 pad1", y, p["y64"], p["y24"], p["yex"])


CASES = [
    pytest.param((2, 9, 11, 64, 64, 1), id="ragged-2x9x11-64-64"),
    pytest.param((3, 14, 14, 128, 64, 1), id="stacked-3x14x14-128-64-pad1"),
    pytest.param((3, 14, 14, 128, 64, 0), id="stacked-3x14x14-128-64-pad0"),
    pytest.param((1, 40, 52, 64, 128, 1), id="regions-1x40x52-64-128"),
    pytest.param((1, 10, 10, 192, 64, 0), id="valid-1x10x10-192-64"),
    pytest.param((2, 25, 25, 256, 64, 1), id="long-k-2x25x25-256-64"),
]


@pytest.mark.parametrize("case", CASES)
def test_vs_float64_and_exact(env, case):
    _, lib, dev = env
    n, h, w, c, k, pad = case
    p = problem(env, *case)
    y = run_sx(lib, dev, p["x"], p["u"], None, None, None, k, pad, 0).cpu()
    gates(str(case), y, p["y64"], p["y24"], p["yex"])


@pytest.mark.parametrize("mode", ["scale_shift", "residual", "relu", "residual_relu"])
def test_epilogue_modes(env, mode):
    """Every epilogue mode on the ragged shape; the fp32 kernels run the same epilogue on the same inputs."""
    ops, lib, dev = env
    n, h, w, c, k, pad = 2, 9, 11, 64, 64, 1
    p = problem(env, n, h, w, c, k, pad)
    sc = torch.from_numpy(synth.uniform(synth.stream_id(73, "sc"), (k,), 0.5, 1.5))
    sh = rnd(74, (k,), "sh") * 0.1
    res = rnd(75, tuple(p["y64"].shape), "res") if "residual" in mode else None
    relu = 1 if "relu" in mode else 0
    ref = p["y64"] * sc.double() + sh.double()
    if res is not None:
        ref = ref + res.double()
    if relu:
        ref = F.relu(ref)
    scd, shd, resd = sc.to(dev), sh.to(dev), None if res is None else res.to(dev)
    y24 = torch.empty(tuple(p["y64"].shape), dtype=torch.float32, device=dev)
    yex = torch.empty_like(y24)
    assert lib.seam_conv3x3_wino24_f32(ptr(p["x"]), ptr(pack_w24(lib, p["w"], dev)), ptr(scd), ptr(shd), ptr(resd), ptr(y24), n, h, w, c, k,
                                       pad, relu, None) == 0
    pc = ops.pack_conv(p["w"], None, stride=1, pad=pad)
    assert lib.seam_conv2d_f32(ptr(p["x"]), ptr(pc.w), ptr(scd), ptr(shd), ptr(resd), ptr(yex), n, h, w, c, k, 3, 3, 1, pad, relu, None) == 0
    y = run_sx(lib, dev, p["x"], p["u"], scd, shd, resd, k, pad, relu).cpu()
    gates(mode, y, ref, y24.cpu(), yex.cpu())


def test_pack_planes_sum_to_the_fp32_pack(env):
    """The three planes, un-permuted, sum bit for bit to the fp32 U of seam_pack_conv_weight_wino24_f32."""
    _, lib, dev = env
    k, c = 128, 192
    wt = (rnd(76, (k, c, 3, 3), "w") / math.sqrt(c * 9)).to(dev)
    u24 = pack_w24(lib, wt, dev).view(k // 32, c // 8, 24, 64, 4)
    ux = pack_sx(lib, wt, dev).view(torch.int16).view(k // 32, c // 16, 24, 3, 64, 2, 4)
    planes = (ux.to(torch.int32) << 16).view(torch.float32)
    # [tn, ks, p, pl, lane, j, e] -> [pl, tn, chunk = 2 ks + j, p, lane, e]
    planes = planes.permute(3, 0, 1, 5, 2, 4, 6).reshape(3, k // 32, c // 8, 24, 64, 4)
    total = (planes[0] + planes[1]) + planes[2]
    assert torch.equal(total.view(torch.int32), u24.view(torch.int32))
    assert bool((planes[1].abs() <= planes[0].abs() * 2.0 ** -7).all()) and bool((planes[2].abs() <= planes[0].abs() * 2.0 ** -15).all())


@pytest.mark.parametrize("case", [pytest.param((2, 40, 52, 64, 128, 1), id="regions"), pytest.param((3, 14, 14, 128, 64, 1), id="stacked")])
def test_determinism_and_batch_invariance(env, case):
    _, lib, dev = env
    n, h, w, c, k, pad = case
    p = problem(env, *case)
    y = run_sx(lib, dev, p["x"], p["u"], None, None, None, k, pad, 0)
    y2 = run_sx(lib, dev, p["x"], p["u"], None, None, None, k, pad, 0)
    assert torch.equal(y, y2)
    for i in range(n):
        yi = run_sx(lib, dev, p["x"][i:i + 1].contiguous(), p["u"], None, None, None, k, pad, 0)
        assert torch.equal(yi[0], y[i]), f"image {i} alone differs from image {i} in the batch"


@pytest.mark.parametrize("relu", [0, 1])
def test_zero_input_gives_the_shift(env, relu):
    _, lib, dev = env
    p = problem(env, 2, 9, 11, 64, 64, 1)
    sh = (rnd(77, (64,), "sh")).to(dev)
    y = run_sx(lib, dev, torch.zeros_like(p["x"]), p["u"], None, sh, None, 64, 1, relu)
    want = (F.relu(sh) if relu else sh).expand_as(y)
    assert torch.equal(y, want)


@pytest.mark.parametrize("c,k,stride", [(96, 64, 1), (64, 32, 1), (64, 64, 2)])
def test_refusals(env, c, k, stride):
    _, lib, dev = env
    x = torch.zeros((1, 8, 8, c), dtype=torch.float32, device=dev)
    u = torch.zeros((144 * 128 * 128,), dtype=torch.uint8, device=dev)
    o = Out((1, 8, 8, k), dev)
    assert lib.seam_conv3x3_wino24sx_supported(1, 8, 8, c, k, 1, stride) == 0
    assert lib.seam_conv3x3_wino24sx_f32(ptr(x), ptr(u), None, None, None, ptr(o.y), 1, 8, 8, c, k, 1, stride, 0, None) != 0
    torch.cuda.synchronize()
    assert o.intact() and bool(torch.isnan(o.y).all())
