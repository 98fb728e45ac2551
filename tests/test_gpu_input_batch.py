"""GPU: ``ops.preprocess_u8_batch`` (``seam_preprocess_u8_batch_f32``, csrc/seam_input.hip) -- ToTensor + flip + normalise + resize +
pad + layout for a batch of uint8 images of different sizes in one launch -- against the existing fp32 path, bit for bit:

    ops.preprocess([to_tensor(img).flip(-1) if f else to_tensor(img) ...], sizes, hp, wp, s2d=...)

in both layouts (NHWC4 and space-to-depth), onto an output pre-filled with NaN so that every pad cell is checked.  The shapes are
small, each aimed at one way to go wrong: odd widths and odd byte offsets, the no-resize branch, an upscale and a
``max_size``-limited downscale, flips (none, all, mixed), one image, rows of width 1 and 2."""
import math

import numpy as np
import pytest
import torch

from seam_match_rcnn_amd import _native, ops
from seam_match_rcnn_amd.models.detection import resized_size
from seam_match_rcnn_amd.ops import preprocess_u8_batch, preprocess_u8_flat      # the feature: absent, this file fails at import

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


def to_tensor(img):
    return img.permute(2, 0, 1).float().div(255).contiguous()


def images_of(shapes, seed):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in shapes]


def plan(shapes, min_size, max_size, d=32):
    sizes = [resized_size(h, w, min_size, max_size)[:2] for h, w in shapes]
    hp = int(math.ceil(max(s[0] for s in sizes) / d) * d)
    wp = int(math.ceil(max(s[1] for s in sizes) / d) * d)
    return sizes, hp, wp


CASES = {      # name: (image shapes, min_size, max_size, the resized sizes and padded frame these must give)
    # odd widths: image 1 starts at byte 37*53*3 = 5883 of the flat buffer, image 2 at 15099, both odd
    "mixed_odd": ([(37, 53), (64, 48), (50, 51)], 64, 96, ([(64, 91), (85, 64), (64, 65)], 96, 96)),
    # min side 64 -> scale 1: the sizes map to themselves and the kernel takes its no-resize branch
    "no_resize": ([(64, 80), (64, 64)], 64, 96, ([(64, 80), (64, 64)], 64, 96)),
    # x3.1 up (31 -> 96) and 301 -> 96, a 3.1x downscale: both limited by max_size
    "up_and_capped_down": ([(20, 31), (90, 301)], 64, 96, ([(61, 96), (28, 96)], 64, 96)),
    "single": ([(45, 67)], 64, 96, ([(64, 95)], 64, 96)),
    "degenerate_rows": ([(64, 1), (64, 2), (1, 64), (33, 2)], 64, 96, ([(96, 1), (96, 3), (1, 96), (96, 5)], 96, 96)),
}


def check(shapes, min_size, max_size, expect, flips, seed, host=True):
    imgs = images_of(shapes, seed)
    sizes, hp, wp = plan(shapes, min_size, max_size)
    assert (sizes, hp, wp) == expect                                 # the case is the one its name says
    floats = [(to_tensor(i).flip(-1) if f else to_tensor(i)).contiguous().to(DEV) for i, f in zip(imgs, flips)]
    n = len(imgs)
    for s2d in (False, True):
        want = ops.preprocess(floats, sizes, hp, wp, s2d=s2d)
        shape = (n, hp // 2, wp // 2, 12) if s2d else (n, hp, wp, 4)
        assert tuple(want.shape) == shape
        out = torch.full(shape, float("nan"), device=DEV)
        src = imgs if host else [i.to(DEV) for i in imgs]
        got = preprocess_u8_batch(src, sizes, hp, wp, flips, s2d, device=DEV, out=out)
        assert got is out and not bool(torch.isnan(got).any())
        assert torch.equal(got, want), (shapes, flips, s2d, float((got - want).abs().max()))
        assert torch.equal(preprocess_u8_batch(src, sizes, hp, wp, flips, s2d, device=DEV), want)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("flip", ["none", "all", "mixed"])
def test_batch_equals_the_fp32_path(name, flip):
    shapes, min_size, max_size, expect = CASES[name]
    flips = [dict(none=False, all=True, mixed=k % 2 == 0)[flip] for k in range(len(shapes))]
    check(shapes, min_size, max_size, expect, flips, seed=len(name))


def test_device_images_take_the_same_launch():
    check(*CASES["mixed_odd"], flips=[True, False, True], seed=3, host=False)


def test_refusals():
    img = images_of([(8, 9)], 0)[0]
    with pytest.raises(TypeError):
        preprocess_u8_batch([img.float()], [(8, 9)], 32, 32)
    with pytest.raises(ValueError, match=r"\[H,W,3\]"):
        preprocess_u8_batch([img.permute(2, 0, 1).contiguous()], [(8, 9)], 32, 32)
    with pytest.raises(ValueError):
        preprocess_u8_batch([], [], 32, 32)
    with pytest.raises(ValueError):
        preprocess_u8_batch([img], [(8, 9)], 32, 33, s2d=True)
    with pytest.raises(ValueError):
        preprocess_u8_batch([img], [(40, 9)], 32, 32)               # a resized size beyond the padded frame
    with pytest.raises(ValueError):
        preprocess_u8_batch([img, img.to(DEV)], [(8, 9)] * 2, 32, 32)
    flat = img.reshape(-1).to(DEV)
    off = torch.zeros(1, dtype=torch.int64)
    dims = torch.tensor([[8, 9, 8, 9, 0]], dtype=torch.int32)
    with pytest.raises(_native.SeamNativeError):                        # a table that lies on the host only
        preprocess_u8_flat(flat, off, dims.to(DEV), 32, 32, False)
    with pytest.raises(_native.SeamNativeError):
        preprocess_u8_flat(flat, off.to(DEV), dims, 32, 32, False)
    with pytest.raises(TypeError):
        preprocess_u8_flat(flat, off.to(DEV).to(torch.int32), dims.to(DEV), 32, 32, False)
    lib = _native.lib()
    st = torch.cuda.current_stream().cuda_stream
    out = torch.empty((1, 32, 32, 4), device=DEV)
    args = (flat.data_ptr(), flat.numel(), off.to(DEV).data_ptr(), dims.to(DEV).data_ptr(), out.data_ptr())
    bad = int(lib.seam_preprocess_u8_batch_f32(*args, 0, 32, 32, 0, st))
    assert bad != 0
    assert lib.seam_preprocess_u8_batch_f32(*args, 65536, 32, 32, 0, st) == bad
    assert lib.seam_preprocess_u8_batch_f32(*args, 1, 32, 33, 1, st) == bad
    assert lib.seam_preprocess_u8_batch_f32(*args, 1, 33, 32, 1, st) == bad
    assert lib.seam_preprocess_u8_batch_f32(args[0], args[1], None, args[3], args[4], 1, 32, 32, 0, st) == bad
    assert lib.seam_preprocess_u8_batch_f32(args[0], args[1], args[2], None, args[4], 1, 32, 32, 0, st) == bad


def test_an_entry_that_does_not_fit_is_written_as_zeros():
    """The kernel's own bound: a table entry that points past the buffer reads nothing and its frame is zeros."""
    img = images_of([(8, 9)], 1)[0]
    flat = img.reshape(-1).to(DEV)
    off = torch.tensor([0, 1], dtype=torch.int64, device=DEV)           # the second entry ends one byte past the buffer
    dims = torch.tensor([[8, 9, 8, 9, 0], [8, 9, 8, 9, 0]], dtype=torch.int32, device=DEV)
    out = preprocess_u8_flat(flat, off, dims, 32, 32, False, out=torch.full((2, 32, 32, 4), float("nan"), device=DEV))
    want = ops.preprocess([to_tensor(img).to(DEV)], [(8, 9)], 32, 32)
    assert torch.equal(out[0], want[0]) and bool((out[1] == 0).all())
