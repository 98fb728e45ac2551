"""split3_bf16 (csrc/seam_split.h) pinned through the kernels that use it on activations: ``seam_conv1x1_sxpc`` (its producers)
and ``seam_conv2d_sx`` (conv_igemm_sx).  With ``w = I`` (C = K = 256) the six-term product of a row is the sum of the row's three
bf16 pieces, lowest first, which is the value itself when -- and only when -- the truncation split is exact and every element keeps
its own top piece; with ``w = 2^-20 I`` the same pieces meet a scaled weight.  So ``y`` must equal ``x w`` bit for bit.

The inputs are every one of the 2^16 low-half bit patterns combined with four high-mantissa patterns, eight exponents from 2^-100
to the binade of FLT_MAX and both signs: 2^22 values, M = 16 384 rows of 256.  A row's columns are rotated by 17 x (the value's
upper six index bits), so every low-half pattern appears in each of the four slots of a 16-byte vector and in chunks of both
parities (asserted below): a packed-operation fold that gives an element its neighbour's top piece cannot hide in one slot."""
import numpy as np
import pytest
import torch

from test_gpu_sxpc import DEV, both

gpu = pytest.mark.gpu
HIGH = (0x00, 0x7f, 0x55, 0x2a)                         # mantissa bits 16..22
EXPONENTS = (27, 60, 100, 126, 127, 150, 200, 254)      # biased: 2^-100 ... the binade of FLT_MAX
_X = []


def patterns():
    """x [16384, 256] on the host (built once)"""
    if not _X:
        v = np.arange(1 << 22, dtype=np.uint32)
        low, g = v & 0xffff, v >> 16
        word = ((g >> 5) << 31) | (np.array(EXPONENTS, dtype=np.uint32)[(g >> 2) & 7] << 23) | (np.array(HIGH, dtype=np.uint32)[g & 3] << 16) | low
        col = ((v & 255) + 17 * g) & 255
        x = np.empty((1 << 14, 256), dtype=np.uint32)
        x[v >> 8, col] = word
        # every low-half pattern in every vector slot and in chunks of both parities
        seen = np.bincount((low.astype(np.int64) << 3) | ((col & 3) << 1).astype(np.int64) | ((col >> 6) & 1).astype(np.int64), minlength=1 << 19)
        assert seen.shape[0] == 1 << 19 and int(seen.min()) >= 1
        assert np.unique(x).shape[0] == 1 << 22
        _X.append(torch.from_numpy(x.view(np.float32)))
    return _X[0]


@gpu
@pytest.mark.parametrize("factor", [1.0, 2.0 ** -20])
def test_identity_weights_return_the_input_bits(factor):
    from seam_match_rcnn_amd import ops
    x = patterns().to(DEV)
    assert bool(torch.isfinite(x).all())
    pc = ops.pack_conv((torch.eye(256) * factor).view(256, 256, 1, 1).to(DEV), dtype=ops.SX6)
    assert pc.wx is not None
    want = x * factor                                   # exact: a power of two, no result below the normal range
    assert bool((want.abs() >= 2.0 ** -126).all())
    igemm, sxpc = both(x, pc)
    for name, y in (("seam_conv2d_sx", igemm), ("seam_conv1x1_sxpc", sxpc)):
        wrong = int((y.view(torch.int32) != want.view(torch.int32)).sum())
        print(f"split identity x {factor:g} through {name}: {wrong} of {y.numel()} words differ")
        assert wrong == 0, name
