"""GPU: the values ``split3_bf16`` / ``split3_bf16_single`` (csrc/seam_split.h) hand the matrix pipe, on the inputs where a cut can go
wrong -- denormals, +-0, values below 2^-110 (whose low pieces leave the normal range), alternating signs, values whose low pieces
are zero -- through one launch of every split 1x1 entry point on a 64-row problem: ``seam_conv2d_sx`` (conv_igemm_sx, six terms),
``seam_conv1x1_sxpc``, ``_dual``, ``_up``, ``seam_conv1x1_sxpc64`` and ``seam_stem_sxpc``.  Each kernel is its own instantiation of
the producers' cut, so each is launched.

Reference: an integer NumPy restatement of the cut (mask the top 16 bits of the word, subtract exactly, twice; the third piece is
the top 16 bits of what is left), then the product sum in float64, rounded to fp32.  Every output column reads ONE input column,
times a power of two (1, -2, 128, -1): every product and every partial sum is exact, so the order of the six terms and the
rounding of the sum do not enter and the comparison is byte for byte.  The model of the hardware in it: the VALU keeps fp32
subnormals, and the MFMA flushes neither its bf16 operands nor its fp32 accumulator, so a piece in the subnormal range counts as it
is; only what a subnormal remainder holds below its top 16 bits is lost.

Geometry per entry (all M = 64 rows of the same [64, 256] words, families by row):
  * conv2d_sx, conv1x1_sxpc, _up: C = K = 256, the smallest reduction conv1x1_sxpc serves (the issue's C = 64 is refused by it);
    column k reads column k.  _up adds a zero 4 x 4 top map to the 8 x 8 output map: +0 changes no sum.
  * _dual: the same rows as two sources, columns 0..63 (C1 = 64) and 64..255 (C2 = 192, stride 1) of one 8 x 8 map; the same pack.
  * conv1x1_sxpc64: K = 64, C = 256; column k reads column 4 k + k % 4 (both signs).
  * stem_sxpc: its rows are the 4 x 4 x 12 windows of a padded frame, which overlap, so a free [64, 192] matrix cannot be laid
    out; the words fill the whole [1, 11, 11, 12] frame (its border cells too: the entry reads the frame as given) and column k
    reads window element 3 k + k % 3 -- the diagonal form over the gathered rows.
``tests/test_gpu_split_identity.py`` pins the cut on every low-half bit pattern of the normal range; conv3x3_wino24sx applies the
(unchanged) cut to transformed values, which have no such closed form, and is pinned by ``tests/test_gpu_w24sx.py``."""
import numpy as np
import pytest
import torch

from test_gpu_sxpc import DEV, guarded

pytestmark = pytest.mark.gpu
M, C, K = 64, 256, 256
FACTORS = (1.0, -2.0, 128.0, -1.0)


def inputs():
    """[64, 256] fp32 words: each row one family, signs alternating along the row"""
    rng = np.random.RandomState(11)
    col = np.arange(C, dtype=np.uint32) % 64
    sign = (np.arange(C, dtype=np.uint32) & 1) << 31
    rows = []
    for r in range(M):
        fam = r % 8
        rnd = rng.randint(0, 1 << 23, C).astype(np.uint32)
        if fam == 0:      # denormals: every mantissa width, the smallest and the largest included
            w = np.where(col < 23, np.uint32(1) << (col % 23), rnd)
            w[-1] = 0x007fffff
        elif fam == 1:    # +-0 among ordinary values
            w = np.where(col % 3 == 0, np.uint32(0), (np.uint32(120) << 23) | rnd)
        elif fam == 2:    # 2^-126 .. 2^-111: the low pieces are denormal
            w = ((1 + col % 16).astype(np.uint32) << 23) | rnd
        elif fam == 3:    # low pieces zero: only the top 7 mantissa bits set
            w = ((100 + col).astype(np.uint32) << 23) | (rnd & 0x7f0000)
        elif fam == 4:    # middle piece zero, third piece not
            w = ((90 + col).astype(np.uint32) << 23) | (rnd & 0x7f00ff) | 1
        elif fam == 5:    # all-ones mantissas from the denormal border upwards
            w = ((col % 40).astype(np.uint32) << 23) | 0x7fffff
        elif fam == 6:    # one low bit only: the third piece is a single bit 23 places below the top
            w = ((1 + col * 2 % 120).astype(np.uint32) << 23) | (np.uint32(1) << (col % 16))
        else:             # ordinary values of every scale that stays finite under x 128
            w = ((1 + col * 3 % 240).astype(np.uint32) << 23) | rnd
        rows.append(w | sign)
    return np.stack(rows).astype(np.uint32)


def cut(words):
    """the three pieces as float64 arrays (each a bf16 value): truncate, subtract exactly, truncate, subtract exactly"""
    x = words.view(np.float32).astype(np.float64)
    p0 = (words & 0xffff0000).view(np.float32).astype(np.float64)
    r = (x - p0).astype(np.float32)
    assert np.array_equal(r.astype(np.float64), x - p0)                  # <= 16 significant bits: exact in fp32, subnormals kept
    p1 = (r.view(np.uint32) & 0xffff0000).view(np.float32).astype(np.float64)
    s = (r.astype(np.float64) - p1).astype(np.float32)
    assert np.array_equal(s.astype(np.float64), r.astype(np.float64) - p1)
    # while the remainders stay normal, <= 8 bits are left here, a bf16 as it stands; a subnormal remainder is fixed-point, more can
    # be left, and the third plane keeps the top 16 bits of the word like the other two
    p2 = (s.view(np.uint32) & 0xffff0000).view(np.float32).astype(np.float64)
    return p0, p1, p2


def reference(words, src, f):
    """fp32 bits of the six-term product: output column k = sum of the three pieces of words[:, src[k]], each times f[k]"""
    p0, p1, p2 = cut(words)
    total = 0.0 + p2[:, src] * f + p1[:, src] * f + p0[:, src] * f       # float64: exact; from +0 as the accumulator, so no -0 result
    want = total.astype(np.float32)
    assert np.array_equal(want.astype(np.float64), total) and np.all(np.isfinite(want))
    return want.view(np.uint32)


def diagonal(k, c, src):
    """(factors [k], weight [k, c] with factor k at column src[k])"""
    f = np.array([FACTORS[i % 4] for i in range(k)])
    wt = torch.zeros(k, c)
    wt[torch.arange(k), torch.from_numpy(src)] = torch.from_numpy(f).float()
    return f, wt


def dev(words):
    return torch.from_numpy(np.ascontiguousarray(words).view(np.float32)).to(DEV)


ENTRIES = ["seam_conv2d_sx", "seam_conv1x1_sxpc", "seam_conv1x1_sxpc_dual", "seam_conv1x1_sxpc_up", "seam_conv1x1_sxpc64", "seam_stem_sxpc"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_special_values_byte_for_byte(entry):
    from seam_match_rcnn_amd import _native, ops
    lib, P, st = _native.lib(), ops._ptr, ops._stream()
    words = inputs()
    if entry == "seam_stem_sxpc":
        frame = np.ascontiguousarray(words.T).reshape(-1)[:11 * 11 * 12].reshape(11, 11, 12)       # every family, both signs
        rows = np.lib.stride_tricks.sliding_window_view(frame, (4, 4), axis=(0, 1))                 # [8, 8, 12, r, s]
        rows = np.ascontiguousarray(rows.transpose(0, 1, 3, 4, 2)).reshape(M, 192)                  # (r, s, c) order
        k, src = 64, 3 * np.arange(64) + np.arange(64) % 3
    elif entry == "seam_conv1x1_sxpc64":
        rows, k, src = words, 64, 4 * np.arange(64) + np.arange(64) % 4
    else:
        rows, k, src = words, K, np.arange(K)
    f, wt = diagonal(k, rows.shape[1], src)
    want = reference(rows, src, f)
    pc = ops.pack_conv(wt.view(k, rows.shape[1], 1, 1).to(DEV), dtype=ops.SX6)
    x = dev(rows)
    y, intact = guarded(M, k)
    if entry == "seam_conv2d_sx":
        rc = lib.seam_conv2d_sx(P(x), P(pc.w), None, None, None, P(y), 1, M, 1, C, K, 1, 1, 1, 0, 0, 6, st)
    elif entry == "seam_conv1x1_sxpc":
        assert pc.wx is not None
        rc = lib.seam_conv1x1_sxpc(P(x), P(pc.wx), None, None, None, P(y), M, C, K, 0, st)
    elif entry == "seam_conv1x1_sxpc_dual":
        assert pc.wx is not None
        x1, x2 = dev(rows[:, :64]), dev(rows[:, 64:])
        rc = lib.seam_conv1x1_sxpc_dual(P(x1), P(x2), P(pc.wx), None, None, P(y), 1, 8, 8, 64, 8, 8, 192, 1, K, 0, st)
    elif entry == "seam_conv1x1_sxpc_up":
        assert pc.wx is not None
        top = torch.zeros((1, 4, 4, K), device=DEV)
        rc = lib.seam_conv1x1_sxpc_up(P(x), P(pc.wx), None, None, P(top), P(y), 1, 8, 8, C, K, 4, 4, 0, st)
    elif entry == "seam_conv1x1_sxpc64":
        assert pc.wx64 is not None
        rc = lib.seam_conv1x1_sxpc64(P(x), P(pc.wx64), None, None, None, P(y), M, C, 64, 0, st)
    else:
        assert pc.wx64 is not None
        xp = dev(frame).view(1, 11, 11, 12)
        rc = lib.seam_stem_sxpc(P(xp), P(pc.wx64), None, None, P(y), 1, 8, 8, 0, st)
    torch.cuda.synchronize()
    assert rc == 0 and intact(), (entry, rc)
    got = y.cpu().numpy().view(np.uint32)
    diff = got != want
    fams = sorted(set(np.nonzero(diff)[0] % 8)) if entry != "seam_stem_sxpc" else "-"
    print(f"split3 values through {entry}: {int(diff.sum())} of {diff.size} words differ (input families {fams})")
    for r, c in list(zip(*np.nonzero(diff)))[:6]:
        print(f"  row {r} col {c}: x {rows[r, src[c]]:#010x} x {f[c]:g}: got {got[r, c]:#010x} want {want[r, c]:#010x}")
    assert int(diff.sum()) == 0, entry
