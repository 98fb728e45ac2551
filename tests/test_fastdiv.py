"""CPU: the one rule for the kernels' multiply-high divisions (csrc/seam_fastdiv.h, exported as ``seam_fastdiv_exact``).

A kernel computes n / d as ``__umulhi(n, ceil(2^32 / d))``.  Whenever the helper says "exact" for (d, n_max), numpy replays that
arithmetic and it must equal n // d (for every n < n_max up to 2e7, past that on the numerators that can fail first); the helper must say "not exact" for the max-pool shapes that were computed
wrongly under the launcher's old ``per_img < 2^31`` rule; and the model's own max-pool shapes must keep the 32-bit kernel.
"""
import os
import random
import subprocess

import numpy as np
import pytest

from conftest import ROOT

NMAX_SCAN = 20_000_000          # pairs with a larger n_max are scanned on the residues that can fail (n = k d - 1)


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    if not os.path.exists(_native.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "seam-match-rcnn_amd", "csrc"), "-j4"], check=True)
    return _native.lib()


def magic(d):
    return 0 if d <= 1 else ((1 << 32) + d - 1) // d


def umulhi_div(n, d):
    """The device's quotient for uint64 numerators n (< 2^32)."""
    if d == 1:
        return n
    m = np.uint64(magic(d))
    lo, hi = n & np.uint64(0xFFFF), n >> np.uint64(16)          # n * m overflows 64 bits: split n
    return ((hi * m) + ((lo * m) >> np.uint64(16))) >> np.uint64(16)


def first_wrong(d, n_max):
    """Smallest n < n_max with umulhi_div(n) != n // d, or None.  Every n is scanned up to NMAX_SCAN; past that, the numerators
    n = k d - 1 only -- the error term n e / (d 2^32) grows with n and r = d - 1 leaves it the least room -- the largest 2^22 of
    them and the smallest 2^16 (so a failure is found wherever the quotient can go wrong at all)."""
    if n_max <= NMAX_SCAN:
        chunks = [np.arange(lo, min(n_max, lo + (1 << 22)), dtype=np.uint64) for lo in range(0, n_max, 1 << 22)]
    else:
        kmax = n_max // d               # n = k d - 1 < n_max for k <= kmax (when k d - 1 < n_max)
        ks = np.concatenate([np.arange(1, min(kmax, 1 << 16) + 1), np.arange(max(1, kmax - (1 << 22)), kmax + 1)])
        n = np.unique(ks.astype(np.uint64) * np.uint64(d) - np.uint64(1))
        chunks = [n[n < np.uint64(n_max)]]
    for n in chunks:
        bad = np.nonzero(umulhi_div(n, d) != n // np.uint64(d))[0]
        if bad.size:
            return int(n[bad[0]])
    return None


def maxpool_pairs(n, h, w, c, f16):
    ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    cv = c // (8 if f16 else 4)
    return [(cv, ho * wo * cv), (wo, ho * wo)]


# the model's stem max-pools: fp32 800^2 frames (400^2 stem output), fp16 1080p (the 1088 x 1920 padded frame: 544 x 960)
MODEL_POOLS = [(80, 400, 400, 64, 0), (8, 400, 400, 64, 0), (240, 544, 960, 64, 1), (30, 544, 960, 64, 1), (2, 64, 80, 64, 0)]
# (shape, dtype) computed wrongly by the old launcher: cv = 3906 (e = 3556) at 17 x 17 outputs, cv = 250 at 320 x 1000 outputs
REGRESSION_POOLS = [(1, 34, 34, 15624, 0), (1, 34, 34, 31248, 1), (1, 640, 2000, 1000, 0), (1, 640, 2000, 2000, 1)]


def test_rule_against_exhaustive_umulhi(lib):
    rng = random.Random(2024)
    pairs = [(3906, 1_128_834), (250, 80_000_000), (3, 1 << 31), (7, 1 << 32), (641, 6_700_417), (2, 1 << 32), (1, 1 << 32),
             (1 << 16, 1 << 32), (65537, 65_536), (3906, 1_000_000), (200, 40_000), (480, 130_560)]
    for (n, h, w, c, f16) in MODEL_POOLS + REGRESSION_POOLS:
        pairs += maxpool_pairs(n, h, w, c, f16)
    for _ in range(60):
        d = rng.choice([rng.randint(2, 64), rng.randint(2, 5000), rng.randint(2, 1 << 20), rng.randint(2, (1 << 32) - 1)])
        e = magic(d) * d - (1 << 32)
        edge = (1 << 32) // e + 1 if e else rng.randint(1, 1 << 24)   # the sharp rule's boundary: n_max - 1 = floor(2^32 / e)
        n_max = rng.choice([rng.randint(1, 1 << 21), rng.randint(1, NMAX_SCAN), edge, edge + 1, max(1, edge - 1)])
        pairs.append((d, min(n_max, 1 << 32)))
    exact_seen = inexact_seen = 0
    for d, n_max in pairs:
        ok = lib.seam_fastdiv_exact(d, n_max)
        e = magic(d) * d - (1 << 32) if d > 1 else 0
        assert ok == int(d == 1 or n_max <= 1 or (n_max - 1) * e < (1 << 32)), (d, n_max)
        if ok:
            exact_seen += 1
            assert first_wrong(d, n_max) is None, (d, n_max)
        else:
            inexact_seen += 1
    assert exact_seen >= 30 and inexact_seen >= 10, (exact_seen, inexact_seen)


def test_rule_refuses_the_wrong_maxpool_shapes(lib):
    assert lib.seam_fastdiv_exact(3906, 1_128_834) == 0
    assert lib.seam_fastdiv_exact(250, 80_000_000) == 0
    # and those two really go wrong: the first bad numerator of each (the fp32 [1, 34, 34, 15624] case at i = 1101491)
    assert first_wrong(3906, 1_128_834) == 1_101_491
    assert first_wrong(250, 80_000_000) is not None
    for (n, h, w, c, f16) in REGRESSION_POOLS:
        assert lib.seam_maxpool2d_fast(n, h, w, c, 3, 2, 1, f16) == 0, (n, h, w, c, f16)
    # d = 0, numerators past 32 bits: never exact; d = 1 is (every device helper takes n itself)
    assert lib.seam_fastdiv_exact(0, 10) == 0 and lib.seam_fastdiv_exact(3, (1 << 32) + 1) == 0
    assert lib.seam_fastdiv_exact(1, 1 << 32) == 1


def test_model_maxpools_keep_the_fast_kernel(lib):
    for (n, h, w, c, f16) in MODEL_POOLS:
        assert lib.seam_maxpool2d_fast(n, h, w, c, 3, 2, 1, f16) == 1, (n, h, w, c, f16)
        for d, n_max in maxpool_pairs(n, h, w, c, f16):
            assert lib.seam_fastdiv_exact(d, n_max) == 1
    # other windows, odd channel counts: the generic kernel
    assert lib.seam_maxpool2d_fast(2, 50, 50, 64, 1, 2, 0, 0) == 0 and lib.seam_maxpool2d_fast(2, 50, 50, 60, 3, 2, 1, 1) == 0
