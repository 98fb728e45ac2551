"""Random-shape stress of the hand-scheduled kernels through the C ABI.

``conv3x3_wino24pc`` (persistent producer / consumer Winograd F(2x4,3x3), hand-counted ``vmcnt`` waits, a cross-tile software
pipeline, cached per-region addresses, 24-bit multiplies guarded by launcher caps), ``conv1x1_pc``, ``conv3x3_f16pc``,
``conv1x1_sw``, ``conv1x1_swh``, ``conv1x1_f16pc`` and the fp16 stem on the streaming kernel (round 6) each get >= 200 seeded random shapes: every launch goes onto a POISONED output, twice, and must be bit-identical;
results are compared with the implicit GEMM (``seam_conv2d_f32`` / ``_f16``) AND with a plain torch fp32 convolution of the same
operands (tap-wise ``matmul`` form for every shape -- no per-shape MIOpen search -- and ``F.conv2d`` itself on a sample).
Unserved channel counts must be REFUSED (non-zero return), not hang.  Shapes cover N in [1, 3000], H, W in [3, 210] including
primes, pad 0 / 1, every epilogue mode, grids smaller than the CU count (one tile, one tile per XCD), tile ranges that end
mid-region, and the launcher's 2^31-byte cap from both sides.  (The ``blocks >= 2^24`` cap is hit from the refusing side only:
a launch just under it needs a 1 TB output.)

The whole sweep runs in ONE child process under a wall-clock timeout, so a kernel that hangs is a test FAILURE that names the
shape it hung on (the child prints every shape before launching it) -- not a lost GPU lease.  The reference's own layers are
shape-polymorphic in the same way: ``MatchPredictor.conv_seq`` (/root/reference/models/match_head.py:50-62) runs on whatever ROI
count arrives.
"""
import os
import sys

import pytest

import stress_kit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 200
WALL_S = 240          # a hang shows as this timeout; the sweep itself takes well under 90 s
CHILD = os.path.join(ROOT, "tests", "stress_child_conv.py")


@pytest.fixture(scope="module")
def sweep():
    """One child process runs all seven sweeps (one ``import torch``); its stdout is what the tests below read."""
    return stress_kit.run_child([sys.executable, CHILD, str(NCASE), "6"], WALL_S, ROOT)


def _kernel_ok(sweep, name):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    assert int(f["cases"]) >= NCASE, f
    return f


def test_stress_conv3x3_wino24pc(sweep):
    f = _kernel_ok(sweep, "wino24pc")
    # the sweep really reached the small-grid corners
    assert int(f["grids<256"]) >= 20 and int(f["grids<=8"]) >= 5 and int(f["ragged-XCD-ranges"]) >= 20, f


def test_stress_conv1x1_pc(sweep):
    _kernel_ok(sweep, "conv1x1_pc")


def test_stress_conv3x3_f16pc(sweep):
    _kernel_ok(sweep, "f16pc")


def test_stress_conv1x1_sw(sweep):
    _kernel_ok(sweep, "conv1x1_sw")


def test_stress_conv1x1_swh(sweep):
    _kernel_ok(sweep, "conv1x1_swh")


def test_stress_stem_swh(sweep):
    _kernel_ok(sweep, "stem_swh")


def test_stress_conv1x1_f16pc(sweep):
    _kernel_ok(sweep, "conv1x1_f16pc")


def test_stress_sweep_is_fast(sweep):
    """<= 90 s of sweep (VERDICT's bound), measured inside the child (process start-up and ``import torch`` excluded)."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    assert len(secs) == 7 and sum(secs) <= 90.0, secs
