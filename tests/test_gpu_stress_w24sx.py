"""Seeded random-geometry stress of ``conv3x3_wino24sx`` (csrc/seam_wino24sx.hip, body ``w24_block<2, HS, true>``) and, on the same
operands, of the fp32 F(2x4) kernels behind ``seam_conv3x3_wino24_f32``.

The fixed tables (``w24_layout_cases.py``, ``test_gpu_w24sx.py``) pin every block layout on small problems: C <= 256, K <= 256,
N <= 7.  Here every case (``w24sx_stress_cases.py``: 100, steered through every reachable layout class x HS class, reductions up to
C = 512, up to 16 n-tiles, batches up to 4096 images, grids from one block to more than three per CU, every epilogue -- the ReLU
mask included --, packs with zero-filled channels and with rotated taps) is checked against a float64 reference in plain torch
under the project's own gates, twice onto poisoned guarded outputs, with NaN around every input, one image alone against the same
image in the batch bit for bit, and under forced n-tile splits 2, 4 and 8 with padding blocks.

Gates (``stress_child_w24sx.py``): e_w24 <= 3e-5 for the fp32 kernel; e_new <= 3 e_w24 + 1e-7 and |y_new - y_exact| <= 2e-5 scale
for the split kernel.  Measured figures: profiles/w24sx_stress_sweep.txt.

The sweep runs in ONE child process under a wall-clock limit: a kernel that hangs is a failure that names the case it hung on."""
import os
import sys

import pytest

import stress_kit
import w24sx_stress_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 100
SEED = 6
WALL_S = 240          # the limit of the sibling sweeps; a hang shows as this timeout
CHILD = os.path.join(ROOT, "tests", "stress_child_w24sx.py")


@pytest.fixture(scope="module")
def sweep():
    """One child process runs both families over the one case list; its stdout is what the tests below read."""
    return stress_kit.run_child([sys.executable, CHILD, str(NCASE), str(SEED)], WALL_S, ROOT)


def _kernel_ok(sweep, name):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    assert int(f["cases"]) >= NCASE, f
    assert int(f["bit-identical"]) == int(f["cases"]), f
    for tag, least in SC.REQUIRED.items():              # recounted by the child with the device's CU count
        assert int(f.get(tag, 0)) >= least, (name, tag, f)
    return f


def test_stress_w24sx(sweep):
    f = _kernel_ok(sweep, "w24sx")
    assert int(f["forced-splits"]) >= 15 and int(f["ragged-partitions"]) >= 1, f
    print("\n".join(ln for ln in sweep["out"].splitlines() if ln.startswith("RANGE")))


def test_stress_w24f32(sweep):
    _kernel_ok(sweep, "w24f32")


def test_stress_sweep_is_fast(sweep):
    """<= 90 s of sweep (the bound every sweep of this project keeps), measured inside the child."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    print("seconds per family", secs, "sum", round(sum(secs), 1))
    assert len(secs) == 2 and sum(secs) <= 90.0, secs
