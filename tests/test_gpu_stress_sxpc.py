"""Seeded random-geometry stress of the split-bf16 1x1 kernel family (csrc/seam_pwsx.hip): one body, ``sxpc_body``, behind seven
launch entries -- ``seam_conv1x1_sxpc``, ``_short``, ``_dual``, ``_dual_short``, ``_up``, ``seam_conv1x1_sxpc64`` and
``seam_stem_sxpc``.

The fixed-shape tests of these entries (``test_gpu_sxpc*.py``, ``test_gpu_stem_sxpc.py``) compare kernel with kernel along a chain
whose root is ``seam_conv2d_sx``; an error of ``sxpc_src_plan`` / ``sxpc_pixel``, common to three forms, would be compared with
itself.  Here every case (``sxpc_stress_cases.py``: 100 per family, steered through the image-lookup rules, Wo = 1, tiles that start
mid-image or span many images, ragged M, odd and even chunk counts, grids below the CU count and walks of several tiles per CU) is
checked against a float64 reference in plain torch under the project's gate, for the bits of ``seam_conv2d_sx(terms=6)``, twice
onto poisoned guarded outputs, with NaN behind every input and in every cell of x2 / ``top`` that must not be read.

The sweep runs in ONE child process (``stress_child_sxpc.py``) under a wall-clock limit: a kernel that hangs is a failure that names
the case it hung on."""
import os
import sys

import pytest

import stress_kit
import sxpc_stress_cases as SC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 100
SEED = 6
WALL_S = 240          # a hang shows as this timeout; the sweep itself takes well under 90 s
CHILD = os.path.join(ROOT, "tests", "stress_child_sxpc.py")


@pytest.fixture(scope="module")
def sweep():
    """One child process runs all seven families (one ``import torch``); its stdout is what the tests below read."""
    return stress_kit.run_child([sys.executable, CHILD, str(NCASE), str(SEED)], WALL_S, ROOT)


def _kernel_ok(sweep, name):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    assert int(f["cases"]) >= NCASE, f
    assert int(f["bit-identical"]) == int(f["cases"]), f
    for tag, least in SC.REQUIRED[name].items():        # recounted by the child with the device's CU count
        assert int(f.get(tag, 0)) >= least, (name, tag, f)
    return f


def test_stress_sxpc(sweep):
    _kernel_ok(sweep, "sxpc")


def test_stress_sxpc_short(sweep):
    _kernel_ok(sweep, "sxpc_short")


def test_stress_sxpc_dual(sweep):
    _kernel_ok(sweep, "sxpc_dual")


def test_stress_sxpc_dual_short(sweep):
    _kernel_ok(sweep, "sxpc_dual_short")


def test_stress_sxpc_up(sweep):
    _kernel_ok(sweep, "sxpc_up")


def test_stress_sxpc64(sweep):
    _kernel_ok(sweep, "sxpc64")


def test_stress_stem_sxpc(sweep):
    _kernel_ok(sweep, "stem_sxpc")


def test_stress_sweep_is_fast(sweep):
    """<= 90 s of sweep (the bound of test_gpu_stress.py for its seven families), measured inside the child."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    print("seconds per family", secs, "sum", round(sum(secs), 1))
    assert len(secs) == 7 and sum(secs) <= 90.0, secs
