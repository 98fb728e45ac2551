"""Random-shape stress of the non-conv kernels on the hot path, through the C ABI.

``test_gpu_stress.py`` does this for the hand-scheduled convolutions; here the max-pools (the 3x3 / stride-2 kernel with its
multiply-high index divisions, and the generic one), the FPN's nearest upsample-add, the average pool, the four layout bridges and
RoIAlign (all three kernel forms) and the frame preprocess (normalise + bilinear resize + pad: per image, batched,
space-to-depth, space-to-depth with zero cells, uint8 input) each get >= 100 seeded random shapes.  Every launch writes a POISONED output with a 1 MiB guard
behind it, runs twice and must be bit-identical; each result is compared with a plain host reference in float64, or bit-exactly
where the operation is exact.  The generators aim at the edges: channel-group counts that are prime or odd up to ~4000 (the
shapes whose ``__umulhi`` divisions were inexact under the max-pool launcher's old rule -- both named regression shapes run in
both dtypes), all-negative maps, non-integer upsample ratios, 1 x 1 maps, boxes off every edge, zero-size and sub-pixel, box
sizes exactly on the FPN level boundaries, and one RoIAlign per run whose ROI lies past byte 2^31 of its level map.

The sweep runs in ONE child process under a wall-clock timeout; the child prints every shape before launching it.
"""
import os
import sys

import pytest

import stress_kit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 120
WALL_S = 180          # a hang shows as this timeout; the sweep itself must stay under 120 s (test below)
CHILD = os.path.join(ROOT, "tests", "stress_child_aux.py")


@pytest.fixture(scope="module")
def sweep():
    return stress_kit.run_child([sys.executable, CHILD, str(NCASE), "11"], WALL_S, ROOT)


def _family_ok(sweep, name):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    assert int(f["cases"]) >= NCASE, f
    return f


def test_stress_maxpool(sweep):
    f = _family_ok(sweep, "maxpool")
    assert int(f["fast"]) >= 20 and int(f["generic"]) >= 20, f        # both kernels really ran


def test_stress_upsample_add(sweep):
    _family_ok(sweep, "upsample_add")


def test_stress_avgpool(sweep):
    _family_ok(sweep, "avgpool")


def test_stress_layout_bridges(sweep):
    _family_ok(sweep, "transpose")


def test_stress_roi_align(sweep):
    _family_ok(sweep, "roi_align")


def test_stress_preprocess(sweep):
    _family_ok(sweep, "preprocess")


def test_stress_aux_sweep_is_fast(sweep):
    """<= 120 s of sweep, measured inside the child (process start-up and ``import torch`` excluded)."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    assert len(secs) == 6 and sum(secs) <= 120.0, secs
