"""Random-shape stress of the training gradient kernels (``csrc/seam_backward.hip``) through the C ABI.

``test_gpu_stress.py`` and ``test_gpu_stress_aux.py`` do this for the forward kernels; here the conv / linear weight gradient,
the column sum behind every bias gradient, the avg-pool + ReLU backward, BatchNorm1d (training forward and backward, frozen
too), the pairwise classifier's backward, the NLB + attention pooling backward (both entry points) and the weighted 2-class
cross entropy each get >= 100 seeded shapes aimed at their edges.  Every output and the workspace are POISONED with a 1 MiB
guard behind them; every case runs twice and the two results must be bit-identical (the kernels promise fixed-order
reductions).  Each result is compared with a plain float64 reference (``train_refs.py``, itself checked on the CPU by
``test_train_references.py``): bit for bit where the data are small integers whose partial sums stay below 2^24 (then fp32
is exact in any summation order, so a dropped or doubled chunk, split, slab or tap shows), else elementwise within
``C_ERR * 2^-24 * L * sum|terms|`` with the chain length L stated at each check.  Each launcher's refusals are called and
must leave every output untouched.

The sweep runs in ONE child process under a wall-clock timeout; the child prints every shape before launching it.
"""
import os
import sys

import pytest

import stress_kit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 100
WALL_S = 300          # a hang shows as this timeout; the sweep itself must stay under 120 s (test below)
CHILD = os.path.join(ROOT, "tests", "stress_child_train.py")


@pytest.fixture(scope="module")
def sweep():
    return stress_kit.run_child([sys.executable, CHILD, str(NCASE), "13"], WALL_S, ROOT)


def _family_ok(sweep, name):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    assert int(f["cases"]) >= NCASE and int(f["exact"]) >= NCASE // 10, f     # case count, and a share of exact cases
    return f


def test_stress_conv_wgrad(sweep):
    f = _family_ok(sweep, "conv_wgrad")
    assert int(f["one_split"]) >= 10 and int(f["single_tile"]) >= 10 and int(f["few_chunks"]) >= 10, f        # all three split regimes ran


def test_stress_colsum(sweep):
    _family_ok(sweep, "colsum")


def test_stress_avgpool_relu_bwd(sweep):
    _family_ok(sweep, "avgpool_relu_bwd")


def test_stress_bn1d(sweep):
    _family_ok(sweep, "bn1d")


def test_stress_pair_logits_bwd(sweep):
    _family_ok(sweep, "pair_logits_bwd")


def test_stress_nlb_bwd(sweep):
    f = _family_ok(sweep, "nlb_bwd")
    assert int(f["redraws"]) <= NCASE, f                    # redraws stay rare: the margin is not what the sweep tests


def test_stress_ce2(sweep):
    f = _family_ok(sweep, "ce2")
    assert int(f["nan"]) >= 1, f                        # the all-zero-weight NaN case ran


def test_stress_train_sweep_is_fast(sweep):
    """<= 120 s of sweep, measured inside the child (process start-up and ``import torch`` excluded)."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    assert len(secs) == 7 and sum(secs) <= 120.0, secs
