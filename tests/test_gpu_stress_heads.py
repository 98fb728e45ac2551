"""Random-shape stress of the match-head and ranking kernels (``csrc/seam_heads.hip``, ``seam_topk.h``, ``seam_pairmf.hip``,
``seam_narrow.hip``) through the C ABI -- the sweep the other kernel families already have (``test_gpu_stress*.py``).

Eight families, >= 100 seeded cases each (16 for the 8 MB banks of the matrix-core top-k), aimed at their edges: the pairwise
classifier (every D, the Q / G tails of both tiles, both sides of the tile switch at Q G = 2^20), the ranking kernels
(rank_topk / rank_of / rank_of_scores / match_scores on logits full of ties, NaN, +-inf, -0.0 against +0.0, constant and
all-NaN rows, k up to the 256-winner capacity), the fused top-k (last segments shorter than k, whole NaN / -inf queries),
the matrix-core top-k, the block-diagonal self-similarity, the score reductions, the non-local block + attention pooling in
its VALU and MFMA forms (every length edge, both layouts, padded strides, len > Tmax, len < 0, att / z present or NULL) and
the narrow linear layer.  Every output and workspace is POISONED (NaN in one run, 3e4 in the other, an integer pattern for
idx / rank / stats) with a 1 MiB guard behind it; every case runs twice and the two results must be bit-identical; each
launcher's refusals must return non-zero and leave every output untouched (k = 257 on ``seam_rank_topk_f32`` is the regression
test of the capacity check).

References and tolerances come from ``heads_refs.py`` (checked on the CPU by ``test_heads_references.py``): indices and ranks
exact; integer-grid data bit for bit against float64; sums within ``train_refs.bound(majorant, L)`` with L at each check;
scores within ``(|d| + 6) 2^-24 ref + FLT_MIN`` of the float64 score of the device's own logits (1-ulp expf, correctly rounded
division: derived, the ROCm installation has no accuracy table); the NLB stage by stage, its block stage with the MEASURED
constant NLB_BLOCK_RHO = 1.376e-4 = 4 x 3.44e-5, the worst error of the fp32 CPU oracle relative to the propagated worst-case
bound on Z over the 100 cases of this sweep (the derived bound is ~3e4 x fp32's real error and has no teeth).  The worst
observed error / bound per family is printed in its SUMMARY line and must stay below 1.

The sweep runs in ONE child process under a wall-clock timeout; the child prints every case before launching it.
"""
import os
import sys

import pytest

import stress_kit

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCASE = 100
WALL_S = 300          # a hang shows as this timeout; the sweep itself must stay under 120 s (test below)
CHILD = os.path.join(ROOT, "tests", "stress_child_heads.py")


@pytest.fixture(scope="module")
def sweep():
    return stress_kit.run_child([sys.executable, CHILD], WALL_S, ROOT)


def _family_ok(sweep, name, ncase=NCASE, exact=True):
    f = stress_kit.family_ok(sweep, name, WALL_S)
    assert int(f["cases"]) >= ncase, f                    # every case ran: none is skipped or left out
    if exact:
        assert int(f["exact"]) >= ncase // 10, f          # a share of bit-exact cases
    if "worst" in f:
        assert float(f["worst"]) < 1.0, f                 # worst observed error / bound
    return f


def test_stress_pair_logits(sweep):
    f = _family_ok(sweep, "pair_logits")
    assert int(f["tile4x4"]) >= 3 and 0 < float(f["worst"]), f          # both tiles ran, and the bound was exercised


def test_stress_rank(sweep):
    f = _family_ok(sweep, "rank")
    assert 0 < float(f["worst"]), f
    out = sweep["out"]
    for desc in ("k>G", "k257 G257", "k257 G1000", "k5000 G5000"):      # the capacity check: k = 257 is refused
        assert f"START rank refuse {desc}" in out and not [ln for ln in out.splitlines() if ln.startswith(f"FAIL rank {desc}")]


def test_stress_pair_topk(sweep):
    f = _family_ok(sweep, "pair_topk")
    assert int(f["shortseg"]) >= 10, f                                  # last segments shorter than k


def test_stress_pair_topk_mfma(sweep):
    _family_ok(sweep, "pair_topk_mfma", ncase=16, exact=False)
    assert len([ln for ln in sweep["out"].splitlines() if ln.startswith("STATS pair_topk_mfma")]) >= 16


def test_stress_blockdiag(sweep):
    _family_ok(sweep, "blockdiag")


def test_stress_score_reduce(sweep):
    _family_ok(sweep, "score_reduce")


def test_stress_nlb(sweep):
    f = _family_ok(sweep, "nlb", exact=False)
    assert int(f["both_forms"]) >= 70 and int(f["scratch_path"]) >= 10 and 0 < float(f["worst"]), f


def test_stress_linear_narrow(sweep):
    _family_ok(sweep, "linear_narrow")


def test_stress_heads_sweep_is_fast(sweep):
    """<= 120 s of sweep, measured inside the child (process start-up and ``import torch`` excluded)."""
    secs = [float(ln.split()[-1]) for ln in sweep["out"].splitlines() if ln.startswith("SUMMARY")]
    assert len(secs) == 8 and sum(secs) <= 120.0, secs
