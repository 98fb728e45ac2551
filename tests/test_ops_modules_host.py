"""CPU: the module layout of the launch wrappers.  ``ops.py`` holds the convolutions and is the public namespace; the other kernel
families live in leaf modules beside it, which import only ``torch``, ``_native``, ``_ops_common`` and each other; ``pack_plan``
sits above ``ops``.  Checked here: the import rule (an AST scan), that import order does not matter (a fresh interpreter per leaf),
that the knobs assigned from outside exist only where they are read, and that every ``ops.<name>`` the repository used before the
split still resolves."""
import ast
import os
import subprocess
import sys

import pytest

from conftest import ROOT

PKG = os.path.join(ROOT, "seam-match-rcnn_amd")
LEAVES = ("ops_elementwise", "ops_input", "ops_heads", "ops_detect", "ops_train", "ops_masks")
# assigned by tests and tools: a star import into ``ops`` would leave a dead copy there, so they are not re-exported
KNOBS = {"NLB_MFMA": "ops_heads", "PAIR_MFMA": "ops_heads", "WGRAD_MAX_OPERAND_BYTES": "ops_train",
         "RLE_BITS_BUDGET_BYTES": "ops_masks", "_staging": "ops_input"}


def package_imports(module):
    """Names of the package's own modules that ``module``.py imports, at any depth of nesting (``from . import a``: ``a``;
    ``from .a.b import c``: ``a.b``); absolute imports of the package count too."""
    tree = ast.parse(open(os.path.join(PKG, module + ".py")).read())
    found = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.ImportFrom):
            if node.level == 1:
                found |= {node.module} if node.module else {a.name for a in node.names}
            elif node.level == 0 and node.module and node.module.split(".")[0] == "seam_match_rcnn_amd":
                rest = node.module.split(".", 1)
                found |= {rest[1]} if len(rest) > 1 else {a.name for a in node.names}
            else:
                assert node.level == 0, f"{module}: an import from above the package"
        elif isinstance(node, ast.Import):
            found |= {a.name.split(".", 1)[1] for a in node.names if a.name.startswith("seam_match_rcnn_amd.")}
    return found


def test_the_import_rule_holds():
    allowed = {"_native", "_ops_common", *LEAVES}
    assert package_imports("_ops_common") == {"_native"}
    for leaf in LEAVES:
        got = package_imports(leaf)
        assert got <= allowed - {leaf}, f"{leaf} imports {sorted(got - allowed)}"
        assert "_ops_common" in got
    ops = package_imports("ops")
    assert ops == {"_native", "_ops_common", *LEAVES}, sorted(ops)          # every leaf, and nothing of the model layer
    assert not any(m.split(".")[0] == "models" for m in ops)
    assert package_imports("pack_plan") == {"_native", "_ops_common", "ops", "models.packed"}


def test_ops_ends_with_one_star_import_per_leaf():
    body = ast.parse(open(os.path.join(PKG, "ops.py")).read()).body
    tail = body[-len(LEAVES):]
    assert all(isinstance(n, ast.ImportFrom) and n.level == 1 and [a.name for a in n.names] == ["*"] for n in tail)
    assert sorted(n.module for n in tail) == sorted(LEAVES)
    assert not any(isinstance(n, ast.ImportFrom) and n.names[0].name == "*" for n in body[:-len(LEAVES)])


CHILD = """
import importlib, sys
first, knobs = sys.argv[1], dict(k.split("=") for k in sys.argv[2:])
leaf = importlib.import_module("seam_match_rcnn_amd." + first)
from seam_match_rcnn_amd import ops
for name in leaf.__all__:
    assert getattr(ops, name) is getattr(leaf, name), name
assert not set(knobs) & set(leaf.__all__)
for name, home in knobs.items():
    assert not hasattr(ops, name), name
    assert hasattr(importlib.import_module("seam_match_rcnn_amd." + home), name), name
print("ok", len(leaf.__all__))
"""


@pytest.mark.parametrize("leaf", LEAVES)
def test_a_leaf_imported_first_still_lands_on_ops(leaf):
    """Import order is the hazard of the split: any single leaf first, then ``ops``, in an interpreter of its own.  The knobs are
    looked up in the same run: absent from ``ops`` (reading one there is an AttributeError), present where they are read."""
    res = subprocess.run([sys.executable, "-c", CHILD, leaf] + [f"{k}={v}" for k, v in KNOBS.items()], cwd=ROOT,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.split()[0] == "ok" and int(res.stdout.split()[1]) > 0


def test_all_lists_every_public_name_but_the_knobs():
    import importlib
    for leaf in LEAVES:
        mod = importlib.import_module("seam_match_rcnn_amd." + leaf)
        tree = ast.parse(open(os.path.join(PKG, leaf + ".py")).read())
        defined = [n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))]
        defined += [e.id for n in tree.body if isinstance(n, ast.Assign) for t in n.targets for e in ast.walk(t) if isinstance(e, ast.Name)]
        public = {n for n in defined if not n.startswith("_")} - set(KNOBS)
        assert set(mod.__all__) == public, (leaf, sorted(set(mod.__all__) ^ public))
        assert len(mod.__all__) == len(set(mod.__all__))


def test_every_name_used_through_ops_before_the_split_resolves():
    """tests/golden/ops_names.txt: the ``ops.<name>`` uses of the package, the tests, the tools, bench.py, __graft_entry__.py,
    INTEGRATION.md and DESIGN.md before the split -- without the knobs above and without ``PackPlan`` (in ``pack_plan``,
    which ``ops`` cannot import: it is the module above).  The private helpers among them (``_upload``, ``_launch_noise``,
    ``_resized_tables``, ``_topk_k``) are imported into ``ops`` by name."""
    from seam_match_rcnn_amd import ops
    names = open(os.path.join(ROOT, "tests", "golden", "ops_names.txt")).read().split()
    assert len(names) == 154 and len(set(names)) == 154
    missing = [n for n in names if not hasattr(ops, n)]
    assert not missing, missing
    for n in ("CONV_TRACE", "BX3", "cat_rows", "pair_topk", "rank_topk", "_ptr", "_stream", "FRAME_RGB", "SAMPLE_MAX_CANDIDATES", "sgd_chunk_table", "_upload",
              "_topk_k"):
        assert n in names
