#!/usr/bin/env python3
"""One-off check of the ops.py split: every function and class of a commit's ``seam-match-rcnn_amd/ops.py`` against the definition of
the same name in the working tree's modules, source text against source text (decorators and docstrings included).

    python tools/ops_split_compare.py REV        (the commit before the split; run from anywhere inside the repository)

Prints one line per name that is missing or differs, then the counts.  Needs git and no GPU."""
import ast
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "seam-match-rcnn_amd"
MODULES = ("_ops_common", "ops", "ops_elementwise", "ops_input", "ops_heads", "ops_detect", "ops_train", "ops_masks", "pack_plan")


def definitions(text):
    """name -> source text of every top-level function and class, from the first decorator to the last line"""
    lines, out = text.split("\n"), {}
    for node in ast.parse(text).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            first = min([node.lineno] + [d.lineno for d in node.decorator_list])
            assert node.name not in out, node.name
            out[node.name] = "\n".join(lines[first - 1:node.end_lineno])
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    rev = sys.argv[1]
    before = definitions(subprocess.check_output(["git", "show", f"{rev}:{PKG}/ops.py"], cwd=ROOT, text=True))
    after, home = {}, {}
    for m in MODULES:
        for name, text in definitions(open(os.path.join(ROOT, PKG, m + ".py")).read()).items():
            assert name not in after, f"{name} is defined in {home[name]} and in {m}"
            after[name], home[name] = text, m
    differ = [n for n in before if n in after and after[n] != before[n]]
    missing = [n for n in before if n not in after]
    for n in missing:
        print(f"missing   {n}")
    for n in differ:
        print(f"differs   {n}  ({home[n]}.py)")
    per = {m: sum(1 for n in before if home.get(n) == m) for m in MODULES}
    print(f"{len(before)} functions and classes in {rev}:{PKG}/ops.py; identical {len(before) - len(differ) - len(missing)}, "
          f"differing {len(differ)}, missing {len(missing)}; new in the tree: {sorted(set(after) - set(before))}")
    print("where they are now: " + ", ".join(f"{m} {k}" for m, k in per.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
