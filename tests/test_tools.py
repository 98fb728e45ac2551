"""Host-side tools that shape the committed evidence (no GPU)."""
import csv
import importlib.util
import io
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trace(path, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f, quoting=csv.QUOTE_ALL)
        w.writerow(["Kind", "Kernel_Name", "Start_Timestamp", "End_Timestamp"])
        for name, t0, t1 in rows:
            w.writerow(["KERNEL_DISPATCH", name, t0, t1])


def test_kernel_trace_steps_keeps_the_timed_region_only(tmp_path):
    """tools/kernel_trace_steps.py: per-kernel statistics of the dispatches BETWEEN the two marker launches bench.py brackets its timed
    region with -- the bank pass / warm-up before and the instrumented legs behind are left out; rows may come in any order."""
    rows = [("conv_a", 100, 110), ("conv_a", 120, 150),                         # bank pass / warm-up
            ("void at::native::spin_kernel(long)", 200, 201),
            ("conv_a", 300, 400), ("conv_b", 410, 430), ("conv_a", 500, 700),   # the timed steps
            ("void at::native::spin_kernel(long)", 800, 801),
            ("conv_a", 900, 5000)]                                              # an instrumented leg
    p = tmp_path / "b_kernel_trace.csv"
    _trace(p, list(reversed(rows)))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_trace_steps.py"), str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = {row["Name"]: row for row in csv.DictReader(io.StringIO(r.stdout))}
    assert set(out) == {"conv_a", "conv_b"}
    assert int(out["conv_a"]["Calls"]) == 2 and float(out["conv_a"]["AverageNs"]) == 150.0 and int(out["conv_a"]["MaxNs"]) == 200
    assert int(out["conv_b"]["Calls"]) == 1 and float(out["conv_b"]["TotalDurationNs"]) == 20.0
    assert "3 dispatches of 8" in r.stderr


def test_kernel_trace_steps_needs_both_markers(tmp_path):
    p = tmp_path / "t.csv"
    _trace(p, [("conv_a", 1, 2), ("void at::native::spin_kernel(long)", 3, 4), ("conv_a", 5, 6)])
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_trace_steps.py"), str(p)], capture_output=True, text=True)
    assert r.returncode != 0 and "marker" in r.stderr


def test_isa_same_compares_kernels_not_comments_or_cuids():
    """tools/isa_same.py: the same device code with another __hip_cuid_<hash> and other comments is equal; one changed instruction is a
    difference, reported under its kernel's label with the first differing line."""
    spec = importlib.util.spec_from_file_location("isa_same", os.path.join(ROOT, "tools", "isa_same.py"))
    isa_same = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(isa_same)
    asm = ("\t.text\n_Z3fooPf:\n; %bb.0:\n\ts_load_dwordx2 s[0:1], s[4:5], 0x0 ; a note\n\tv_add_f32_e32 v0, v1, v2\n\ts_endpgm\n"
           "\t.amdhsa_next_free_vgpr 3\n_Z3barPf:\n\tv_mov_b32_e32 v0, 0\n\ts_endpgm\n"
           "\t.globl __hip_cuid_0123abcd\n__hip_cuid_0123abcd:\n\t.byte 0\n")
    same = asm.replace("0123abcd", "fedc9876").replace("; a note", "; another note").replace("; %bb.0:", "; %bb.0: entry\n\n; extra")
    assert isa_same.differing(asm, same) == []
    assert isa_same.differing(asm, asm.replace("v_mov_b32_e32 v0, 0", "v_mov_b32_e32 v0, 1")) == \
        [("_Z3barPf", "v_mov_b32_e32 v0, 0", "v_mov_b32_e32 v0, 1")]
    assert [d[0] for d in isa_same.differing(asm, asm.replace(".amdhsa_next_free_vgpr 3", ".amdhsa_next_free_vgpr 4"))] == ["_Z3fooPf"]
