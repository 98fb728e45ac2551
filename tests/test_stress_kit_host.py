"""``stress_kit.py`` on the CPU: the kit catches what it exists to catch, each shown by one deliberate edit of a CPU buffer; the
parent's side reads canned child output; the five ``stress_child_*.py`` import without a GPU and declare the families their test
files ask for."""
import ast
import importlib
import os
import sys

import pytest
import torch

import stress_kit as K

HERE = os.path.dirname(os.path.abspath(__file__))
DTYPES = [torch.float32, torch.float16, torch.int64, torch.int32, torch.int8, torch.uint8]
F32, F16, I32 = torch.float32, torch.float16, torch.int32


def buf(shape, dtype, which):
    return K.Buf(shape, dtype, which, device="cpu")


@pytest.fixture
def fails():
    K.fails.clear()
    yield K.fails
    K.fails.clear()


# ------------------------------------------------------------------------------------------------ Buf
@pytest.mark.parametrize("which", [None, 0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_fresh_buf_is_poisoned_guarded_and_aligned(dtype, which):
    b = buf((3, 5), dtype, which)                                       # 15 elements: no whole number of words for 1- and 2-byte types
    assert b.t.shape == (3, 5) and b.t.dtype == dtype and b.t.data_ptr() % 16 == 0
    assert b.before.numel() >= 1 << 16 and b.behind.numel() >= 1 << 20
    assert b.behind.data_ptr() == b.t.data_ptr() + 15 * b.t.element_size()      # the guard starts at the byte behind the body
    assert b.guard_ok() and b.untouched() and not b.filled()
    if which is None and b.t.element_size() == 4:
        assert bool((b.t.view(I32) == 0x7FC00001).all())
    if which is not None and dtype.is_floating_point:
        assert bool(torch.isnan(b.t).all()) if which == 0 else bool((b.t == 3.0e4).all())
    if which is not None and dtype == torch.int64:
        assert int(b.t[0, 0]) == (0x5B5B5B5B5B5B5B5B, 0x3C3C3C3C3C3C3C3C)[which]


@pytest.mark.parametrize("dtype", [F32, F16, torch.int8])
def test_one_element_behind_the_body_is_caught(dtype):
    b = buf((7,), dtype, None)
    b.behind.view(dtype)[0] = 1
    assert not b.guard_ok() and b.untouched()


@pytest.mark.parametrize("dtype", [F32, F16, torch.int8])
def test_one_element_before_the_body_is_caught(dtype):
    b = buf((7,), dtype, 0)
    b.before.view(dtype)[-1] = 1
    assert not b.guard_ok() and b.untouched()


def test_the_last_guard_byte_counts():
    b = buf((4,), F32, 1)
    b.behind[-1] = 0
    assert not b.guard_ok()


@pytest.mark.parametrize("which", [None, 0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_written_mask(dtype, which):
    written = torch.zeros((4, 6), dtype=torch.bool)
    written[1, 2:5] = True
    b = buf((4, 6), dtype, which)
    b.t[1, 3] = 1                                                       # inside the mask: allowed
    assert b.untouched(written) and not b.untouched() and b.guard_ok()
    b.t[2, 3] = 1                                                       # outside it
    assert not b.untouched(written)


def test_filled_wants_every_element():
    b = buf((2, 3), F32, None)
    b.t.fill_(1.0)
    assert b.filled()
    b.t.view(I32)[1, 2] = K.POISON_WORD
    assert not b.filled()


def test_bits_tell_the_zeros_apart_and_the_same_nan_equal():
    a, b = buf((4,), F32, 0), buf((4,), F32, 0)
    assert torch.equal(a.bits(), b.bits())                              # NaN against the same NaN
    a.t.fill_(0.0)
    b.t.fill_(0.0)
    b.t[2] = -0.0
    assert torch.equal(a.t, b.t) and not torch.equal(a.bits(), b.bits())


# ------------------------------------------------------------------------------------------------ twice / refused
def writer(value=2.0, rc=0):
    def launch(bufs):
        for b in bufs:
            b.t.fill_(value)
        return rc
    return launch


def test_twice_accepts_a_clean_launch(fails):
    out = K.twice("fam", "case", [(3, 4), (5,)], writer(), dtypes=[F32, I32], device="cpu")
    assert not fails and [tuple(o.shape) for o in out] == [(3, 4), (5,)] and float(out[0][0, 0]) == 2.0


def test_twice_reports_a_return_code(fails, capsys):
    assert K.twice("fam", "case", [(3,)], writer(rc=5), device="cpu") is None
    assert fails == [("fam", "case", "rc 5")] and "FAIL fam case rc 5" in capsys.readouterr().out


def test_twice_compares_bits(fails):
    calls = []

    def launch(bufs):
        bufs[0].t.fill_(0.0)
        if calls:
            bufs[0].t[1] = -0.0                                         # the second run differs in one bit
        calls.append(1)
        return 0
    assert K.twice("fam", "zeros", [(4,)], launch, device="cpu") is None
    assert fails == [("fam", "zeros", "output 0: two launches differ")]
    fails.clear()
    nan = writer(float("nan"))
    assert K.twice("fam", "nan", [(4,)], nan, device="cpu") is not None and not fails


def test_twice_guards_and_masks(fails):
    def past(bufs):
        bufs[0].t.fill_(1.0)
        bufs[0].behind[0] = 0
        return 0
    assert K.twice("fam", "past", [(4,)], past, device="cpu") is None
    assert fails[-1][2] == "output 0 written past its end"

    def before(bufs):
        bufs[0].t.fill_(1.0)
        bufs[0].before[-1] = 0
        return 0
    assert K.twice("fam", "before", [(4,)], before, live=["ws"], device="cpu") is None
    assert fails[-1][2] == "output 0 written past its end"
    assert K.twice("fam", "dead", [(4,)], writer(), live=[False], device="cpu") is None
    assert fails[-1][2] == "output 0: must stay untouched"
    m = torch.tensor([True, True, False, False])
    assert K.twice("fam", "mask", [(4,)], writer(), live=[m], device="cpu") is None
    assert fails[-1][2] == "output 0: element outside the written region changed"
    n = len(fails)

    def masked(bufs):
        bufs[0].t[:2] = 1.0
        return 0
    assert K.twice("fam", "mask ok", [(4,)], masked, live=[m], device="cpu") is not None and len(fails) == n
    assert K.twice("fam", "ws", [(4,)], lambda bufs: 0, live=["ws"], device="cpu") is not None and len(fails) == n


def test_refused(fails, capsys):
    K.refused("fam", "bad arg", [(4,), (2,)], lambda bufs: 3, dtypes=[F32, I32], device="cpu")
    assert not fails and "START fam refuse bad arg" in capsys.readouterr().out
    K.refused("fam", "quiet", [(4,)], lambda bufs: 3, device="cpu", start=False)
    assert "START" not in capsys.readouterr().out
    K.refused("fam", "accepted", [(4,)], lambda bufs: 0, device="cpu")
    assert fails == [("fam", "accepted", "not refused")]
    fails.clear()
    K.refused("fam", "wrote", [(4,), (2,)], writer(rc=1), dtypes=[F32, I32], device="cpu")
    assert fails == [("fam", "wrote", "refused but wrote an output")]


# ------------------------------------------------------------------------------------------------ the parent's side
GOOD = """START a case 1
START a case 2
SUMMARY a cases 2 exact 1 worst 0.2500 seconds 0.1
KERNEL a failures 0
START b case 1
FAIL b case 1 output 0: two launches differ
START b case 2
SUMMARY b cases 2 exact 0 seconds 0.2
KERNEL b failures 1
START c case 1
"""


def canned(out=GOOD, rc=1, hung=False):
    return {"rc": rc, "out": out, "err": "Traceback: boom", "hung": hung}


def test_summary_fields():
    assert K.summary_fields("SUMMARY fam cases 12 grids<=8 3 worst 0.5000 seconds 1.5") == \
        {"cases": "12", "grids<=8": "3", "worst": "0.5000", "seconds": "1.5"}


def test_family_ok_on_canned_output(capsys):
    assert K.family_ok(canned(), "a", 9) == {"cases": "2", "exact": "1", "worst": "0.2500", "seconds": "0.1"}
    assert "SUMMARY a cases 2" in capsys.readouterr().out
    with pytest.raises(AssertionError, match="FAIL b case 1 output 0: two launches differ"):
        K.family_ok(canned(), "b", 9)
    with pytest.raises(AssertionError) as e:                            # the child died in c: no KERNEL line
        K.family_ok(canned(), "c", 9)
    assert "sweep of c did not run to its end (rc 1); last case started: START c case 1" in str(e.value) and "boom" in str(e.value)
    with pytest.raises(AssertionError) as e:
        K.family_ok(canned(hung=True, rc=-1), "a", 9)
    assert "did not finish in 9 s -- last case started: START c case 1" in str(e.value)
    with pytest.raises(AssertionError, match="last case started: \\(none\\)"):
        K.family_ok(canned(out="", hung=True), "a", 9)


def test_run_child_keeps_the_output_of_a_hung_child(tmp_path):
    child = "import time\nprint('START x', flush=True)\ntime.sleep(30)\n"
    r = K.run_child([sys.executable, "-c", child], 1, str(tmp_path))
    assert r["hung"] and r["rc"] == -1 and r["out"] == "START x\n"
    r = K.run_child([sys.executable, "-c", "import sys\nprint('DONE')\nsys.exit(3)"], 30, str(tmp_path))
    assert r == {"rc": 3, "out": "DONE\n", "err": "", "hung": False}


# ------------------------------------------------------------------------------------------------ the children
def asked_families(test_file):
    """the family names the tests of ``test_file`` hand to ``_family_ok`` / ``_kernel_ok``, in order"""
    tree = ast.parse(open(os.path.join(HERE, test_file)).read())
    return [c.args[1].value for c in ast.walk(tree)
            if isinstance(c, ast.Call) and getattr(c.func, "id", "") in ("_family_ok", "_kernel_ok") and isinstance(c.args[1], ast.Constant)]


@pytest.mark.parametrize("child, test_file", [("stress_child_conv", "test_gpu_stress.py"), ("stress_child_aux", "test_gpu_stress_aux.py"),
                                              ("stress_child_heads", "test_gpu_stress_heads.py"),
                                              ("stress_child_train", "test_gpu_stress_train.py"),
                                              ("stress_child_sxpc", "test_gpu_stress_sxpc.py"),
                                              ("stress_child_w24sx", "test_gpu_stress_w24sx.py")])
def test_child_imports_without_a_gpu_and_declares_the_families_asked_for(child, test_file):
    mod = importlib.import_module(child)
    names = [n for n, _ in mod.FAMILIES]
    assert len(set(names)) == len(names) and sorted(names) == sorted(asked_families(test_file))
    assert callable(mod.main) and all(callable(fn) for _, fn in mod.FAMILIES)
    assert not hasattr(mod, "lib") and not hasattr(mod, "dev")          # the GPU and the library are main()'s business
