"""The harness the stress sweeps share (``test_gpu_stress*.py``, ``stress_child_*.py``, ``test_gpu_w24sx_layouts.py``), held once
and checked on the CPU by ``test_stress_kit_host.py``.  The library, the references and each family's ``check`` stay with the sweeps.

In the process that launches kernels: ``Buf`` (a poisoned output or workspace between two guard regions), ``twice`` (two launches
onto differently poisoned outputs must agree bit for bit), ``refused`` (a non-zero return that left every output alone), ``say`` /
``fail`` / ``fails`` and the ``P`` / ``st`` argument helpers.  In the test that reads a child's output: ``run_child``,
``summary_fields`` and ``family_ok``.

A child prints ``START <family> <case>`` before every launch, ``FAIL <family> <case> <why>`` per failure, one ``SUMMARY <family>
<key> <value> ...`` line and one ``KERNEL <family> failures <n>`` line per family.
"""
import subprocess

import torch

GUARD_BEFORE = 1 << 16          # bytes; a multiple of 16, so the body keeps the allocation's alignment (the kernels store 16-byte vectors)
GUARD_BEHIND = 1 << 20          # bytes
GUARD_BYTE = 0x5A
POISON_WORD = 0x7FC00001        # which=None: every 32-bit word of the body; a NaN in fp32, a large value in the integer outputs
POISON_FLOAT = (float("nan"), 3.0e4)                                   # which=0 / 1, fp16 included
POISON_INT = (0x5B5B5B5B5B5B5B5B, 0x3C3C3C3C3C3C3C3C)                  # which=0 / 1, cut to the integer type's width
_BITS = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}

fails = []


def say(*a):
    print(*a, flush=True)


def fail(name, desc, why):
    fails.append((name, desc, why))
    say("FAIL", name, desc, why)


def P(t):
    return None if t is None else t.data_ptr()


def st():
    return torch.cuda.current_stream().cuda_stream


def _word_pattern(shape, dtype, device):
    """POISON_WORD repeated over the bytes of a tensor of ``shape`` and ``dtype`` (cut where they are no whole number of words)"""
    nbytes = torch.Size(shape).numel() * torch.empty((), dtype=dtype).element_size()
    words = torch.full(((nbytes + 3) // 4,), POISON_WORD, dtype=torch.int32, device=device)
    return words.view(torch.uint8)[:nbytes].view(dtype).view(shape)


class Buf:
    """An output / workspace ``t`` of ``shape`` and ``dtype``, poisoned, with GUARD_BEFORE bytes before it and GUARD_BEHIND bytes
    directly behind its last element.  which=None: the word pattern POISON_WORD; which=0 / 1: the two-run poison (NaN then 3e4
    for floating types, POISON_INT for integer types)."""

    def __init__(self, shape, dtype=torch.float32, which=None, device="cuda:0"):
        n = torch.Size(shape).numel()
        es = torch.empty((), dtype=dtype).element_size()
        lo, hi = GUARD_BEFORE, GUARD_BEFORE + n * es
        self.raw = torch.full((hi + GUARD_BEHIND,), GUARD_BYTE, dtype=torch.uint8, device=device)
        self.before, self.behind = self.raw[:lo], self.raw[hi:]
        self.t = self.raw[lo:hi].view(dtype).view(shape)
        self.which = which
        if which is None:
            self.t.copy_(_word_pattern(shape, dtype, device))
        else:
            value = POISON_FLOAT[which] if dtype.is_floating_point else POISON_INT[which] & ((1 << (8 * es)) - 1)
            self.poison = torch.tensor(value, dtype=dtype, device=device)          # as the type holds it: 3e4 is 29952 in fp16
            self.t.copy_(self.poison)

    def guard_ok(self):
        return bool((self.before == GUARD_BYTE).all()) and bool((self.behind == GUARD_BYTE).all())

    def bits(self):
        """``t`` as integers of its element size: what two launches must agree on"""
        return self.t.view(_BITS[self.t.element_size()])

    def _keeps(self):
        """bool, shaped like ``t``: the element still holds its poison"""
        if self.which is None:
            return self.bits() == _word_pattern(self.t.shape, self.t.dtype, self.t.device).view(self.bits().dtype)
        return torch.isnan(self.t) if self.which == 0 and self.t.dtype.is_floating_point else self.t == self.poison

    def untouched(self, written=None):
        """``written`` (a bool mask shaped like ``t``; None: nothing) marks the elements the launch may write: every other
        element still holds its poison."""
        keeps = self._keeps()
        return bool((keeps if written is None else keeps | written).all())

    def filled(self):
        """no element still holds the poison: the launch wrote all of ``t``"""
        return not bool(self._keeps().any())


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def twice(name, desc, shapes, launch, live=None, dtypes=None, device="cuda:0"):
    """launch(bufs) -> rc on two sets of poisoned outputs; all rc 0, guards intact, and the outputs bit-identical.
    live[i]: True / None all of output i, False none of it (it must keep its poison), a bool mask the elements written (the
    others must keep their poison), "ws" a workspace (guards only).  -> list of outputs of run 0."""
    runs = []
    for which in (0, 1):
        bufs = [Buf(s, torch.float32 if dtypes is None else dtypes[i], which, device) for i, s in enumerate(shapes)]
        rc = launch(bufs)
        if rc != 0:
            fail(name, desc, f"rc {rc}")
            return None
        runs.append(bufs)
    _sync(device)
    for i in range(len(shapes)):
        a, b = runs[0][i], runs[1][i]
        if not (a.guard_ok() and b.guard_ok()):
            fail(name, desc, f"output {i} written past its end")
            return None
        m = None if live is None else live[i]
        if isinstance(m, str):
            continue
        if m is False:
            if not (a.untouched() and b.untouched()):
                fail(name, desc, f"output {i}: must stay untouched")
                return None
        elif m is not None and m is not True:
            if not (a.untouched(m) and b.untouched(m)):
                fail(name, desc, f"output {i}: element outside the written region changed")
                return None
            if not torch.equal(a.bits()[m], b.bits()[m]):
                fail(name, desc, f"output {i}: two launches differ")
                return None
        elif not torch.equal(a.bits(), b.bits()):
            fail(name, desc, f"output {i}: two launches differ")
            return None
    return [b.t for b in runs[0]]


def refused(name, desc, shapes, launch, dtypes=None, device="cuda:0", start=True):
    """A launch that must return non-zero and leave every (poisoned) output untouched."""
    if start:
        say("START", name, "refuse", desc)
    bufs = [Buf(s, torch.float32 if dtypes is None else dtypes[i], 1, device) for i, s in enumerate(shapes)]
    rc = launch(bufs)
    _sync(device)
    if rc == 0:
        fail(name, desc, "not refused")
    elif not all(b.untouched() and b.guard_ok() for b in bufs):
        fail(name, desc, "refused but wrote an output")


# ------------------------------------------------------------------------------------------------ the parent's side
def run_child(argv, wall_s, cwd):
    """Start the child once, under a wall-clock limit -> {"rc", "out", "err", "hung"}; a child killed at the limit keeps what it
    printed.  Nothing is retried and nothing is started after it."""
    try:
        r = subprocess.run(argv, cwd=cwd, capture_output=True, text=True, timeout=wall_s)
        return {"rc": r.returncode, "out": r.stdout, "err": r.stderr, "hung": False}
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
        err = e.stderr.decode() if isinstance(e.stderr, bytes) else (e.stderr or "")
        return {"rc": -1, "out": out, "err": err, "hung": True}


def summary_fields(line):
    """"SUMMARY <family> k1 v1 k2 v2 ..." -> {k1: v1, k2: v2, ...}"""
    t = line.split()
    return dict(zip(t[2::2], t[3::2]))


def family_ok(sweep, name, wall_s):
    """The family ran to its end without a failure -> the fields of its SUMMARY line."""
    lines = sweep["out"].splitlines()
    starts = [ln for ln in lines if ln.startswith("START")]
    last = starts[-1] if starts else "(none)"
    assert not sweep["hung"], f"the sweep did not finish in {wall_s} s -- last case started: {last}"
    line = [ln for ln in lines if ln.startswith(f"KERNEL {name} ")]
    assert line, f"sweep of {name} did not run to its end (rc {sweep['rc']}); last case started: {last}\n" \
                 + sweep["out"][-1500:] + sweep["err"][-3000:]
    failed = [ln for ln in lines if ln.startswith("FAIL") and f" {name} " in ln]
    assert line[0].split()[-1] == "0", "\n".join(failed[:20])
    summary = [ln for ln in lines if ln.startswith(f"SUMMARY {name} ")]
    assert summary, sweep["out"][-1500:]
    print(summary[0])
    return summary_fields(summary[0])
