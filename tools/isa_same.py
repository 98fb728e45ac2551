#!/usr/bin/env python3
"""ISA identity: is the gfx950 device code of csrc/*.hip in the working tree the same text as at <git-ref>?

A refactor that only moves helpers between files must leave every kernel's assembly as it was, down to register numbers and the
.amdhsa_* resource directives (registers, LDS, scratch).  This script extracts csrc at <git-ref> with `git archive`, compiles every
.hip there and here with the Makefile's flags plus -S --cuda-device-only, drops comments, replaces the per-translation-unit
__hip_cuid_<hash> by a constant, splits the rest at the kernel labels and prints every kernel whose text differs, with the first
differing line.  It compares texts only.  Exit code 1 if any kernel differs (or a file fails to compile).  Needs no GPU.
A kernel that <git-ref> does not have is listed as added and is no difference; the module's closing metadata, which names every
kernel, is then not compared.
usage: isa_same.py <git-ref> [-DNAME[=VALUE] ...] [file.hip ...]"""
import glob, io, os, re, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "seam-match-rcnn_amd/csrc"
METADATA = "<module metadata>"


def kernels(asm):
    """{label: [lines]} of one assembly text: comments dropped, the cuid hash normalised, split at the kernel (function) labels;
    what precedes the first label and the metadata behind the last kernel are kept too, under '' and under their own labels.  A
    function's own `.section .text.<symbol>` line opens its text (it precedes the label), the module's closing sections open
    METADATA: what follows a kernel does not depend on which kernel comes next."""
    out, label = {"": []}, ""
    for l in re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", asm).splitlines():
        l = l.split(";")[0].rstrip() if '"' not in l else l.rstrip()
        if not l.strip():
            continue
        m = re.match(r"^(_Z[\w$]*|[A-Za-z][\w$]*):", l) or re.match(r"^\s*\.section\s+\.text\.([\w$]+),", l)
        if m:
            label = m.group(1)
        elif re.match(r"^\s*(\.section\s+\.AMDGPU\.|\.amdgpu_metadata)", l):
            label = METADATA
        out.setdefault(label, []).append(l)
    return out


def differing(a, b):
    """[(label, first differing line of a, of b)] for two assembly texts; empty when they are the same device code."""
    ka, kb = kernels(a), kernels(b)
    res = []
    for k in sorted(set(ka) | set(kb)):
        la, lb = ka.get(k, []), kb.get(k, [])
        if la != lb:
            i = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), min(len(la), len(lb)))
            res.append((k or "<file scope>", la[i].strip() if i < len(la) else "<absent>", lb[i].strip() if i < len(lb) else "<absent>"))
    return res


def compile_asm(job):
    src_dir, f, defs = job
    return subprocess.run(["hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", f"-I{ROOT}/include", f"-I{src_dir}", *defs,
                           "-S", "--cuda-device-only", os.path.join(src_dir, f), "-o", "-"], capture_output=True, text=True)


def main(argv):
    ref = argv[0]
    defs = [a for a in argv[1:] if a.startswith("-")]
    files = [os.path.basename(a) for a in argv[1:] if not a.startswith("-")]
    here = os.path.join(ROOT, CSRC)
    files = files or sorted(os.path.basename(f) for f in glob.glob(os.path.join(here, "*.hip")))
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", ref, CSRC], capture_output=True, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        there = os.path.join(tmp, CSRC)
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
            asms = list(pool.map(compile_asm, [(d, f, defs) for f in files for d in (there, here)]))
    for f, old, new in zip(files, asms[0::2], asms[1::2]):
        if old.returncode or new.returncode:
            print(f"{f}: compile failed\n{(old.stderr + new.stderr)[-2000:]}")
            bad += 1
            continue
        diff = differing(old.stdout, new.stdout)
        added = [k for k, x, _ in diff if x == "<absent>" and k not in kernels(old.stdout)]
        if added:
            print(f"{f}: added, not at {ref}: {', '.join(k[:100] for k in added)}")
            diff = [d for d in diff if d[0] not in added and d[0] != METADATA]
        for k, x, y in diff:
            print(f"{f}: {k[:100]}: `{x}` -> `{y}`")
        print(f"{f}: {len(kernels(new.stdout)) - 1} labels compared, {len(diff)} differ")
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
