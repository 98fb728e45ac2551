"""GPU: conv3x3_wino24sx and the fp32 F(2x4) kernels in every block layout ``choose_layout`` can give them
(csrc/seam_wino24_common.h): the fixed table of tests/w24_layout_cases.py, whose layouts tests/test_w24_layout_cases_host.py
proves on the CPU -- every HS class of ``w24_block`` as a region alone, as a main region, as a right and as a bottom strip and in
the stacked form, the two layouts of the 100 x 100 and 200 x 200 maps, partly filled edge tiles and edge blocks, G up to 7 images
per patch, a one-row and a one-column output, C = 64 / 128 / 192, K = 64 ... 256, every epilogue.

Per case, through the C ABI, with the helpers of tests/test_gpu_w24sx.py (``Out``, ``pack_sx``, ``pack_w24``, ``gates``): inputs
from ``synth.normal``, weights scaled by 1 / sqrt(9 C); the reference is ``F.conv2d`` in float64 on the CPU with the case's epilogue
in float64.  ``seam_conv3x3_wino24sx_f32`` runs twice, onto a NaN-filled and a 3e4-filled output between guard zones: finite,
bit-identical, guards intact.  ``seam_conv3x3_wino24_f32`` and ``seam_conv2d_f32`` run on the same inputs with the same epilogue.
The gates are the project's own:
  * e_new <= 3 e_w24 + 1e-7 and |y_new - y_exact| <= 2e-5 scale (tests/test_gpu_w24sx.py),
  * e_w24 <= 3e-5, the fp32 3x3 figure of tests/test_gpu_stress.py -- which makes the table a test of w24_block<1 | 2, HS, false>
    in every layout as well.
Stacked cases and their many-image siblings: every image run alone (a different layout, asserted from the query) equals the image
in the batch bit for bit.  The two production layouts at K = 256: forced n-tile splits 1, 2 and 4 give the same bytes.

The sweep runs in ONE child process (this file as a script) under a wall-clock limit.  Every case prints a ``START`` line before
its first launch; the child stops at the first non-zero return code, overwritten guard or exception, so nothing is launched after
trouble, and every case without a ``CASE`` line fails here.  Measured on the MI355X: the 48 cases take 0.8 s inside the child, the
child as a whole (process start-up and ``import torch`` included) 2.9 s, about 4 s on a cold start: WALL_MEASURED_S = 4, and
the limit WALL_S = 16 is four times that.  Measured there too: e_new / e_w24 = 0.55-1.25, e_w24 <= 3.3e-6
(profiles/w24sx_layout_sweep.txt)."""
import math
import os
import sys
import time

import pytest

import stress_kit
import w24_layout_cases as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALL_MEASURED_S = 4          # the child, cold start included
WALL_S = 4 * WALL_MEASURED_S
TOL_W24 = 3e-5               # tests/test_gpu_stress.py: fp32 3x3 kernels against float64, reductions up to 4608
FORCED = (1, 2, 4)


# ------------------------------------------------------------------------------------------------ the child: launches and checks
class Stop(Exception):
    """trouble after which nothing more is launched"""


def child_main(argv):
    sys.path.insert(0, ROOT)
    import torch
    import torch.nn.functional as F
    import seam_match_rcnn_amd.ops as ops
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd import _native
    import test_gpu_w24sx as W

    t_start = time.time()
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    lib, dev = _native.lib(), torch.device("cuda:0")
    ptr = W.ptr
    lines = []

    def say(*a):
        print(*a, flush=True)

    def record(line):
        lines.append(line)
        say(line)

    def launch_sx(c, x, u, sc, sh, res, relu, fill=None):
        """one launch onto a guarded output; a return code or a touched guard ends the sweep"""
        n, h, w, _ = x.shape
        o = W.Out((n, h + 2 * c.pad - 2, w + 2 * c.pad - 2, c.k), dev)
        if fill is not None:
            o.y.fill_(fill)
        rc = lib.seam_conv3x3_wino24sx_f32(ptr(x), ptr(u), ptr(sc), ptr(sh), ptr(res), ptr(o.y), n, h, w, c.c, c.k, c.pad, 1, relu, None)
        torch.cuda.synchronize()
        if rc != 0:
            raise Stop(f"{c.id}: seam_conv3x3_wino24sx_f32 returned {rc}")
        if not o.intact():
            raise Stop(f"{c.id}: bytes outside the output were overwritten")
        return o.y

    def run_case(i, c):
        lay = T.query(lib, c.n, c.h, c.w, c.c, c.k, c.pad)
        sig = T.signature(lay, c.n, c.h, c.w, c.pad)
        say("START", c.id, f"{c.n}x{c.h}x{c.w} {c.c}->{c.k} pad{c.pad} {c.epilogue or 'plain'}", T.describe(sig))
        if not T.meets(sig, c.expect):
            raise Stop(f"{c.id}: the library lays this case out as {T.describe(sig)}, not as {c.expect}")
        rnd = lambda name, shape: torch.from_numpy(synth.normal(synth.stream_id(1000 + i, name), shape))
        x = rnd("x", (c.n, c.c, c.h, c.w))
        wt = rnd("w", (c.k, c.c, 3, 3)) * (1.0 / math.sqrt(9 * c.c))
        ref = F.conv2d(x.double(), wt.double(), None, 1, c.pad).permute(0, 2, 3, 1).contiguous()
        sc = sh = res = None
        if c.epilogue == "scale_shift":
            sc = torch.from_numpy(synth.uniform(synth.stream_id(1000 + i, "sc"), (c.k,), 0.5, 1.5))
            sh = rnd("sh", (c.k,)) * 0.1
            ref = ref * sc.double() + sh.double()
        if "residual" in c.epilogue:
            res = rnd("res", tuple(ref.shape))
            ref = ref + res.double()
        relu = int("relu" in c.epilogue)
        if relu:
            ref = F.relu(ref)
        xd, wd = W.nhwc(x).to(dev), wt.to(dev)
        scd, shd, resd = (None if t is None else t.to(dev) for t in (sc, sh, res))
        u = W.pack_sx(lib, wd, dev)
        y = launch_sx(c, xd, u, scd, shd, resd, relu)
        y2 = launch_sx(c, xd, u, scd, shd, resd, relu, fill=3.0e4)
        y24 = torch.full(tuple(ref.shape), float("nan"), dtype=torch.float32, device=dev)
        yex = torch.full_like(y24, float("nan"))
        rc = lib.seam_conv3x3_wino24_f32(ptr(xd), ptr(W.pack_w24(lib, wd, dev)), ptr(scd), ptr(shd), ptr(resd), ptr(y24), c.n, c.h, c.w, c.c,
                                         c.k, c.pad, relu, None)
        if rc != 0:
            raise Stop(f"{c.id}: seam_conv3x3_wino24_f32 returned {rc}")
        pc = ops.pack_conv(wd, None, stride=1, pad=c.pad)
        rc = lib.seam_conv2d_f32(ptr(xd), ptr(pc.w), ptr(scd), ptr(shd), ptr(resd), ptr(yex), c.n, c.h, c.w, c.c, c.k, 3, 3, 1, c.pad, relu, None)
        torch.cuda.synchronize()
        if rc != 0:
            raise Stop(f"{c.id}: seam_conv2d_f32 returned {rc}")
        why = []
        if not (bool(torch.isfinite(y).all()) and bool(torch.isfinite(y2).all())):
            why.append("poison or non-finite values left in the output")
        if not torch.equal(y.view(torch.int32), y2.view(torch.int32)):
            why.append("two launches differ")
        yc, y24c, yexc = y.cpu(), y24.cpu(), yex.cpu()
        scale = float(ref.abs().max())
        e_new = float((yc.double() - ref).abs().max()) / scale
        e_w24 = float((y24c.double() - ref).abs().max()) / scale
        d_ex = float((yc - yexc).abs().max()) / scale
        try:
            W.gates(c.id, yc, ref, y24c, yexc)
        except AssertionError as e:
            why.append(str(e))
        if not e_w24 <= TOL_W24:
            why.append(f"e_w24 {e_w24:.3e} > {TOL_W24:.0e}")
        # stacked: every image alone (another layout) is the image in the batch, bit for bit
        if sig["stack"]:
            alone = T.query(lib, 1, c.h, c.w, c.c, c.k, c.pad)
            if (alone["stack"], alone["TX"], alone["TY"]) == (lay["stack"], lay["TX"], lay["TY"]):
                why.append("one image alone has the layout of the batch: the comparison proves nothing")
            for j in range(c.n):
                rj = None if resd is None else resd[j:j + 1].contiguous()
                yj = launch_sx(c, xd[j:j + 1].contiguous(), u, scd, shd, rj, relu)
                if not torch.equal(yj[0].view(torch.int32), y[j].view(torch.int32)):
                    why.append(f"image {j} alone differs from image {j} in the batch")
        # the production layouts at K = 256: the n-tile split over XCD groups only renumbers the blocks
        if c.role == "nsplit":
            before = lib.seam_conv3x3_wino24sx_get_nsplit()
            try:
                for ns in FORCED:
                    if lib.seam_conv3x3_wino24sx_set_nsplit(ns) != 0:
                        raise Stop(f"{c.id}: set_nsplit({ns}) refused")
                    got = T.query(lib, c.n, c.h, c.w, c.c, c.k, c.pad)["nsplit"]
                    if got != ns:
                        why.append(f"forced split {ns} runs as {got}")
                    yn = launch_sx(c, xd, u, scd, shd, resd, relu)
                    if not torch.equal(yn.view(torch.int32), y.view(torch.int32)):
                        why.append(f"nsplit {ns} differs from the rule's output")
            finally:
                lib.seam_conv3x3_wino24sx_set_nsplit(before)
        record(f"CASE {c.id} {'FAIL' if why else 'OK'} | {c.n}x{c.h}x{c.w} {c.c}->{c.k} pad{c.pad} {c.epilogue or 'plain'} | {T.describe(sig)} | "
               f"e_new {e_new:.3e} e_w24 {e_w24:.3e} ratio {e_new / max(e_w24, 1e-30):.2f} |new-exact|/scale {d_ex:.3e}"
               + "".join(f" | {w_}" for w_ in why))
        return e_new / max(e_w24, 1e-30)

    rc, ratios = 0, []
    try:
        for i, c in enumerate(T.CASES):
            ratios.append(run_case(i, c))
    except Stop as e:
        say("STOP", e)
        rc = 2
    except Exception as e:          # a HIP error surfaces as a RuntimeError of torch: nothing more is launched
        say("STOP", type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        rc = 3
    if ratios:
        record(f"RATIO min {min(ratios):.2f} max {max(ratios):.2f} over {len(ratios)} cases")
    record(f"WALL seconds {time.time() - t_start:.1f}")
    say("DONE cases", len(ratios), "of", len(T.CASES))
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc or (1 if any(" FAIL " in ln for ln in lines) else 0)


# ------------------------------------------------------------------------------------------------ the tests: read the child's output
@pytest.fixture(scope="module")
def sweep():
    t0 = time.time()
    res = stress_kit.run_child([sys.executable, os.path.abspath(__file__)], WALL_S, ROOT)
    res["wall"] = time.time() - t0
    print(f"\nw24sx layout sweep: {res['wall']:.1f} s of wall time (limit {WALL_S} s)")
    return res


def _last_start(sweep):
    starts = [ln for ln in sweep["out"].splitlines() if ln.startswith("START")]
    return starts[-1] if starts else "(none)"


@pytest.mark.parametrize("cid", [c.id for c in T.CASES])
def test_layout_case(sweep, cid):
    if sweep["hung"]:
        pytest.fail(f"the sweep did not finish in {WALL_S} s -- last case started: {_last_start(sweep)}")
    line = [ln for ln in sweep["out"].splitlines() if ln.startswith(f"CASE {cid} ")]
    stop = [ln for ln in sweep["out"].splitlines() if ln.startswith("STOP")]
    assert len(line) == 1, f"no result for {cid} (child rc {sweep['rc']}); {stop[0] if stop else ''} last case started: {_last_start(sweep)}\n" \
                           + sweep["out"][-1500:] + sweep["err"][-3000:]
    print(line[0])
    assert line[0].split()[2] == "OK", line[0]


def test_sweep_ran_to_its_end_within_its_time(sweep):
    out = sweep["out"].splitlines()
    assert not sweep["hung"] and sweep["rc"] == 0, (sweep["rc"], [ln for ln in out if ln.startswith(("STOP", "CASE")) and " OK " not in ln][:5],
                                                    sweep["err"][-2000:])
    assert f"DONE cases {len(T.CASES)} of {len(T.CASES)}" in out
    print([ln for ln in out if ln.startswith(("RATIO", "WALL"))], f"parent wall {sweep['wall']:.1f} s")
    assert sweep["wall"] <= WALL_S


if __name__ == "__main__":
    sys.exit(child_main(sys.argv[1:]))
