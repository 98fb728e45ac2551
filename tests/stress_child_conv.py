"""The child of ``test_gpu_stress.py``: ``python stress_child_conv.py NCASE SEED [kernel ...]`` runs the sweep on the GPU and prints
the lines ``stress_kit.family_ok`` reads.  Importing it launches nothing."""
import math, os, random, sys, time
import torch
import torch.nn.functional as F
from stress_kit import Buf, P, fails, say, st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMES = [3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37, 41, 43, 47, 53, 59, 61, 67, 71, 73, 79, 83, 89, 97, 101, 103, 107, 109, 113, 127,
          131, 137, 139, 149, 151, 157, 163, 167, 173, 179, 181, 191, 193, 197, 199]


def gen(rng):
    g = torch.Generator(device=dev)
    g.manual_seed(rng.randrange(1 << 30))
    return g


def dim(rng, lo=3, hi=210):
    r = rng.random()
    if r < 0.3:
        return rng.choice([p for p in PRIMES if lo <= p <= hi])
    if r < 0.5:
        return rng.choice([v for v in (6, 8, 10, 12, 14, 16, 25, 50, 100, 200, 210) if lo <= v <= hi])
    return rng.randint(lo, hi)


def pick_n(rng, per_img, budget):
    nmax = max(1, min(3000, budget // max(per_img, 1)))
    r = rng.random()
    if r < 0.25:
        return rng.randint(1, min(3, nmax))
    if r < 0.35:
        return nmax
    return rng.randint(1, nmax)


def epilogue_vectors(rng, k, g):
    mode = rng.choice(["none", "bias", "bn"])
    scale = shift = None
    if mode == "bias":
        shift = torch.randn(k, device=dev, generator=g) * 0.2
    elif mode == "bn":
        scale = torch.rand(k, device=dev, generator=g) + 0.5
        shift = torch.randn(k, device=dev, generator=g) * 0.2
    return scale, shift


def torch_epilogue(acc, scale, shift, res, relu):
    y = acc
    if scale is not None:
        y = y * scale
    if shift is not None:
        y = y + shift
    if relu == 2:
        return torch.where(res > 0, y, torch.zeros_like(y))
    if res is not None:
        y = y + res
    return F.relu(y) if relu == 1 else y


def torch_conv3x3(x, wt, pad):
    """fp32 3x3 / stride-1 convolution of an NHWC tensor as nine tap-wise matmuls (plain torch, no per-shape algorithm search)."""
    n, h, w, c = x.shape
    k = wt.shape[0]
    xp = F.pad(x, (0, 0, pad, pad, pad, pad)) if pad else x
    ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
    acc = torch.zeros((n * ho * wo, k), dtype=torch.float32, device=x.device)
    for r in range(3):
        for s in range(3):
            acc += xp[:, r:r + ho, s:s + wo, :].reshape(-1, c).float() @ wt[:, :, r, s].float().t()
    return acc.view(n, ho, wo, k)


def check(name, desc, got, got2, refs, tol):
    ok = True
    why = ""
    if not guards_intact():
        ok, why = False, "bytes BEHIND the output tensor were overwritten"
    elif not torch.equal(got, got2):
        ok, why = False, "two launches differ"
    elif not bool(torch.isfinite(got.float()).all()):
        ok, why = False, "poison / non-finite values left in the output"
    else:
        for rname, ref in refs:
            sc = max(float(ref.float().abs().max()), 1e-20)
            err = float((got.float() - ref.float()).abs().max()) / sc
            if not err <= tol:
                ok, why = False, f"{err:.2e} of scale from {rname}"
                break
    if not ok:
        fails.append((name, desc, why))
        say("FAIL", name, desc, why)
    return ok


_bufs = []


def poisoned(shape, dtype, which):
    """A poisoned output between guards (``stress_kit.Buf``) that guards_intact() checks: a kernel that computes a ragged last
    tile's addresses wrongly (or trusts a range check that does not cover them) writes past the tensor."""
    _bufs.append(Buf(shape, dtype, which))
    return _bufs[-1].t


def guards_intact():
    ok = all(b.guard_ok() for b in _bufs)
    _bufs.clear()
    return ok


# ------------------------------------------------------------------------------------------------ conv3x3_wino24pc
def stress_wino24pc(rng):
    t0 = time.time()
    done = conv_checked = 0
    small = xcd1 = mid = 0
    while done < NCASE:
        c = rng.choice([64, 64, 128, 192, 256, 256, 320, 512])
        k = rng.choice([64, 128, 192, 256, 512])
        pad = rng.randint(0, 1)
        big = rng.random() < 0.08
        r = rng.random()
        if r < 0.35:            # ROI-sized / stacked maps
            h = rng.choice([3, 4, 5, 6, 7, 8, 10, 12, 13, 14, 16, 17, 20, 25])
            w = h if rng.random() < 0.6 else rng.choice([3, 5, 6, 8, 10, 12, 14, 16, 19, 25, 31])
        else:
            h, w = dim(rng), dim(rng)
        if h + 2 * pad < 3 or w + 2 * pad < 3:
            continue
        budget = (24 if big else 3) << 20
        n = pick_n(rng, h * w * max(c, k), budget)
        forced = rng.random() < 0.55
        _native.set_option("SEAM_W24_NT", 2 if forced else 0)
        if lib.seam_wino24_form(n, h, w, c, k, pad) != 1:
            if forced:
                continue
            # natural dispatch: grow the batch until the launcher picks the producer / consumer kernel (it wants >= 1024 blocks)
            n2 = n
            while n2 * h * w * max(c, k) < (48 << 20) and lib.seam_wino24_form(n2, h, w, c, k, pad) != 1:
                n2 = n2 * 2 + 1
            if n2 > 3000 or lib.seam_wino24_form(n2, h, w, c, k, pad) != 1:
                continue
            n = n2
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1, 1])
        res_mode = rng.choice([0, 0, 1, 2])
        ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
        slots = int(lib.seam_wino24_issue_slots(n, h, w, c, k, pad)) // (2 * 32 * 24)       # tiles of the launch
        small += slots < 256
        xcd1 += slots <= 8
        mid += (slots % 8) != 0
        desc = f"n={n} {h}x{w} c={c} k={k} pad={pad} relu={relu} res={res_mode} forced_nt2={int(forced)} tiles={slots}"
        say("START wino24pc", desc)
        x = torch.randn(n, h, w, c, device=dev, generator=g)
        wt = torch.randn(k, c, 3, 3, device=dev, generator=g) / math.sqrt(9 * c)
        scale, shift = epilogue_vectors(rng, k, g)
        res = torch.randn(n, ho, wo, k, device=dev, generator=g) if res_mode else None
        mode = 2 if res_mode == 2 else relu
        pc = ops.pack_conv(wt, None, None, stride=1, pad=pad)
        outs = []
        for rep in range(2):
            y = poisoned((n, ho, wo, k), torch.float32, rep)
            rc = lib.seam_conv3x3_wino24_f32(P(x), P(pc.u24), P(scale), P(shift), P(res), P(y), n, h, w, c, k, pad, mode, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        yi = poisoned((n, ho, wo, k), torch.float32, 0)
        rc = lib.seam_conv2d_f32(P(x), P(pc.w), P(scale), P(shift), P(res), P(yi), n, h, w, c, k, 3, 3, 1, pad, mode, st())
        assert rc == 0, (desc, rc)
        refs = [("implicit GEMM", yi), ("torch fp32 (tap-wise matmul)", torch_epilogue(torch_conv3x3(x, wt, pad), scale, shift, res, mode))]
        if conv_checked < 10 and n * h * w * c < (2 << 20):
            conv_checked += 1
            refs.append(("torch F.conv2d", torch_epilogue(F.conv2d(x.permute(0, 3, 1, 2), wt, None, 1, pad).permute(0, 2, 3, 1), scale, shift, res, mode)))
        check("wino24pc", desc, outs[0], outs[1], refs, 3e-5)
    _native.set_option("SEAM_W24_NT", 0)
    # unserved channel counts: refused, not launched (pointers are never dereferenced)
    dummy = torch.zeros(1 << 16, device=dev)
    for (c, k) in [(60, 64), (64, 48), (4, 64), (64, 16), (0, 64)]:
        rc = lib.seam_conv3x3_wino24_f32(P(dummy), P(dummy), None, None, None, P(dummy), 1, 8, 8, c, k, 1, 0, st())
        if rc == 0:
            fails.append(("wino24pc", f"c={c} k={k}", "unserved channel count was not refused"))
    # the launcher caps.  An image of >= 2^31 bytes: refused ...
    rc = lib.seam_conv3x3_wino24_f32(P(dummy), P(dummy), None, None, None, P(dummy), 1, 210, 210, 12224, 64, 1, 0, st())
    if rc == 0:
        fails.append(("wino24pc", "210x210x12224", "an image of >= 2^31 bytes was not refused"))
    # ... more than 2^24 blocks: refused ...
    rc = lib.seam_conv3x3_wino24_f32(P(dummy), P(dummy), None, None, None, P(dummy), 3000, 210, 210, 64, 2048, 1, 0, st())
    if rc == 0:
        fails.append(("wino24pc", "3000x210x210 k=2048", ">= 2^24 blocks were not refused"))
    # ... and the largest image under the byte cap runs (24-bit multiplies at their largest operands): 210 x 210 x 12160 x 4 B = 2^31 - 2.4 MB
    _native.set_option("SEAM_W24_NT", 2)
    n, h, w, c, k, pad = 1, 210, 210, 12160, 64, 1
    if lib.seam_wino24_form(n, h, w, c, k, pad) == 1:
        desc = f"n={n} {h}x{w} c={c} k={k} pad={pad} (just under the 2^31-byte cap)"
        say("START wino24pc", desc)
        g = gen(rng)
        x = torch.randn(n, h, w, c, device=dev, generator=g)
        wt = torch.randn(k, c, 3, 3, device=dev, generator=g) / math.sqrt(9 * c)
        pc = ops.pack_conv(wt, None, None, stride=1, pad=pad)
        outs = []
        for rep in range(2):
            y = poisoned((n, h, w, k), torch.float32, rep)
            rc = lib.seam_conv3x3_wino24_f32(P(x), P(pc.u24), None, None, None, P(y), n, h, w, c, k, pad, 0, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        check("wino24pc", desc, outs[0], outs[1], [("torch fp32 (tap-wise matmul)", torch_conv3x3(x, wt, pad))], 3e-5)
        del x, wt, pc, outs
    else:
        fails.append(("wino24pc", "210x210x12160", "the largest image under the cap is not served"))
    _native.set_option("SEAM_W24_NT", 0)
    say(f"SUMMARY wino24pc cases {done} grids<256 {small} grids<=8 {xcd1} ragged-XCD-ranges {mid} F.conv2d-checked {conv_checked} "
        f"seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ conv1x1_pc
def stress_pwpc(rng):
    t0 = time.time()
    done = exact = conv_checked = 0
    while done < NCASE:
        c = rng.choice([256, 384, 512, 640, 768, 1024, 1536, 2048])
        k = rng.choice([128, 256, 384, 512, 1024, 2048])
        h, w = dim(rng, 1, 120), dim(rng, 1, 120)
        n = pick_n(rng, h * w * max(c, k), 3 << 20)
        m = n * h * w
        if lib.seam_conv1x1_pc_supported(m, c, k) != 1:
            continue
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1])
        use_res = rng.random() < 0.4
        desc = f"M={m} c={c} k={k} relu={relu} res={int(use_res)}"
        say("START conv1x1_pc", desc)
        x = torch.randn(m, c, device=dev, generator=g)
        wt = torch.randn(k, c, device=dev, generator=g) / math.sqrt(c)
        scale, shift = epilogue_vectors(rng, k, g)
        res = torch.randn(m, k, device=dev, generator=g) if use_res else None
        wq = torch.empty((int(lib.seam_conv1x1_pc_weight_floats(k, c)),), dtype=torch.float32, device=dev)
        assert lib.seam_pack_conv1x1_pc_f32(P(wt), P(wq), k, c, st()) == 0
        wi = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred(c, 1, 1)), dtype=torch.float32, device=dev)
        assert lib.seam_pack_conv_weight_f32(P(wt), P(wi), k, c, 1, 1, c, 0, st()) == 0
        outs = []
        for rep in range(2):
            y = poisoned((m, k), torch.float32, rep)
            rc = lib.seam_conv1x1_pc_f32(P(x), P(wq), P(scale), P(shift), P(res), P(y), m, c, k, relu, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        yi = poisoned((m, k), torch.float32, 0)
        assert lib.seam_conv2d_f32(P(x), P(wi), P(scale), P(shift), P(res), P(yi), 1, 1, m, c, k, 1, 1, 1, 0, relu, st()) == 0
        exact += bool(torch.equal(outs[0], yi))
        refs = [("implicit GEMM", yi), ("torch fp32 matmul", torch_epilogue(x @ wt.t(), scale, shift, res, relu))]
        if conv_checked < 10:
            conv_checked += 1
            refs.append(("torch F.conv2d", torch_epilogue(F.conv2d(x.t().reshape(1, c, m, 1), wt[:, :, None, None])[0, :, :, 0].t(), scale, shift, res, relu)))
        check("conv1x1_pc", desc, outs[0], outs[1], refs, 2e-5)
    dummy = torch.zeros(1 << 16, device=dev)
    for (c, k) in [(320, 128), (128, 128), (256, 192), (512, 64)]:
        if lib.seam_conv1x1_pc_f32(P(dummy), P(dummy), None, None, None, P(dummy), 64, c, k, 0, st()) == 0:
            fails.append(("conv1x1_pc", f"c={c} k={k}", "unserved channel count was not refused"))
    say(f"SUMMARY conv1x1_pc cases {done} bit-identical-to-implicit-GEMM {exact} seconds {time.time() - t0:.1f}")
    if exact != done:
        fails.append(("conv1x1_pc", "-", f"only {exact} of {done} results bit-identical to the implicit GEMM (same k order claimed)"))


# ------------------------------------------------------------------------------------------------ conv3x3_f16pc
def stress_f16pc(rng):
    t0 = time.time()
    done = conv_checked = 0
    while done < NCASE:
        if rng.random() < 0.5:
            h, w = dim(rng, 3, 120), dim(rng, 26, 210)
        else:
            w = rng.choice([3, 4, 6, 8, 10, 12, 13, 14, 16, 17, 18])
            h = w if rng.random() < 0.7 else rng.choice([3, 5, 6, 8, 10, 12, 14, 16, 18])
        pad = rng.randint(0, 1)
        c, k = rng.choice([128, 256, 384, 512]), rng.choice([128, 256, 384, 1024])
        if w >= 26 and rng.random() < 0.3:
            c = k = 64                      # conv3x3_f16pc64 (round 6): one chunk per tile, weights in registers, 16 x 16 tiles
        if h + 2 * pad < 3 or w + 2 * pad < 3:
            continue
        n = pick_n(rng, h * w * max(c, k), 4 << 20)
        if lib.seam_conv3x3_f16pc_supported(n, h, w, c, k, pad) != 1:
            continue
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1, 1])
        ho, wo = h + 2 * pad - 2, w + 2 * pad - 2
        desc = f"n={n} {h}x{w} c={c} k={k} pad={pad} relu={relu}"
        say("START f16pc", desc)
        x = torch.randn(n, h, w, c, device=dev, generator=g).half()
        wt = (torch.randn(k, c, 3, 3, device=dev, generator=g) / math.sqrt(9 * c)).half().float()
        scale, shift = epilogue_vectors(rng, k, g)
        wh = torch.empty((int(lib.seam_f16pc_weight_halves(k, c)),), dtype=torch.float16, device=dev)
        assert lib.seam_pack_conv_weight_f16pc(P(wt), P(wh), k, c, c, st()) == 0
        wi = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred_f16(c, 3, 3)), dtype=torch.float16, device=dev)
        assert lib.seam_pack_conv_weight_f16(P(wt), P(wi), k, c, 3, 3, c, 0, st()) == 0
        outs = []
        for rep in range(2):
            y = poisoned((n, ho, wo, k), torch.float16, rep)
            rc = lib.seam_conv3x3_f16pc(P(x), P(wh), P(scale), P(shift), None, P(y), n, h, w, c, k, pad, relu, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        yi = poisoned((n, ho, wo, k), torch.float16, 0)
        assert lib.seam_conv2d_f16(P(x), P(wi), P(scale), P(shift), None, P(yi), n, h, w, c, k, 3, 3, 1, pad, relu, 0, st()) == 0
        refs = [("implicit GEMM (fp16)", yi), ("torch fp32 (tap-wise matmul)", torch_epilogue(torch_conv3x3(x, wt, pad), scale, shift, None, relu))]
        if conv_checked < 10 and n * h * w * c < (2 << 20):
            conv_checked += 1
            refs.append(("torch F.conv2d", torch_epilogue(F.conv2d(x.float().permute(0, 3, 1, 2), wt, None, 1, pad).permute(0, 2, 3, 1), scale, shift, None, relu)))
        check("f16pc", desc, outs[0], outs[1], refs, 2e-3)
    dummy = torch.zeros(1 << 16, device=dev)
    for (c, k) in [(64, 128), (128, 64), (192, 128), (136, 128), (64, 64)]:       # (64 -> 64 is served on large maps only)
        if lib.seam_conv3x3_f16pc(P(dummy), P(dummy), None, None, None, P(dummy), 2, 14, 14, c, k, 1, 1, st()) == 0:
            fails.append(("f16pc", f"c={c} k={k}", "unserved channel count was not refused"))
    if lib.seam_conv3x3_f16pc(P(dummy), P(dummy), None, None, P(dummy), P(dummy), 2, 14, 14, 128, 128, 1, 1, st()) == 0:
        fails.append(("f16pc", "residual", "a residual operand was not refused"))
    say(f"SUMMARY f16pc cases {done} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ conv1x1_sw
def stress_sw(rng):
    t0 = time.time()
    done = conv_checked = 0
    while done < NCASE:
        c = rng.choice([32, 64, 96, 128, 160, 192, 224, 256])
        k = rng.choice([64, 128, 192, 256, 512, 1024, 2048])
        h, w = dim(rng, 1, 150), dim(rng, 1, 150)
        n = pick_n(rng, h * w * max(c, k), 3 << 20)
        m = n * h * w
        dual = c % 64 == 0 and rng.random() < 0.25
        c1, c2 = (c // 2, c // 2) if dual else (c, 0)
        if lib.seam_conv1x1_sw_config(m, c1, c2, k) == 0:
            continue
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1])
        res_mode = 0 if dual else rng.choice([0, 0, 1, 2])
        desc = f"n={n} {h}x{w} c={c1}+{c2} k={k} relu={relu} res_mode={res_mode} cfg={lib.seam_conv1x1_sw_config(m, c1, c2, k)}"
        say("START conv1x1_sw", desc)
        x = torch.randn(n, h, w, c, device=dev, generator=g)
        wt = torch.randn(k, c, device=dev, generator=g) / math.sqrt(c)
        shift = torch.randn(k, device=dev, generator=g) * 0.2
        rh, rw = (h + 1) // 2, (w + 1) // 2
        res = None
        if res_mode == 1:
            res = torch.randn(n, h, w, k, device=dev, generator=g)
        elif res_mode == 2:
            res = torch.randn(n, rh, rw, k, device=dev, generator=g)
        xa = x[..., :c1].contiguous() if dual else x
        xb = x[..., c1:].contiguous() if dual else None
        outs = []
        for rep in range(2):
            y = poisoned((n, h, w, k), torch.float32, rep)
            rc = lib.seam_conv1x1_sw_f32(P(xa), P(xb), P(wt), P(shift), P(res), P(y), m, c1, c2, k, relu, res_mode,
                                         h if res_mode == 2 else 0, w if res_mode == 2 else 0, rh if res_mode == 2 else 0,
                                         rw if res_mode == 2 else 0, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        full = res
        if res_mode == 2:
            full = F.interpolate(res.permute(0, 3, 1, 2), size=(h, w), mode="nearest").permute(0, 2, 3, 1)
        acc = (x.reshape(m, c) @ wt.t()).view(n, h, w, k)
        refs = [("torch fp32 matmul", torch_epilogue(acc, None, shift, full, relu))]
        wi = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred(c, 1, 1)), dtype=torch.float32, device=dev)
        assert lib.seam_pack_conv_weight_f32(P(wt), P(wi), k, c, 1, 1, c, 0, st()) == 0
        yi = poisoned((n, h, w, k), torch.float32, 0)
        fr = full.contiguous() if full is not None else None
        assert lib.seam_conv2d_f32(P(x), P(wi), None, P(shift), P(fr), P(yi), n, h, w, c, k, 1, 1, 1, 0, relu, st()) == 0
        refs.append(("implicit GEMM", yi))
        if conv_checked < 10:
            conv_checked += 1
            refs.append(("torch F.conv2d", torch_epilogue(F.conv2d(x.permute(0, 3, 1, 2), wt[:, :, None, None]).permute(0, 2, 3, 1), None, shift, full, relu)))
        check("conv1x1_sw", desc, outs[0], outs[1], refs, 2e-5)
    dummy = torch.zeros(1 << 16, device=dev)
    for (c, k) in [(288, 64), (64, 96), (48, 64), (64, 768), (64, 8448)]:
        if lib.seam_conv1x1_sw_f32(P(dummy), None, P(dummy), P(dummy), None, P(dummy), 64, c, 0, k, 0, 0, 0, 0, 0, 0, st()) == 0:
            fails.append(("conv1x1_sw", f"c={c} k={k}", "unserved channel count was not refused"))
    say(f"SUMMARY conv1x1_sw cases {done} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ conv1x1_f16pc (fp16, long reductions)
def stress_pwhpc(rng):
    t0 = time.time()
    done = exact = 0
    while done < NCASE:
        c = rng.choice([512, 768, 1024, 1536, 2048])
        k = rng.choice([128, 256, 384, 512, 1024, 2048])
        h, w = dim(rng, 1, 120), dim(rng, 1, 120)
        n = pick_n(rng, h * w * max(c, k), 3 << 20)
        m = n * h * w
        if lib.seam_conv1x1_f16pc_supported(m, c, k) != 1:
            continue
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1])
        desc = f"m={m} c={c} k={k} relu={relu}"
        say("START conv1x1_f16pc", desc)
        x = torch.randn(m, c, device=dev, generator=g).half()
        wt = (torch.randn(k, c, device=dev, generator=g) / math.sqrt(c)).half().float()
        scale, shift = epilogue_vectors(rng, k, g)
        wp = torch.empty((int(lib.seam_conv1x1_f16pc_weight_halves(k, c)),), dtype=torch.float16, device=dev)
        assert lib.seam_pack_conv1x1_weight_f16pc(P(wt), P(wp), k, c, st()) == 0
        outs = []
        for rep in range(2):
            y = poisoned((m, k), torch.float16, rep)
            rc = lib.seam_conv1x1_f16pc(P(x), P(wp), P(scale), P(shift), None, P(y), m, c, k, relu, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        refs = [("torch fp32 matmul", torch_epilogue(x.float() @ wt.t(), scale, shift, None, relu))]
        wi = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred_f16(c, 1, 1)), dtype=torch.float16, device=dev)
        assert lib.seam_pack_conv_weight_f16(P(wt), P(wi), k, c, 1, 1, c, 0, st()) == 0
        yi = poisoned((m, k), torch.float16, 0)
        assert lib.seam_conv2d_f16(P(x), P(wi), P(scale), P(shift), None, P(yi), 1, 1, m, c, k, 1, 1, 1, 0, relu, 0, st()) == 0
        refs.append(("implicit GEMM (fp16)", yi))
        exact += int(torch.equal(outs[0], yi))
        check("conv1x1_f16pc", desc, outs[0], outs[1], refs, 2e-3)
    dummy = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    for (c, k) in [(256, 128), (384, 256), (640, 128), (512, 64), (512, 192)]:
        if lib.seam_conv1x1_f16pc(P(dummy), P(dummy), None, None, None, P(dummy), 64, c, k, 0, st()) == 0:
            fails.append(("conv1x1_f16pc", f"c={c} k={k}", "unserved channel count was not refused"))
    if lib.seam_conv1x1_f16pc(P(dummy), P(dummy), None, None, P(dummy), P(dummy), 64, 512, 128, 0, st()) == 0:
        fails.append(("conv1x1_f16pc", "residual", "a residual operand was not refused"))
    say(f"SUMMARY conv1x1_f16pc cases {done} bit-identical-to-implicit-GEMM {exact} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ conv1x1_swh (fp16)
def stress_swh(rng):
    t0 = time.time()
    done = conv_checked = 0
    while done < NCASE:
        c = rng.choice([64, 128, 192, 256, 320, 512, 768, 1024])
        k = rng.choice([64, 128, 256, 512, 1024, 2048])
        h, w = dim(rng, 1, 150), dim(rng, 1, 150)
        n = pick_n(rng, h * w * max(c, k), 3 << 20)
        m = n * h * w
        dual = c % 128 == 0 and rng.random() < 0.25
        c1, c2 = (c // 2, c // 2) if dual else (c, 0)
        if lib.seam_conv1x1_swh_config(m, c1, c2, k) == 0:
            continue
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1])
        res_mode = rng.choice([0, 0, 1, 2]) if not dual else rng.choice([0, 0, 1])
        if res_mode == 2 and h * w < 128:
            res_mode = 1
        desc = f"n={n} {h}x{w} c={c1}+{c2} k={k} relu={relu} res_mode={res_mode} cfg={lib.seam_conv1x1_swh_config(m, c1, c2, k)}"
        say("START conv1x1_swh", desc)
        x = torch.randn(m, c, device=dev, generator=g).half()
        wt = (torch.randn(k, c, device=dev, generator=g) / math.sqrt(c)).half()
        scale, shift = epilogue_vectors(rng, k, g)
        rh, rw = (h + 1) // 2, (w + 1) // 2
        res = full = None
        if res_mode == 1:
            res = full = torch.randn(m, k, device=dev, generator=g).half()
        elif res_mode == 2:         # FPN top-down merge: a coarse map under a nearest-neighbour upsample
            res = torch.randn(n, rh, rw, k, device=dev, generator=g).half()
            full = F.interpolate(res.permute(0, 3, 1, 2).float(), size=(h, w), mode="nearest").permute(0, 2, 3, 1).reshape(m, k).half()
        xa = x[:, :c1].contiguous() if dual else x
        xb = x[:, c1:].contiguous() if dual else None
        outs = []
        for rep in range(2):
            y = poisoned((m, k), torch.float16, rep)
            rc = lib.seam_conv1x1_swh_f16(P(xa), P(xb), P(wt), P(scale), P(shift), P(res), P(y), m, c1, c2, k, relu, res_mode,
                                          h if res_mode == 2 else 0, w if res_mode == 2 else 0, rh if res_mode == 2 else 0,
                                          rw if res_mode == 2 else 0, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        acc = x.float() @ wt.float().t()
        refs = [("torch fp32 matmul", torch_epilogue(acc, scale, shift, None if full is None else full.float(), relu))]
        res = full.contiguous() if full is not None else None
        wi = torch.empty((lib.seam_conv_rows_padded(k), lib.seam_conv_kred_f16(c, 1, 1)), dtype=torch.float16, device=dev)
        wf = wt.float()
        assert lib.seam_pack_conv_weight_f16(P(wf), P(wi), k, c, 1, 1, c, 0, st()) == 0
        yi = poisoned((m, k), torch.float16, 0)
        assert lib.seam_conv2d_f16(P(x), P(wi), P(scale), P(shift), P(res), P(yi), 1, 1, m, c, k, 1, 1, 1, 0, relu, 0, st()) == 0
        refs.append(("implicit GEMM (fp16)", yi))
        check("conv1x1_swh", desc, outs[0], outs[1], refs, 2e-3)
    dummy = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    for (c, k) in [(96, 256), (1024, 256), (32, 64), (64, 96), (576, 128), (256, 64)]:
        if lib.seam_conv1x1_swh_f16(P(dummy), None, P(dummy), None, None, None, P(dummy), 64, c, 0, k, 0, 0, 0, 0, 0, 0, st()) == 0:
            fails.append(("conv1x1_swh", f"c={c} k={k}", "unserved channel count was not refused"))
    say(f"SUMMARY conv1x1_swh cases {done} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ the fp16 stem (flattened-shift form)
def stress_stem(rng):
    """seam_stem_s2d_swh_f16 on the padded space-to-depth frame"""
    t0 = time.time()
    done = 0
    while done < NCASE:
        h, w = dim(rng, 2, 150), dim(rng, 2, 150)
        if (h + 3) * (w + 3) < 128:
            continue
        n = pick_n(rng, h * w * 64, 3 << 20)
        done += 1
        g = gen(rng)
        relu = rng.choice([0, 1])
        scale, shift = epilogue_vectors(rng, 64, g)
        desc = f"stem n={n} {h}x{w} relu={relu}"
        say("START stem_swh", desc)
        x = torch.randn(n, h, w, 16, device=dev, generator=g).half()
        x[..., 12:] = 0
        ws = (torch.randn(64, 16, 4, 4, device=dev, generator=g) / math.sqrt(192)).half()
        rows = ws.permute(0, 2, 3, 1).reshape(64, 256).contiguous()
        xp = F.pad(x, (0, 0, 2, 1, 2, 1))
        outs = []
        for rep in range(2):
            y = poisoned((n, h, w, 64), torch.float16, rep)
            rc = lib.seam_stem_s2d_swh_f16(P(xp), P(rows), P(scale), P(shift), P(y), n, h, w, relu, st())
            assert rc == 0, (desc, rc)
            outs.append(y)
        acc = F.conv2d(xp.permute(0, 3, 1, 2).float(), ws.float()).permute(0, 2, 3, 1)
        check("stem_swh", desc, outs[0], outs[1], [("torch F.conv2d (fp32)", torch_epilogue(acc, scale, shift, None, relu))], 2e-3)
    dummy = torch.zeros(1 << 16, dtype=torch.float16, device=dev)
    if lib.seam_stem_s2d_swh_f16(P(dummy), P(dummy), None, None, P(dummy), 1, 5, 5, 0, st()) == 0:
        fails.append(("stem_swh", "stem 5x5", "a frame of fewer than 128 padded cells was not refused"))
    say(f"SUMMARY stem_swh cases {done} seconds {time.time() - t0:.1f}")


FAMILIES = [("wino24pc", stress_wino24pc), ("conv1x1_pc", stress_pwpc), ("f16pc", stress_f16pc), ("conv1x1_sw", stress_sw),
            ("conv1x1_swh", stress_swh), ("stem_swh", stress_stem), ("conv1x1_f16pc", stress_pwhpc)]


def main(argv):
    global NCASE, SEED, _native, dev, lib, ops
    sys.path.insert(0, ROOT)
    import seam_match_rcnn_amd.ops as ops
    from seam_match_rcnn_amd import _native
    NCASE, SEED = int(argv[0]), int(argv[1])
    dev = torch.device("cuda:0")
    lib = _native.lib()
    for idx, (name, fn) in enumerate(FAMILIES):
        if len(argv) > 2 and name not in argv[2:]:
            continue
        before = len(fails)
        fn(random.Random(SEED * 7919 + idx))
        torch.cuda.synchronize()
        say("KERNEL", name, "failures", len(fails) - before)
    say("DONE failures", len(fails))
    for f in fails[:40]:
        say("FAILED", *f)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

