"""The child of ``test_gpu_stress_train.py``: ``python stress_child_train.py NCASE SEED [family ...]`` runs the sweep on the GPU and
prints the lines ``stress_kit.family_ok`` reads.  Importing it launches nothing."""
import ctypes as C, functools, os, random, sys, time
import torch
import torch.nn.functional as F
import train_refs as TR
import stress_kit
from stress_kit import P, fail, fails, say, st, twice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32 = torch.float64, torch.float32
U = TR.U
refused = functools.partial(stress_kit.refused, start=False)           # this sweep's callers print their own START lines


def check(name, desc, what, got, ref, tol):
    """|got - ref| <= tol elementwise (tol 0: bit-exact to the float64 value, which must then be an fp32 number)."""
    got = got.to(F64)
    ref = ref.to(F64)
    if got.shape != ref.shape:
        fail(name, desc, f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}")
        return False
    tol = torch.as_tensor(tol, dtype=F64, device=got.device)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        tb = tol.expand_as(err).reshape(-1)[i]
        fail(name, desc, f"{what}: {int(bad.sum())} of {bad.numel()} off; first at flat {i}: got {float(got.reshape(-1)[i])!r} "
                         f"want {float(ref.reshape(-1)[i])!r} tol {float(tb):.3g}")
        return False
    return True


def gen(rng):
    g = torch.Generator(device=dev)
    g.manual_seed(rng.randrange(1 << 30))
    return g


def ints(shape, g, lo=-2, hi=2):
    return torch.randint(lo, hi + 1, shape, generator=g, device=dev).to(F32)


def normal(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device=dev) * scale


# ------------------------------------------------------------------------------------------------ conv wgrad
def wgrad_plan(M, C, K, R, S):
    tk, tc, nch = (K + 127) // 128, (C + 127) // 128, (M + 31) // 32
    tiles = tk * tc * R * S
    splits = max(1, min((1024 + tiles - 1) // tiles, nch))
    cps = (nch + splits - 1) // splits
    return tiles, nch, (nch + cps - 1) // cps, cps


def wgrad_case(rng, N, H, W, Cc, K, R, S, stride, pad, exact, name="conv_wgrad", rows=None):
    Ho, Wo = TR.conv_out(H, W, R, S, stride, pad)
    M = N * Ho * Wo
    tiles, nch, splits, cps = wgrad_plan(M, Cc, K, R, S)
    desc = f"N{N} H{H} W{W} C{Cc} K{K} {R}x{S} s{stride} p{pad} M{M} tiles{tiles} splits{splits} cps{cps} exact{int(exact)}"
    say("START", name, desc)
    g = gen(rng)
    x = ints((N, H, W, Cc), g) if exact else normal((N, H, W, Cc), g)
    dy = ints((N, Ho, Wo, K), g) if exact else normal((N, Ho, Wo, K), g)
    wsn = int(lib.seam_conv_wgrad_workspace_floats(M, Cc, K, R, S))
    if wsn != splits * R * S * K * Cc:
        fail(name, desc, f"workspace {wsn} != splits*R*S*K*C")
    out = twice(name, desc, [(K, Cc, R, S), (wsn,)],
                lambda b: lib.seam_conv_wgrad_f32(P(x), P(dy), P(b[0].t), N, H, W, Cc, K, R, S, stride, pad, P(b[1].t), st()),
                live=[True, "ws"])
    if out is None:
        return splits
    dw = out[0]
    if rows is not None:
        dw = dw[rows]
        ref = TR.wgrad_rows(x, dy, R, S, stride, pad, rows)
    else:
        ref = TR.wgrad(x, dy, R, S, stride, pad)
    if exact:
        check(name, desc, "dW (exact)", dw, ref, 0.0)
    else:
        # L: each split chains 32-pixel chunks of 16 MFMA 32x32x2 steps (2 products, <= 2 roundings per step: 2 per pixel),
        # then the reduce kernel adds the `splits` partials in order
        maj = TR.wgrad(x.abs(), dy.abs(), R, S, stride, pad)
        check(name, desc, "dW", dw, ref, TR.bound(maj, 2 * cps * 32 + splits + 1))
    return splits


def stress_wgrad(rng):
    t0 = time.time()
    done = exact_n = 0
    regimes = {"one": 0, "single_tile": 0, "few_chunks": 0, "other": 0}
    TAPS = [(1, 1), (3, 3), (1, 3), (3, 1), (5, 5)]
    EDGE_CK = [4, 8, 124, 128, 132, 260, 256, 252, 36, 60, 64, 68]
    i = 0
    while done < NCASE:
        kind = i % 4
        i += 1
        R, S = rng.choice(TAPS)
        stride = rng.choice([1, 2])
        pad = rng.randint(0, max(R, S) - 1)
        if kind == 0:                                       # tiles >= 1024: one split
            R, S = 5, 5
            Cc = rng.choice([1024, 1028, 900, 1100, 1052])
            K = rng.choice([1024, 1100, 1096, 900])
            N, H, W = 1, rng.randint(1, 6), rng.randint(1, 6)
            pad = 4 if H < 5 or W < 5 else rng.randint(0, 4)
        elif kind == 1:                                     # one 128x128 tile: up to 1024 splits, long pixel axis
            R, S, pad, stride = 1, 1, 0, 1
            Cc, K = rng.choice([4, 8, 124, 128, 64, 36]), rng.choice([4, 8, 124, 128, 100, 32])
            N = rng.randint(1, 4)
            H, W = rng.randint(1, 180), rng.randint(1, 180)
        elif kind == 2:                                     # nchunks below the split target
            Cc, K = rng.choice(EDGE_CK), rng.choice(EDGE_CK)
            N, H, W = rng.randint(1, 2), rng.randint(1, 9), rng.randint(1, 9)
        else:
            Cc = rng.choice(EDGE_CK + [4 * rng.randint(1, 275)])
            K = rng.choice(EDGE_CK + [4 * rng.randint(1, 275)])
            N, H, W = rng.randint(1, 6), rng.randint(1, 40), rng.randint(1, 40)
            while N * H * W * max(Cc, K) > (6 << 20):
                H, W = max(1, H // 2), max(1, W // 2)
        Ho, Wo = TR.conv_out(H, W, R, S, stride, pad)
        if Ho <= 0 or Wo <= 0:
            continue
        M = N * Ho * Wo
        if rng.random() < 0.5 and M % 32 == 0 and kind != 0:
            H += 1                                           # prefer a partial last chunk
            Ho, Wo = TR.conv_out(H, W, R, S, stride, pad)
            M = N * Ho * Wo
        tiles, nch, splits, cps = wgrad_plan(M, Cc, K, R, S)
        reg = "one" if tiles >= 1024 else ("single_tile" if tiles == 1 and splits > 1 else
                                          ("few_chunks" if nch < (1024 + tiles - 1) // tiles else "other"))
        regimes[reg] += 1
        exact = done % 3 == 0
        wgrad_case(rng, N, H, W, Cc, K, R, S, stride, pad, exact)
        done += 1
        exact_n += exact
    # the pixel axis at its longest: M ~ 1e5 on one tile (1024 splits of few chunks)
    wgrad_case(rng, 2, 250, 211, 12, 8, 1, 1, 1, 0, True); done += 1; exact_n += 1
    wgrad_case(rng, 1, 317, 317, 128, 128, 1, 1, 1, 0, False); done += 1
    # just under each 2^31-byte cap (1x1, K = C = 1024; M*K*4 = 2^31 - 4096), exact on sampled rows of dW
    wgrad_case(rng, 1, 524287, 1, 1024, 1024, 1, 1, 1, 0, True, rows=[0, 1, 511, 640, 1023]); done += 1; exact_n += 1
    torch.cuda.empty_cache()
    # refusals: nothing launched, dw keeps its poison
    tiny = torch.zeros(64, device=dev)
    for desc, (N, H, W, Cc, K, R, S, s_, p_) in [("C%4", (1, 4, 4, 6, 8, 1, 1, 1, 0)), ("K%4", (1, 4, 4, 8, 10, 1, 1, 1, 0)),
                                               ("Ho<=0", (1, 2, 5, 8, 8, 3, 3, 1, 0)), ("Wo<=0", (1, 5, 2, 8, 8, 3, 3, 1, 0)),
                                               ("N<=0", (0, 4, 4, 8, 8, 1, 1, 1, 0))]:
        say("START conv_wgrad refuse", desc)
        refused("conv_wgrad", "refuse " + desc, [(max(K, 1), Cc, R, S), (4096,)],
                lambda b: lib.seam_conv_wgrad_f32(P(tiny), P(tiny), P(b[0].t), N, H, W, Cc, K, R, S, s_, p_, P(b[1].t), st()))
    # the byte caps, with real-size operands (a broken refusal would stay in bounds): M*K*4 = 2^31, N*H*W*C*4 = 2^31
    for desc, (H, Cc, K) in [("M*K*4>=2^31", (524288, 4, 1024)), ("N*H*W*C*4>=2^31", (524288, 1024, 4))]:
        say("START conv_wgrad refuse", desc)
        x = torch.empty((H * Cc,), device=dev)
        dy = torch.empty((H * K,), device=dev)
        wsn = int(lib.seam_conv_wgrad_workspace_floats(H, Cc, K, 1, 1))
        refused("conv_wgrad", "refuse " + desc, [(K, Cc, 1, 1), (wsn,)],
                lambda b: lib.seam_conv_wgrad_f32(P(x), P(dy), P(b[0].t), 1, H, 1, Cc, K, 1, 1, 1, 0, P(b[1].t), st()))
        del x, dy
    torch.cuda.empty_cache()
    say(f"SUMMARY conv_wgrad cases {done} exact {exact_n} one_split {regimes['one']} single_tile {regimes['single_tile']} "
        f"few_chunks {regimes['few_chunks']} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ colsum
def colsum_plan(M):
    slabs = min(128, max(1, (M + 127) // 128))
    return slabs, (M + slabs - 1) // slabs


def stress_colsum(rng):
    t0 = time.time()
    done = exact_n = 0
    MS = [0, 1, 127, 128, 129, 128 * 128 - 1, 128 * 128, 128 * 128 + 1, 1000000, 3, 64, 255, 257, 4097, 99991]
    KS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4100]
    for i in range(max(NCASE, 110)):
        M = MS[i % len(MS)] if i < 60 else rng.choice(MS + [rng.randint(0, 300000)])
        K = rng.choice(KS) if i % 2 else rng.randint(1, 4100)
        while M * K > (16 << 20):
            K = max(1, K // 4)
        exact = i % 3 == 0
        slabs, rows_per = colsum_plan(M)
        desc = f"M{M} K{K} slabs{slabs} rows_per{rows_per} exact{int(exact)}"
        say("START colsum", desc)
        g = gen(rng)
        x = ints((M, K), g) if exact else normal((M, K), g)
        wsn = int(lib.seam_colsum_workspace_floats(M, K))
        out = twice("colsum", desc, [(K,), (wsn,)], lambda b: lib.seam_colsum_f32(P(x), P(b[0].t), M, K, P(b[1].t), st()),
                    live=[True, "ws"])
        done += 1
        exact_n += exact
        if out is None:
            continue
        ref = TR.colsum(x)
        # L: a thread chains ceil(rows_per / 4) rows, 3 adds join the 4 row groups, the final kernel chains the slabs
        L = (rows_per + 3) // 4 + 3 + slabs
        check("colsum", desc, "sum", out[0], ref, 0.0 if exact else TR.bound(TR.colsum(x.abs()), L))
    say(f"SUMMARY colsum cases {done} exact {exact_n} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ avgpool + relu bwd
def stress_avgpool(rng):
    t0 = time.time()
    done = exact_n = 0
    for i in range(NCASE):
        r = i % 5
        if r == 0:
            N, HW, Cc = rng.randint(1, 4), rng.randint(1, 64), 1
        elif r == 1:
            N, HW, Cc = rng.randint(1, 64), 1, rng.randint(1, 2048)
        elif r == 2:                                        # > 8192 * 256 elements: the grid-stride loop runs
            N, HW, Cc = rng.randint(40, 80), 36, rng.choice([1024, 1000, 1031])
        else:
            N, HW, Cc = rng.randint(1, 40), rng.choice([36, 49, 1, 2, 3, 7, 64, 100]), rng.randint(1, 1100)
        exact = HW & (HW - 1) == 0 and i % 7 != 0           # a power of two, no subnormal result: dpool / HW is exact
        desc = f"N{N} HW{HW} C{Cc} total{N * HW * Cc}"
        say("START avgpool_relu_bwd", desc)
        g = gen(rng)
        y = normal((N, HW, Cc), g)
        kinds = torch.randint(0, 4, (N, HW, Cc), generator=g, device=dev)
        y = torch.where(kinds == 0, torch.zeros_like(y), y)                              # exact zeros
        y = torch.where(kinds == 1, torch.full_like(y, 1.0e-40) * (1 + y.abs()), y)       # subnormal positives
        y = torch.where(kinds == 2, -y.abs() - 1e-30, y)                                   # negatives
        dpool = normal((N, Cc), g)
        if i % 7 == 0:
            dpool = dpool * 1e-37                                                          # results in the subnormal range
        out = twice("avgpool_relu_bwd", desc, [(N, HW, Cc)],
                    lambda b: lib.seam_avgpool_relu_bwd_f32(P(dpool), P(y), P(b[0].t), N, HW, Cc, st()))
        done += 1
        exact_n += exact
        if out is None:
            continue
        ref = TR.avgpool_relu_bwd(dpool, y)
        got = out[0]
        # the mask exactly: zero where y <= 0 (subnormal y > 0 included), non-zero wherever dpool / HW is non-zero in fp32
        if not torch.equal(got != 0, ref.to(F32) != 0):
            fail("avgpool_relu_bwd", desc, f"ReLU mask differs at {int(((got != 0) != (ref.to(F32) != 0)).sum())} elements")
        else:
            check("avgpool_relu_bwd", desc, "dy", got, ref, 0.0 if exact else TR.ulp32(ref))
    say(f"SUMMARY avgpool_relu_bwd cases {done} exact {exact_n} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ BatchNorm1d
def bn_bounds(x, M, ref, gamma, beta, mom, rm, rv, eps):
    """Elementwise error bounds of the fp32 training forward (derivation inline)."""
    x = x.to(F64)
    C2 = TR.C_ERR
    m = ref["mean"]
    dev_abs = (x - m).abs().mean(0)
    # mean0 = x0 + sum(x - x0) / M: terms rounded once, a chain of M, the division and the add of x0
    e0 = C2 * U * ((M + 2) * (x - x[0]).abs().mean(0) + m.abs())
    # mean = mean0 + sum(x - mean0) / M is exact algebra; its error: the terms d (1 rounding each), the chain of M, the
    # division, and the two adds (|m| each)
    em = C2 * U * ((M + 2) * (dev_abs + e0) + 2 * m.abs())
    vb = x.var(0, unbiased=False)
    # var = sum d^2 - (sum d)^2 / M with d = x - mean0 is exactly sum (x - m)^2; rounding: d (1, twice in d^2), the chain
    # of M fmaf, the correction (3) and the division (1); sum d^2 = M (vb + (mean0 - m)^2)
    ev = C2 * U * (M + 6) * (vb + e0 * e0)
    # invstd = 1 / sqrtf(vb + eps): half the relative error of its argument, plus the add, sqrt and division
    rel_inv = 0.5 * ev / (vb + eps) + C2 * 3 * U
    inv = ref["invstd"]
    g = gamma.to(F64).abs()
    xm = (x - m).abs()
    # y = (x - mean) * inv * g + beta: the mean's error, inv's relative error, and 4 roundings of the result's terms
    ey = g * inv * (em + xm * rel_inv) + C2 * 4 * U * (xm * inv * g + beta.to(F64).abs() + ref["y"].abs())
    out = dict(y=ey, mean=em, invstd=rel_inv * inv)
    if rm is not None:
        rm, rv = rm.to(F64), rv.to(F64)
        out["run_mean"] = mom * em + C2 * 3 * U * ((1 - mom) * rm.abs() + mom * m.abs())
        vu = vb * M / (M - 1)
        out["run_var"] = mom * ev * M / (M - 1) + C2 * 4 * U * ((1 - mom) * rv.abs() + mom * vu)
    return out


def stress_bn(rng):
    t0 = time.time()
    done = exact_n = 0
    MS, FS = [2, 3, 17, 250, 4096, 20000], [1, 63, 64, 65, 256, 1024, 1030]
    eps = 1e-5
    for i in range(NCASE):
        M, Fd = MS[i % len(MS)], FS[(i // len(MS)) % len(FS)] if i < 42 else rng.choice(FS)
        if i >= 42:
            M = rng.choice(MS + [rng.randint(2, 600)])
        exact = i % 4 == 0
        frozen = i % 5 == 1
        momk = i % 3
        buffers = i % 7 != 3
        mom = [0.0, 1.0, 1.0 / max(1, i)][momk] if i % 2 else 0.1
        g = gen(rng)
        if exact:
            x = ints((M, Fd), g, -3, 3)
            dy = ints((M, Fd), g)
        else:
            off = torch.where(torch.rand((Fd,), generator=g, device=dev) < 0.5,
                              (torch.rand((Fd,), generator=g, device=dev) * 2 - 1) * 1000.0, torch.zeros((Fd,), device=dev))
            spread = torch.exp(torch.randn((Fd,), generator=g, device=dev) * 2).clamp(1e-2, 1e3)
            x = normal((M, Fd), g) * spread + off
            dy = normal((M, Fd), g)
        x[:, 0] = 0.1 if i % 2 else 7.0                                          # a constant column
        if Fd > 2:
            x[:, -1] = x[0, -1]
        gamma, beta = normal((Fd,), g) * 0.5 + 1, normal((Fd,), g)
        rm, rv = (normal((Fd,), g) * 0.1, normal((Fd,), g).abs() + 0.5) if buffers else (None, None)
        desc = f"M{M} F{Fd} mom{mom:.4g} buffers{int(buffers)} frozen{int(frozen)} exact{int(exact)}"
        say("START bn1d", desc)
        ref = TR.bn_train(x, gamma, beta, rm, rv, mom, eps, dy)

        def fwd(b):
            if buffers:
                b[3].t.copy_(rm); b[4].t.copy_(rv)
            return lib.seam_bn1d_train_fwd_f32(P(x), P(gamma), P(beta), P(b[0].t), P(b[1].t), P(b[2].t),
                                               P(b[3].t) if buffers else None, P(b[4].t) if buffers else None, M, Fd,
                                               C.c_float(mom), C.c_float(eps), st())
        out = twice("bn1d", desc, [(M, Fd), (Fd,), (Fd,), (Fd,), (Fd,)], fwd,
                    live=[True, True, True, True, True] if buffers else [True, True, True, False, False])
        done += 1
        if out is not None:
            bd = bn_bounds(x, M, ref, gamma, beta, mom, rm, rv, eps)
            check("bn1d", desc, "y", out[0], ref["y"], bd["y"])
            check("bn1d", desc, "save_mean", out[1], ref["mean"], bd["mean"])
            check("bn1d", desc, "save_invstd", out[2], ref["invstd"], bd["invstd"])
            if buffers:
                check("bn1d", desc, "running_mean", out[3], ref["run_mean"], bd["run_mean"])
                check("bn1d", desc, "running_var", out[4], ref["run_var"], bd["run_var"])
        # backward at the fp32-rounded float64 statistics (the reference then sees exactly the kernel's inputs)
        mean32, inv32 = ref["mean"].to(F32), ref["invstd"].to(F32)
        out = twice("bn1d", desc + " bwd", [(M, Fd), (Fd,), (Fd,)],
                    lambda b: lib.seam_bn1d_bwd_f32(P(dy), P(x), P(mean32), P(inv32), P(gamma), P(b[0].t), P(b[1].t), P(b[2].t),
                                                    M, Fd, int(frozen), st()))
        if out is None:
            continue
        dx, dg, db = TR.bn_backward(dy, x, mean32, inv32, gamma, frozen)
        x64, dy64, g64 = x.to(F64), dy.to(F64), gamma.to(F64)
        xh = ((x64 - mean32.to(F64)) * inv32.to(F64)).abs()
        e_sb = TR.bound(dy64.abs().sum(0), M)
        # sg = sum fmaf(dy, (x - mean) * inv): 2 roundings inside each term, M links
        e_sg = TR.bound((dy64.abs() * xh).sum(0), M + 2)
        if exact:
            exact_n += 1
            check("bn1d", desc, "dbeta (exact)", out[2], db, 0.0)
        else:
            check("bn1d", desc, "dbeta", out[2], db, e_sb)
        check("bn1d", desc, "dgamma", out[1], dg, e_sg)
        k = (g64 * inv32.to(F64)).abs()
        if frozen:
            # dx = (gamma * inv) * dy: two roundings
            edx = TR.C_ERR * 2 * U * k * dy64.abs()
        else:
            # dx = k (M dy - sb - xh sg), k = gamma inv / M: the errors of sb and sg, xh's 2 roundings, and 5 roundings of the
            # combination and of k
            sgv, sbv = (dy64 * (x64 - mean32.to(F64)) * inv32.to(F64)).sum(0), dy64.sum(0)
            edx = (k / M * (e_sb + xh * e_sg + TR.C_ERR * U * (2 * xh * sgv.abs() + 5 * (M * dy64.abs() + sbv.abs() + xh * sgv.abs())))
                   + TR.C_ERR * 2 * U * dx.abs())
        check("bn1d", desc, "dx", out[0], dx, edx)
    # refusals: M < 2 (forward), M <= 0 / F <= 0 (backward); nothing written
    one = torch.zeros(4096, device=dev)
    for Mr in (1, 0, -1):
        say("START bn1d refuse M", Mr)
        refused("bn1d", f"refuse fwd M{Mr}", [(4, 8), (8,), (8,), (8,), (8,)],
                lambda b: lib.seam_bn1d_train_fwd_f32(P(one), P(one), P(one), P(b[0].t), P(b[1].t), P(b[2].t), P(b[3].t), P(b[4].t),
                                                      Mr, 8, C.c_float(0.1), C.c_float(eps), st()))
    for Mr, Fr in ((0, 8), (4, 0)):
        say("START bn1d refuse bwd", Mr, Fr)
        refused("bn1d", f"refuse bwd M{Mr} F{Fr}", [(4, 8), (8,), (8,)],
                lambda b: lib.seam_bn1d_bwd_f32(P(one), P(one), P(one), P(one), P(one), P(b[0].t), P(b[1].t), P(b[2].t), Mr, Fr, 0, st()))
    say(f"SUMMARY bn1d cases {done} exact {exact_n} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ pair logits bwd
def stress_pair(rng):
    t0 = time.time()
    done = exact_n = 0
    for i in range(NCASE):
        r = i % 6
        if r == 0:
            Q, G = 1, 1
        elif r == 1:
            Q, G = rng.randint(150, 170), rng.randint(14, 18)              # the training batch
        elif r == 2:
            Q, G = rng.randint(1, 2000), rng.randint(1, 8)
        elif r == 3:
            Q, G = rng.randint(1, 8), rng.randint(1, 2000)
        elif r == 4 and i % 24 == 4:
            Q, G = rng.randint(1500, 2000), rng.randint(1500, 2000)
        else:
            Q, G = rng.randint(1, 300), rng.randint(1, 300)
        if (Q * G) % 256 == 0:
            G += 1
        exact = i % 3 == 0 and Q * G <= 400000          # |dw| <= 2 * 16 * Q * G < 2^24
        desc = f"Q{Q} G{G} QG{Q * G} exact{int(exact)}"
        say("START pair_logits_bwd", desc)
        g = gen(rng)
        mk = (lambda *s: ints(s, g)) if exact else (lambda *s: normal(s, g))
        a, b, w, gg = mk(Q, 256), mk(G, 256), mk(2, 256), mk(Q, G, 2)
        gg = gg * (torch.rand((Q, G, 1), generator=g, device=dev) > 0.2)           # zeros in g
        out = twice("pair_logits_bwd", desc, [(Q, 256), (G, 256), (2, 256), (2,)],
                    lambda bb: lib.seam_pair_logits_bwd_f32(P(a), P(b), P(w), P(gg), P(bb[0].t), P(bb[1].t), P(bb[2].t), P(bb[3].t),
                                                            Q, G, 256, st()))
        done += 1
        exact_n += exact
        if out is None:
            continue
        vals, majs = TR.pair_bwd(a, b, w, gg, chunk=max(1, (1 << 22) // (G * 256)))
        n = Q * G
        # da: per term 1 (a - b) + 2 (g0 w0 + g1 w1) roundings, a chain of G fmaf; db likewise over Q;
        # dw / dbias: per term 2 roundings (difference, square), a chain of ceil(QG / 256) per thread, then the
        # 64-lane butterfly (6) and the sum of 4 wave partials (3)
        Ls = [G + 3, Q + 3, (n + 255) // 256 + 2 + 9, (n + 255) // 256 + 9]
        for what, got, ref, maj, L in zip(("da", "db", "dw", "dbias"), out, vals, majs, Ls):
            check("pair_logits_bwd", desc, what, got, ref, 0.0 if exact else TR.bound(maj, L))
    one = torch.zeros(4096, device=dev)
    for Dd, Q, G in ((128, 4, 4), (255, 4, 4), (512, 4, 4), (256, 0, 4), (256, 4, 0)):
        say("START pair_logits_bwd refuse", Dd, Q, G)
        refused("pair_logits_bwd", f"refuse D{Dd} Q{Q} G{G}", [(4, 256), (4, 256), (2, 256), (2,)],
                lambda bb: lib.seam_pair_logits_bwd_f32(P(one), P(one), P(one), P(one), P(bb[0].t), P(bb[1].t), P(bb[2].t), P(bb[3].t),
                                                        Q, G, Dd, st()))
    say(f"SUMMARY pair_logits_bwd cases {done} exact {exact_n} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ NLB backward
NLB_REDRAWS = [0]


def nlb_pack(g, integer_ab):
    pk = dict(w_proj_t=normal((256, 384), g, 0.06), b_proj=normal((384,), g, 0.1), w_cat=normal((256,), g, 0.1),
              w_out_t=normal((128, 256), g, 0.09), b_out=normal((256,), g, 0.1), w_att=normal((256,), g, 0.1),
              b_att=normal((1,), g))
    if integer_ab:              # a, b exact in fp32 (see TR.relu_margin_hits); the g projection scaled so that |Y| stays ~1
        pk["w_proj_t"][:, :256] = ints((256, 256), g, -1, 1)
        pk["b_proj"][:256] = ints((256,), g)
        pk["w_cat"] = ints((256,), g, -1, 1)
        pk["w_proj_t"][:, 256:] *= 0.01
    return {k: v.contiguous() for k, v in pk.items()}


def nlb_case(rng, block, S, Tmax, lens, use_nlb, bm, pad_row, integer_ab, dz_layout=None, name="nlb_bwd"):
    g = gen(rng)
    rs = 256 + pad_row
    desc = (f"{'block' if block else 'attnpool'} S{S} Tmax{Tmax} use{use_nlb} {'bm' if bm else 'tm'} rs{rs} "
            f"int_ab{int(integer_ab)} lens{lens[:6]}{'..' if S > 6 else ''}")
    say("START", name, desc)
    pk = nlb_pack(g, integer_ab)
    p = TR.nlb_params(pk)
    size = S * Tmax * rs
    t_st, s_st = (rs, Tmax * rs) if bm else (S * rs, rs)
    # draw the sequence data; a live pair with a + b inside the fp32 error bound of a and b is redrawn
    for attempt in range(50):
        flat = ints((size,), g, -2, 2) if integer_ab else normal((size,), g)
        rows = TR.seq_rows(flat, t_st, s_st, lens, S, Tmax)
        nlb_on = [r.shape[0] > 0 and (use_nlb == 2 or (use_nlb == 1 and r.shape[0] > 1)) for r in rows]
        hits = sum(TR.relu_margin_hits(r, p) for r, on in zip(rows, nlb_on) if on)
        if hits == 0:
            break
        NLB_REDRAWS[0] += 1
    else:
        fail(name, desc, "no draw without a ReLU-margin pair in 50 attempts")
        return
    lens_d = torch.tensor(lens, dtype=torch.int32, device=dev)
    live = [i for i in range(S) if rows[i].shape[0] > 0]
    dsrs = rs
    if block:
        dz_bm, dz_pad = dz_layout
        drs = 256 + dz_pad
        dzt, dzs = (drs, Tmax * drs) if dz_bm else (S * drs, drs)
        dzflat = normal((S * Tmax * drs,), g)
        dzrows = TR.seq_rows(dzflat, dzt, dzs, lens, S, Tmax)
        desc += f" dz_{'bm' if dz_bm else 'tm'}{drs}"
        ngr, shapes = 9, [(128, 256), (128,), (128, 256), (128,), (128, 256), (128,), (256,), (256, 128), (256,)]
    else:
        dout = normal((S, 256), g)
        ngr, shapes = 11, [(128, 256), (128,), (128, 256), (128,), (128, 256), (128,), (256,), (256, 128), (256,), (256,), (1,)]
    wsn = int(lib.seam_nlb_bwd_workspace_floats(S, Tmax))
    live_mask = torch.zeros(size, dtype=torch.bool, device=dev)
    starts = [i * s_st + t * t_st for i in live for t in range(rows[i].shape[0])]
    if starts:
        idx = torch.tensor(starts, device=dev)[:, None] + torch.arange(256, device=dev)[None, :]
        live_mask[idx.reshape(-1)] = True

    def launch(b, lens_d=lens_d):
        arr = (C.c_void_p * ngr)(*[bb.t.data_ptr() for bb in b[1:1 + ngr]])
        ws = b[-1].t
        if block:
            return lib.seam_nlb_block_bwd_f32(P(flat), t_st, s_st, P(lens_d), S, Tmax, P(pk["w_proj_t"]), P(pk["b_proj"]),
                                              P(pk["w_cat"]), P(pk["w_out_t"]), P(pk["b_out"]), P(dzflat), dzt, dzs, P(b[0].t),
                                              arr, P(ws), use_nlb, st())
        return lib.seam_nlb_attnpool_bwd_f32(P(flat), t_st, s_st, P(lens_d), S, Tmax, P(pk["w_proj_t"]), P(pk["b_proj"]),
                                             P(pk["w_cat"]), P(pk["w_out_t"]), P(pk["b_out"]), P(pk["w_att"]), P(pk["b_att"]),
                                             P(dout), P(b[0].t), arr, P(ws), use_nlb, st())
    out = twice(name, desc, [(size,)] + shapes + [(wsn,)], launch, live=[live_mask] + [True] * ngr + ["ws"])
    if out is None:
        return
    if any(l > Tmax for l in lens):                         # a length above Tmax == a length of exactly Tmax, bit for bit
        lc = torch.tensor([min(l, Tmax) for l in lens], dtype=torch.int32, device=dev)
        out2 = twice(name, desc + " clamped", [(size,)] + shapes + [(wsn,)], lambda b: launch(b, lc),
                     live=[live_mask] + [True] * ngr + ["ws"])
        if out2 is not None and not all(torch.equal(u[m].view(torch.int32), v[m].view(torch.int32))
                                        for u, v, m in zip(out, out2, [live_mask] + [slice(None)] * ngr)):
            fail(name, desc, "len > Tmax differs from len == Tmax")
    seqs = [rows[i] for i in live]
    if block:
        dzl = [dzrows[i] for i in live]
        dx, grads = TR.nlb_bwd(seqs, p, use_nlb, dz=dzl)
        mdx, mgr = TR.nlb_majorants(seqs, p, use_nlb, dz=dzl)
        e_soft = 0.0
    else:
        dx, grads = TR.nlb_bwd(seqs, p, use_nlb, dout=dout[live])
        mdx, mgr = TR.nlb_majorants(seqs, p, use_nlb, dout=dout[live])
        # the attention logits e_t = Z_t . wa + ba carry an fp32 error up to bound(|Z| . |wa| + |ba|, 256 + 4 T + 265) (the
        # block's forward chains then the scorer's); softmax turns an error de in e into a relative error <= 2 max|de| of
        # every weight s_t, which scales every pooled-path gradient: it enters as that relative factor on the majorants
        e_soft = 0.0
        with torch.no_grad():
            for r in seqs:
                za = _zmaj(r, p) if (use_nlb == 2 or (use_nlb == 1 and r.shape[0] > 1)) else r.to(F64).abs()
                me = za @ p["attention_scorer.weight"].abs().reshape(-1) + p["attention_scorer.bias"].abs()
                e_soft = max(e_soft, 2 * float(TR.bound(me.max(), 256 + 4 * Tmax + 265)))
    # L: the per-row backward chains the block's forward (256 projection + T + 128 + scorer 265) and backward (265 ds,
    # T softmax, 256 dY, 128 dS, T da / db, T dG, 128 + 2 dX) stages -- each stage's relative error adds; the parameter
    # gradients then chain every row of every sequence (S * Tmax) and the assembly's 265
    L_row = 1700 + 4 * Tmax
    L_par = L_row + S * Tmax + 265
    dseq = out[0]
    for j, i in enumerate(live):
        T = rows[i].shape[0]
        got = torch.as_strided(dseq, (T, 256), (t_st, 1), dseq.storage_offset() + i * s_st)     # the body follows a guard
        ref = dx[j]
        if block and not (use_nlb == 2 or (use_nlb == 1 and T > 1)):
            check(name, desc, f"dseq[{i}] (bypass: exactly dz)", got, ref, 0.0)
        elif not check(name, desc, f"dseq[{i}]", got, ref, TR.bound(mdx[j], L_row) + e_soft * mdx[j]):
            break
    keys = list(p.keys())[:ngr]
    for k, got in zip(keys, out[1:1 + ngr]):
        ref = grads[k].reshape(got.shape)
        maj = mgr[k].reshape(got.shape)
        check(name, desc, k, got, ref, TR.bound(maj, L_par) + e_soft * maj)


def _zmaj(x, p):
    """Majorant of the block's output rows Z (all operands in absolute value, ReLU the identity)."""
    q = {k: v.abs() for k, v in p.items()}
    from oracle import heads as OH
    return OH.nlb_closed_form(x.to(F64).abs(), q)


def stress_nlb(rng):
    t0 = time.time()
    done = exactmask = 0
    for i in range(NCASE):
        block = i % 2 == 1
        use_nlb = [0, 1, 2][(i // 2) % 3]
        big = i % 10 == 9
        if big:
            S, Tmax = rng.randint(100, 300), rng.randint(8, 64)
        else:
            S, Tmax = rng.randint(1, 12), rng.choice([1, 2, 3, 5, 16, 33, 63, 64, rng.randint(1, 64)])
        lens = []
        for s in range(S):
            r = rng.random()
            lens.append(0 if r < 0.1 else 1 if r < 0.25 else Tmax + rng.randint(1, 5) if r < 0.35 else rng.randint(1, Tmax))
        if i % 8 == 0:
            lens[0] = Tmax
        pairs = sum(min(l, Tmax) ** 2 for l in lens)
        integer_ab = big or pairs > 300 or i % 4 == 0
        bm = rng.random() < 0.5
        pad_row = rng.choice([0, 0, 4, 12])
        dz_layout = (not bm if rng.random() < 0.7 else bm, rng.choice([0, 8, 20])) if block else None
        nlb_case(rng, block, S, Tmax, lens, use_nlb, bm, pad_row, integer_ab, dz_layout)
        done += 1
        exactmask += integer_ab
    # Tmax = 65 refused by both entry points with every output untouched; Tmax = 64 runs (above)
    g = gen(rng)
    pk = nlb_pack(g, False)
    seq = normal((4 * 65 * 256,), g)
    lens_d = torch.full((4,), 65, dtype=torch.int32, device=dev)
    shapes = [(4 * 65 * 256,)] + [(128, 256), (128,), (128, 256), (128,), (128, 256), (128,), (256,), (256, 128), (256,), (256,), (1,)]
    wsn = int(lib.seam_nlb_bwd_workspace_floats(4, 65))
    for block in (False, True):
        say("START nlb_bwd refuse Tmax65", "block" if block else "attnpool")
        ng = 9 if block else 11

        def launch(b):
            arr = (C.c_void_p * ng)(*[bb.t.data_ptr() for bb in b[1:1 + ng]])
            if block:
                return lib.seam_nlb_block_bwd_f32(P(seq), 256, 65 * 256, P(lens_d), 4, 65, P(pk["w_proj_t"]), P(pk["b_proj"]),
                                                  P(pk["w_cat"]), P(pk["w_out_t"]), P(pk["b_out"]), P(seq), 256, 65 * 256,
                                                  P(b[0].t), arr, P(b[-1].t), 2, st())
            return lib.seam_nlb_attnpool_bwd_f32(P(seq), 256, 65 * 256, P(lens_d), 4, 65, P(pk["w_proj_t"]), P(pk["b_proj"]),
                                                 P(pk["w_cat"]), P(pk["w_out_t"]), P(pk["b_out"]), P(pk["w_att"]), P(pk["b_att"]),
                                                 P(seq), P(b[0].t), arr, P(b[-1].t), 1, st())
        refused("nlb_bwd", f"refuse Tmax65 {'block' if block else 'attnpool'}", shapes[:1 + ng] + [(wsn,)], launch)
    say(f"SUMMARY nlb_bwd cases {done} exact {exactmask} redraws {NLB_REDRAWS[0]} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ ce2
def stress_ce2(rng):
    t0 = time.time()
    done = exact_n = nan_n = 0
    WEIGHTS = [(1.0, 0.3), (0.0, 1.0), (1e-3, 1e3), (1.0, 1.0), (0.3, 1.0)]
    for i in range(NCASE + 10):
        r = i % 5
        n = [1, 2, 255, 256, 257][i % 5] if i < 15 else (rng.randint(150000, 200000) if i % 11 == 0 else rng.randint(1, 5000))
        wt = WEIGHTS[i % len(WEIGHTS)]
        tk = (i // 5) % 3                                   # all 0, all 1, mixed
        exact = i % 6 == 0                                  # tied logits, unit weights, n a power of two: p1 = 1/2, k = 1/n
        if exact:
            n = 1 << rng.randint(0, 17)
        g = gen(rng)
        if exact:
            wt = (1.0, 1.0)
            x = ints((n, 1), g, -80, 80).expand(n, 2).contiguous()
        elif r == 0:
            x = normal((n, 2), g)
        elif r == 1:                                        # saturated: gaps above 100
            x = normal((n, 2), g, 3.0)
            x[:, 0] = (torch.rand((n,), generator=g, device=dev) * 160 - 80)
            x[:, 1] = x[:, 0] + torch.where(torch.rand((n,), generator=g, device=dev) < 0.5, -1.0, 1.0) * (100 + 60 * torch.rand((n,), generator=g, device=dev))
        else:
            x = (torch.rand((n, 2), generator=g, device=dev) * 160 - 80)
        tgt = (torch.zeros(n, dtype=torch.int64, device=dev) if tk == 0 else torch.ones(n, dtype=torch.int64, device=dev) if tk == 1
               else (torch.rand((n,), generator=g, device=dev) < 0.5).to(torch.int64))
        w = torch.tensor(wt, device=dev)
        desc = f"n{n} w{wt} targets{['0', '1', 'mixed'][tk]} exact{int(exact)}"
        say("START ce2", desc)
        out = twice("ce2", desc, [(1,), (n, 2)],
                    lambda b: lib.seam_ce2_fwd_bwd_f32(P(x), P(tgt), P(w), P(b[0].t), P(b[1].t), n, st()))
        done += 1
        if out is None:
            continue
        loss, dl = TR.ce2(x, tgt, w)
        if bool(torch.isnan(loss)):                         # every selected weight 0: NaN, as float64 torch gives
            nan_n += 1
            if not (bool(torch.isnan(out[0]).all()) and bool(torch.isnan(out[1]).all())):
                fail("ce2", desc, "weights of the selected classes sum to 0: want NaN loss and gradients")
            continue
        x64 = x.to(F64)
        wi = w.to(F64)[tgt]
        sw = wi.sum()
        m = x64.max(1).values
        dlt = (x64[:, 1] - x64[:, 0]).abs()
        lse = torch.logsumexp(x64, 1)
        xy = x64.gather(1, tgt[:, None])[:, 0]
        Ls = (n + 255) // 256 + 9                           # per-thread chain, then the block sum (6 + 3)
        C2 = TR.C_ERR
        # loss = sum w (lse - x_y) / sum w: each term's lse = m + logf(expf(.) + expf(.)) carries (|gap| + 5) u from the
        # exponents' rounded arguments, expf / logf and the add, plus u |lse| and u |lse - x_y| for the two subtractions
        e_sl = C2 * U * (wi * (dlt + 6 + lse.abs() + (lse - xy).abs())).sum() + TR.bound((wi * (lse - xy).abs()).sum(), Ls)
        e_sw = TR.bound(wi.sum(), Ls)
        e_loss = e_sl / sw + loss.abs() * (e_sw / sw + C2 * U)
        check("ce2", desc, "loss", out[0][0], loss, e_loss)
        p1 = torch.softmax(x64, 1)[:, 1]
        k = wi / sw
        # dlogits: p1 = e1 / (e0 + e1) carries (|gap| + 6) u relative (2 exponent arguments and the exps, the add, the
        # division), p1 - y one rounding, k = w / sw the error of sw plus one rounding
        # and an absolute floor for fp32's range: an expf result in the subnormal range (or flushed to 0) is off by up to
        # 2^-149 absolute, p1 and k (p1 - y) add one subnormal rounding each (k <= 1)
        e_g = (k * (C2 * U * (2 * (dlt + 6) * p1 + (p1 - (tgt == 1).to(F64)).abs())) + dl[:, 1].abs() * (e_sw / sw + C2 * 2 * U)
               + C2 * 3 * 2.0 ** -149)
        if exact:
            exact_n += 1
            check("ce2", desc, "dlogits (exact)", out[1], dl, 0.0)
        else:
            check("ce2", desc, "dlogits", out[1], dl, torch.stack([e_g, e_g], 1))
    one = torch.zeros(16, device=dev)
    onei = torch.zeros(16, dtype=torch.int64, device=dev)
    for n in (0, -1):
        say("START ce2 refuse n", n)
        refused("ce2", f"refuse n{n}", [(1,), (4, 2)],
                lambda b: lib.seam_ce2_fwd_bwd_f32(P(one), P(onei), P(one), P(b[0].t), P(b[1].t), n, st()))
    say(f"SUMMARY ce2 cases {done} exact {exact_n} nan {nan_n} seconds {time.time() - t0:.1f}")


FAMILIES = [("conv_wgrad", stress_wgrad), ("colsum", stress_colsum), ("avgpool_relu_bwd", stress_avgpool), ("bn1d", stress_bn),
            ("pair_logits_bwd", stress_pair), ("nlb_bwd", stress_nlb), ("ce2", stress_ce2)]


def main(argv):
    global NCASE, SEED, dev, lib
    sys.path.insert(0, ROOT)
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
