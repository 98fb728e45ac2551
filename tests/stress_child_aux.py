"""The child of ``test_gpu_stress_aux.py``: ``python stress_child_aux.py NCASE SEED [family ...]`` runs the sweep on the GPU and
prints the lines ``stress_kit.family_ok`` reads.  Importing it launches nothing."""
import math, os, random, sys, time
import torch
import torch.nn.functional as F
import stress_kit
from stress_kit import P, fail, fails, say, st

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMES = [p for p in range(3, 4000) if all(p % q for q in range(2, int(p ** 0.5) + 1))]
BUDGET = 16 << 20          # bytes per tensor, except the named large cases


def rand(shape, dtype, g, neg=False):
    x = torch.randn(shape, device=dev, generator=g)
    if neg:
        x = -x.abs() - 0.5
    return x.to(dtype)


def gen(rng):
    g = torch.Generator(device=dev)
    g.manual_seed(rng.randrange(1 << 30))
    return g


def odd_cv(rng, hi=4000):
    r = rng.random()
    if r < 0.4:
        return rng.choice([p for p in PRIMES if p <= hi])
    if r < 0.7:
        return rng.randrange(1, hi, 2)
    return rng.choice([1, 2, 3, 4, 8, 16, 32, 64])


def dim(rng, lo, hi):
    hi = max(lo, hi)
    r = rng.random()
    if r < 0.3:
        return rng.choice([v for v in [lo, lo + 1, hi, hi - 1] + [p for p in PRIMES[:60]] if lo <= v <= hi])
    return rng.randint(lo, hi)


def twice(launch, shape, dtype, name, desc):
    """launch(y) -> rc into two poisoned outputs; the results must agree bit for bit and the guards must hold."""
    out = stress_kit.twice(name, desc, [shape], lambda bf: launch(bf[0].t), dtypes=[dtype])
    return None if out is None else out[0]


# ------------------------------------------------------------------------------------------------ maxpool
def maxpool_case(rng, dt, N, H, W, C, k, s, p, neg, name="maxpool"):
    E = 4 if dt == torch.float32 else 8
    g = gen(rng)
    x = rand((N, H, W, C), dt, g, neg)
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    desc = f"{str(dt)[6:]} N{N} H{H} W{W} C{C} cv{C // E} k{k} s{s} p{p} neg{int(neg)}"
    say("START", name, desc)
    fast = lib.seam_maxpool2d_fast(N, H, W, C, k, s, p, int(dt == torch.float16))
    fn = lib.seam_maxpool2d_f32 if dt == torch.float32 else lib.seam_maxpool2d_f16
    y = twice(lambda y: fn(P(x), P(y), N, H, W, C, k, s, p, st()), (N, Ho, Wo, C), dt, name, desc)
    if y is None:
        return fast
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    if not torch.equal(y.float(), ref):
        bad = int((y.float() != ref).sum())
        fail(name, desc, f"{bad} of {ref.numel()} outputs differ from F.max_pool2d (fast path {fast})")
    return fast


def stress_maxpool(rng):
    t0 = time.time()
    done = nfast = nslow = 0
    # the two shapes the old launcher computed wrongly (cv = 3906, 17 x 17 outputs), both dtypes; and the model's stem window
    for dt, C in ((torch.float32, 15624), (torch.float16, 31248)):
        f = maxpool_case(rng, dt, 1, 34, 34, C, 3, 2, 1, False)
        nfast += f; nslow += 1 - f; done += 1
    for dt in (torch.float32, torch.float16):
        f = maxpool_case(rng, dt, 2, 40, 50, 64, 3, 2, 1, False)
        if not f:
            fail("maxpool", f"{dt} C64", "the stem shape left the fast kernel")
        nfast += f; nslow += 1 - f; done += 1
    while done < NCASE:
        dt = rng.choice([torch.float32, torch.float16])
        E = 4 if dt == torch.float32 else 8
        es = 4 if dt == torch.float32 else 2
        cv = odd_cv(rng)
        C = E * cv
        if rng.random() < 0.7:
            k, s, p = 3, 2, 1
        else:
            k = rng.choice([1, 2, 3, 5])
            s = rng.choice([1, 2, 3])
            p = rng.randint(0, k // 2)
        hwmax = max(2, BUDGET // (C * es))
        H = dim(rng, max(2, k - 2 * p), min(600, hwmax // 2))
        W = dim(rng, max(2, k - 2 * p), max(2, min(600, hwmax // H)))
        N = rng.randint(1, max(1, min(4, BUDGET // (H * W * C * es))))
        f = maxpool_case(rng, dt, N, H, W, C, k, s, p, rng.random() < 0.25)
        nfast += f; nslow += 1 - f; done += 1
    say(f"SUMMARY maxpool cases {done} fast {nfast} generic {nslow} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ upsample_add
def stress_upsample(rng):
    t0 = time.time()
    done = 0
    while done < NCASE:
        dt = rng.choice([torch.float32, torch.float16])
        E, es = (4, 4) if dt == torch.float32 else (8, 2)
        C = E * odd_cv(rng, 300)
        r = rng.random()
        H, W = dim(rng, 1, 300), dim(rng, 1, 300)
        if r < 0.15:
            Ht, Wt = 1, 1
        elif r < 0.3:
            Ht, Wt = H, W
        elif r < 0.6:
            Ht, Wt = max(1, H // 2), max(1, W // 2)
        else:
            Ht, Wt = rng.randint(1, H), rng.randint(1, W)
        while H * W * C * es > BUDGET:
            H, W = max(1, H // 2), max(1, W // 2)
            Ht, Wt = min(Ht, H), min(Wt, W)
        N = rng.randint(1, max(1, min(3, BUDGET // (H * W * C * es))))
        desc = f"{str(dt)[6:]} N{N} H{H} W{W} Ht{Ht} Wt{Wt} C{C}"
        say("START upsample_add", desc)
        g = gen(rng)
        lat, top = rand((N, H, W, C), dt, g), rand((N, Ht, Wt, C), dt, g)
        fn = lib.seam_upsample_add_f32 if dt == torch.float32 else lib.seam_upsample_add_f16

        def launch(y):
            y.copy_(lat)
            return fn(P(y), P(top), N, H, W, Ht, Wt, C, st())
        y = twice(launch, (N, H, W, C), dt, "upsample_add", desc)
        done += 1
        if y is None:
            continue
        # one fp32 sum, one rounding to the tensor's dtype (fp16 values add exactly in fp32 up to that rounding)
        up = F.interpolate(top.float().permute(0, 3, 1, 2), size=(H, W), mode="nearest").permute(0, 2, 3, 1)
        ref = (lat.float() + up).to(dt)
        if not torch.equal(y, ref):
            fail("upsample_add", desc, f"{int((y != ref).sum())} outputs differ")
    say(f"SUMMARY upsample_add cases {done} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ avgpool
def stress_avgpool(rng):
    t0 = time.time()
    done = 0
    while done < NCASE:
        dt = rng.choice([torch.float32, torch.float16])
        es = 4 if dt == torch.float32 else 2
        C = rng.choice([rng.randint(1, 64), 4 * rng.randint(1, 64), 8 * rng.randint(1, 128), 1024, 2048])
        L = rng.choice([1, 4, 7, 9, 36, 49, 196, rng.randint(1, 3000)])
        K = rng.choice([1, 2, rng.randint(1, 5000)])
        while K * L * C * es > BUDGET:
            K = max(1, K // 2) if K > 1 else K
            if K == 1 and L * C * es > BUDGET:
                L //= 2
        off = rng.choice([0, 0, 0, 1])        # an unaligned view: the scalar kernel
        desc = f"{str(dt)[6:]} K{K} L{L} C{C} off{off}"
        say("START avgpool", desc)
        g = gen(rng)
        flat = rand((K * L * C + off,), dt, g)
        x = flat[off:]
        fn = lib.seam_avgpool_f32 if dt == torch.float32 else lib.seam_avgpool_f16
        y = twice(lambda y: fn(P(x), P(y), K, L, C, st()), (K, C), dt, "avgpool", desc)
        done += 1
        if y is None:
            continue
        xd = x.view(K, L, C).double()
        ref = xd.mean(1)
        tol = L * 2.0 ** -24 * xd.abs().amax(1) + 1e-30
        if dt == torch.float16:
            mag = torch.maximum(ref.abs(), y.double().abs()).clamp(min=2.0 ** -14)
            tol = tol + 0.5 * 2.0 ** (torch.floor(torch.log2(mag)) - 10)
        err = (y.double() - ref).abs()
        if not bool((err <= tol).all()):
            fail("avgpool", desc, f"max err {float(err.max()):.3e} over tol")
    say(f"SUMMARY avgpool cases {done} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ layout bridges
def stress_transpose(rng):
    t0 = time.time()
    done = 0
    kinds = [("nchw_to_nhwc_f32", torch.float32, torch.float32, 0), ("nchw_f32_to_nhwc_f16", torch.float32, torch.float16, 0),
             ("nhwc_to_nchw_f32", torch.float32, torch.float32, 1), ("nhwc_f16_to_nchw_f32", torch.float16, torch.float32, 1)]
    while done < NCASE:
        name, ti, to, back = kinds[done % 4]
        B = rng.randint(1, 6)
        C = rng.choice([1, 3, 5, 7, 13, 31, 33, 64, 255, 256, rng.randint(1, 2100)])
        L = rng.choice([1, 2, 31, 33, 49, 196, rng.randint(1, 20000)])
        while B * C * L * 4 > BUDGET:
            L = max(1, L // 2)
        desc = f"{name} B{B} C{C} L{L}"
        say("START transpose", desc)
        g = gen(rng)
        fn = getattr(lib, "seam_" + name)
        if back == 0:
            x = rand((B, C, L), ti, g)
            y = twice(lambda y: fn(P(x), P(y), B, C, L, st()), (B, L, C), to, "transpose", desc)
            ref = x.permute(0, 2, 1).to(to)
        else:
            x = rand((B, L, C), ti, g)
            y = twice(lambda y: fn(P(x), P(y), B, L, C, st()), (B, C, L), to, "transpose", desc)
            ref = x.permute(0, 2, 1).to(to)
        done += 1
        if y is not None and not torch.equal(y, ref):
            fail("transpose", desc, f"{int((y != ref).sum())} elements differ")
    say(f"SUMMARY transpose cases {done} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ RoIAlign
BOUNDARY = [112.0, 224.0, 448.0]
ROI_ERR = [0.0]            # largest fp32 |error| / max|feature| seen (reported in the SUMMARY line)


def ulps(v, k):
    v = torch.tensor(v, dtype=torch.float32)
    for _ in range(abs(k)):
        v = torch.nextafter(v, torch.tensor(1e9 if k > 0 else 0.0))
    return float(v)


def boundary_box(rng, side):
    """A square box whose side sits on a LevelMapper boundary: the nominal size (112 / 224 / 448) and one fp32 ulp either side,
    or the real threshold the + 1e-6 of floor(4 + log2(s / 224) + 1e-6) moves it to, s * 2^-1e-6 (several ulps lower), and
    up to two ulps either side of that.  The device's level must equal map_levels' on the same fp32 box."""
    t = side * 2.0 ** -1e-6 if rng.random() < 0.6 else side
    v = ulps(t, rng.choice([-2, -1, 0, 0, 1, 2]))
    return [0.0, 0.0, v, v]


def random_box(rng, Himg, Wimg):
    r = rng.random()
    if r < 0.1:                                            # zero-size
        x, y = rng.uniform(-20, Wimg + 20), rng.uniform(-20, Himg + 20)
        return [x, y, x, y]
    if r < 0.2:                                            # sub-pixel
        x, y = rng.uniform(0, Wimg), rng.uniform(0, Himg)
        return [x, y, x + rng.uniform(0, 0.9), y + rng.uniform(0, 0.9)]
    if r < 0.4:                                            # off an edge
        x1, y1 = rng.uniform(-0.5 * Wimg, Wimg * 1.2), rng.uniform(-0.5 * Himg, Himg * 1.2)
        return [x1, y1, x1 + rng.uniform(1, Wimg), y1 + rng.uniform(1, Himg)]
    if r < 0.5:                                            # wider than the whole map
        return [rng.uniform(-50, 0), rng.uniform(-50, 0), Wimg + rng.uniform(0, 80), Himg + rng.uniform(0, 80)]
    x1, y1 = rng.uniform(0, Wimg - 1), rng.uniform(0, Himg - 1)
    return [x1, y1, rng.uniform(x1, Wimg), rng.uniform(y1, Himg)]


def roi_case(rng, dt, N, Himg, Wimg, C, K, Pp, sr, explicit, name="roi_align", big=False):
    es = 4 if dt == torch.float32 else 2
    g = gen(rng)
    hws = [(-(-Himg // s), -(-Wimg // s)) for s in (4, 8, 16, 32)]
    scales = [OD.infer_scales([hw], [(Himg, Wimg)])[0] for hw in hws]
    if big:
        # level 0 past 2^31 bytes: only the last image is filled (the others stay uninitialised -- never read)
        feats = [torch.empty((N,) + hw + (C,), dtype=dt, device=dev) for hw in hws]
        for f in feats:
            f[-1].copy_(rand(f.shape[1:], dt, g))
    else:
        feats = [rand((N,) + hw + (C,), dt, g) for hw in hws]
    boxes = []
    for i in range(K):
        if i < len(BOUNDARY) * 2 and not big:
            boxes.append([float(v) for v in boundary_box(rng, BOUNDARY[i % 3])])
        else:
            boxes.append(random_box(rng, Himg, Wimg))
    bidx = [N - 1 if big else rng.randrange(N) for _ in range(K)]
    rois = torch.tensor([[float(b)] + bx for b, bx in zip(bidx, boxes)], dtype=torch.float32)
    lv = OD.map_levels(rois[:, 1:], 2, 5)
    if explicit:
        lv = torch.tensor([rng.randrange(4) for _ in range(K)]) if not big else torch.zeros(K, dtype=torch.int64)
    desc = (f"{str(dt)[6:]} N{N} img{Himg}x{Wimg} C{C} K{K} P{Pp} sr{sr} levels{'explicit' if explicit else 'mapped'}"
            + (f" level0-bytes {feats[0].numel() * es}" if big else ""))
    say("START", name, desc)
    rd = rois.to(dev)
    ld = lv.to(torch.int32).to(dev) if explicit else None
    hw = (__import__("ctypes").c_int * 8)(*[d for f in feats for d in (f.shape[1], f.shape[2])])
    fn = lib.seam_roi_align_f32 if dt == torch.float32 else lib.seam_roi_align_f16
    outs = []
    for mode in (2, 1, 0):
        lib.seam_roi_align_set_lds(mode)
        y = twice(lambda y: fn(P(feats[0]), P(feats[1]), P(feats[2]), P(feats[3]), hw, C, *scales, 2, P(rd), P(ld), P(y), K, Pp, sr, st()),
                  (K, Pp, Pp, C), dt, name, desc + f" lds{mode}")
        if y is None:
            lib.seam_roi_align_set_lds(2)
            return
        outs.append(y)
    lib.seam_roi_align_set_lds(2)
    for m, y in zip((1, 0), outs[1:]):
        if not torch.equal(y, outs[0]):
            fail(name, desc, f"lds mode {m} differs from mode 2")
    if not explicit:
        # the device's LevelMapper against map_levels on the same fp32 boxes, directly: the mapped launch and a launch with
        # map_levels' levels passed in must give the same bits, ROI by ROI
        lvd = lv.to(torch.int32).to(dev)
        y2 = twice(lambda y: fn(P(feats[0]), P(feats[1]), P(feats[2]), P(feats[3]), hw, C, *scales, 2, P(rd), P(lvd), P(y), K, Pp, sr, st()),
                   (K, Pp, Pp, C), dt, name, desc + " map_levels")
        if y2 is None:
            return
        for i in range(K):
            if not torch.equal(y2[i], outs[0][i]):
                fail(name, desc, f"roi {i} box {boxes[i]}: the device's level differs from map_levels' {int(lv[i])}")
                return
    y = outs[0].double().cpu()
    # reference: sample coordinates in fp32 exactly as the oracle, values accumulated in fp64 (fp16: on the fp16 feature values)
    for i in range(K):
        l = int(lv[i])
        f = feats[l][bidx[i]:bidx[i] + 1].permute(0, 3, 1, 2).double().cpu()
        r = rois[i:i + 1].clone()
        r[0, 0] = 0.0
        ref = OD.roi_align(f, r, scales[l], Pp, sr)[0].permute(1, 2, 0)
        # fp32: the kernel forms the sample positions with fused multiply-adds (seam_roialign.hip: y1 + ph * bh + ...), so a
        # position may sit an ulp or two (2^-23 x up to max(H, W)) away from the oracle's; the bilinear weights move by as much,
        # times a value difference <= 2 max|v|.  The largest error / scale the sweep meets is printed in its SUMMARY line.
        # fp16: plus one fp16 ulp
        amax = float(f.abs().max())
        hl, wl = f.shape[-2:]
        tol = (1e-6 + 2.0 ** -21 * max(hl, wl)) * amax      # two fp32 ulps of a position (< max(H, W)) times a slope <= 2 max|v|
        if dt == torch.float16:
            mag = torch.maximum(ref.abs(), y[i].abs()).clamp(min=2.0 ** -14)
            tol = tol + 2.0 ** (torch.floor(torch.log2(mag)) - 10)
        err = (y[i] - ref).abs()
        if dt == torch.float32 and amax > 0:
            ROI_ERR[0] = max(ROI_ERR[0], float(err.max()) / amax)
        if not bool((err <= tol).all()):
            fail(name, desc, f"roi {i} box {boxes[i]} level {l}: max err {float(err.max()):.3e} amax {amax:.3f}")
            return


def stress_roi(rng):
    t0 = time.time()
    done = 0
    # one ROI past byte 2^31 of its level map (fp32 level 0: 60 x 200 x 200 x 256 x 4 B = 2.46 GB; the ROI is in image 59)
    roi_case(rng, torch.float32, 60, 800, 800, 256, 8, 7, 2, True, big=True)
    done += 1
    torch.cuda.empty_cache()
    while done < NCASE:
        dt = rng.choice([torch.float32, torch.float16])
        es = 4 if dt == torch.float32 else 2
        C = rng.choice([64, 128, 256, 4 * rng.randint(1, 40), 64 * rng.randint(1, 6)])
        Himg, Wimg = rng.randint(32, 400), rng.randint(32, 400)
        if rng.random() < 0.2:
            Himg, Wimg = 800, 800
        N = rng.randint(1, 3)
        while N * (Himg // 4 + 1) * (Wimg // 4 + 1) * C * es > BUDGET:
            Himg, Wimg = Himg * 3 // 4, Wimg * 3 // 4
        Pp = rng.choice([1, 2, 3, 7, 7, 14, 14, 16, rng.randint(1, 16)])
        sr = rng.choice([2, 2, 1, 3, 4])
        K = rng.randint(6, 24)
        roi_case(rng, dt, N, Himg, Wimg, C, K, Pp, sr, rng.random() < 0.3)
        done += 1
    say(f"SUMMARY roi_align cases {done} f32-max-err/scale {ROI_ERR[0]:.2e} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ preprocess
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def axis(n_in, n_out):
    """bilinear_axis() of seam_elementwise.hip, replayed: ATen's align_corners=False source index, scale = in / out rounded to
    fp32, src = fma(scale, dst + 0.5, -0.5) with ONE rounding (the kernel's v_pk_fma_f32; exact in fp64, then rounded), clamp."""
    scale = torch.tensor(n_in, dtype=torch.float32) / torch.tensor(n_out, dtype=torch.float32)
    d = torch.arange(n_out, dtype=torch.float64)
    src = (scale.double() * (d + 0.5) - 0.5).float().clamp(min=0.0)
    i = src.to(torch.int64).clamp(max=n_in - 1)
    i1 = torch.where(i < n_in - 1, i + 1, i)
    l = (src - i.float()).clamp(0.0, 1.0)
    return i, i1, l, 1.0 - l


def pre_ref(img, out_h, out_w, Hp, Wp):
    """img fp64 [3, in_h, in_w] (already in [0, 1]) -> fp64 [Hp, Wp, 3]: normalise, resize (fp32 weights, fp64 values), pad 0"""
    _, in_h, in_w = img.shape
    v = (img - torch.tensor([float(torch.tensor(m, dtype=torch.float32)) for m in MEAN], dtype=torch.float64)[:, None, None]) \
        / torch.tensor([float(torch.tensor(sd, dtype=torch.float32)) for sd in STD], dtype=torch.float64)[:, None, None]
    if (out_h, out_w) != (in_h, in_w):
        y0, y1, ly, hy = axis(in_h, out_h)
        x0, x1, lx, hx = axis(in_w, out_w)
        ly, hy, lx, hx = (t.double() for t in (ly, hy, lx, hx))
        r0, r1 = v[:, y0], v[:, y1]
        v = hy[None, :, None] * (hx * r0[:, :, x0] + lx * r0[:, :, x1]) + ly[None, :, None] * (hx * r1[:, :, x0] + lx * r1[:, :, x1])
    out = torch.zeros((Hp, Wp, 3), dtype=torch.float64)
    out[:out_h, :out_w] = v.permute(1, 2, 0)
    return out


def pre_check(name, desc, y, ref, dt):
    """y: the kernel's output as fp64, same layout as ref; spare channels / pad cells are exact zeros in ref"""
    tol = 1e-6 * 2.7                                        # 1e-6 of the normalised range (|v| <= (1 - 0.406) / 0.225 < 2.7)
    if dt == torch.float16:
        tol = tol + 0.5 * 2.0 ** (torch.floor(torch.log2(torch.maximum(ref.abs(), y.abs()).clamp(min=2.0 ** -14))) - 10)
    zero = ref == 0
    if not torch.equal(y[zero], ref[zero]):
        fail(name, desc, f"{int((y[zero] != 0).sum())} pad / spare-channel values not 0")
        return
    err = (y - ref).abs()
    if not bool((err <= tol).all()):
        fail(name, desc, f"max err {float(err.max()):.3e}")


def s2d(ref, lo, hi, ch):
    """[n, Hp, Wp, 3] -> [n, Hp/2 + lo + hi, Wp/2 + lo + hi, ch], channel (dy * 2 + dx) * 3 + c, zeros elsewhere"""
    n, Hp, Wp, _ = ref.shape
    cells = ref.view(n, Hp // 2, 2, Wp // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, Hp // 2, Wp // 2, 12)
    out = torch.zeros((n, Hp // 2 + lo + hi, Wp // 2 + lo + hi, ch), dtype=torch.float64)
    out[:, lo:lo + Hp // 2, lo:lo + Wp // 2, :12] = cells
    return out


def stress_preprocess(rng):
    t0 = time.time()
    done = 0
    kinds = ["single", "batch", "s2d", "s2d_pad", "u8"]
    while done < NCASE:
        kind = kinds[done % 5]
        dt = torch.float32 if kind == "s2d" and done % 10 < 5 else rng.choice([torch.float32, torch.float16])
        if kind == "s2d_pad":
            dt = torch.float16
        in_h, in_w = dim(rng, 1, 700), dim(rng, 1, 700)
        r = rng.random()
        if r < 0.25:
            out_h, out_w = in_h, in_w                             # identity size
        elif r < 0.5:
            out_h, out_w = rng.randint(in_h, min(4 * in_h, 900)), rng.randint(in_w, min(4 * in_w, 900))   # up-scale
        elif r < 0.75:
            out_h, out_w = rng.randint(1, in_h), rng.randint(1, in_w)                                     # down-scale
        else:
            out_h, out_w = dim(rng, 1, 900), dim(rng, 1, 900)
        extra = rng.choice([0, 0, 1, 7, 32, rng.randint(0, 600)])  # Hp / Wp >> the frame now and then
        Hp, Wp = out_h + rng.choice([0, extra]), out_w + rng.choice([0, extra])
        if kind.startswith("s2d"):
            Hp, Wp = Hp + (Hp & 1), Wp + (Wp & 1)
        while Hp * Wp * 16 > BUDGET:
            out_h, out_w, Hp, Wp = max(1, out_h // 2), max(1, out_w // 2), Hp // 2, Wp // 2
            Hp, Wp = max(Hp, out_h), max(Wp, out_w)
            if kind.startswith("s2d"):
                Hp, Wp = Hp + (Hp & 1), Wp + (Wp & 1)
        n = rng.randint(1, 3) if kind in ("batch", "s2d", "s2d_pad") else 1
        lo, hi = (rng.randint(0, 3), rng.randint(0, 3)) if kind == "s2d_pad" else (0, 0)
        desc = f"{kind} {str(dt)[6:]} n{n} in{in_h}x{in_w} out{out_h}x{out_w} pad{Hp}x{Wp} cells{lo}/{hi}"
        say("START preprocess", desc)
        g = gen(rng)
        if kind == "u8":
            img8 = torch.randint(0, 256, (in_h, in_w, 3), dtype=torch.uint8, device=dev, generator=g)
            imgs = img8.permute(2, 0, 1)[None].double().cpu() / 255.0
        else:
            stride = 3 * in_h * in_w + rng.choice([0, 0, 2, 5])   # batch images need not be packed
            flat = torch.rand((n * stride,), device=dev, generator=g)
            img = flat
            imgs = torch.stack([flat[k * stride:k * stride + 3 * in_h * in_w].view(3, in_h, in_w) for k in range(n)]).double().cpu()
        ref = torch.stack([pre_ref(imgs[k], out_h, out_w, Hp, Wp) for k in range(n)])
        E = 4 if dt == torch.float32 else 8
        f16 = dt == torch.float16
        if kind in ("single", "u8", "batch"):
            shape = (n, Hp, Wp, E)
            if kind == "single":
                fn = lib.seam_preprocess_f16 if f16 else lib.seam_preprocess_f32
                launch = lambda y: fn(P(img), P(y), in_h, in_w, out_h, out_w, Hp, Wp, st())
            elif kind == "u8":
                launch = lambda y: lib.seam_preprocess_u8(P(img8), P(y), in_h, in_w, out_h, out_w, Hp, Wp, int(f16), st())
            else:
                fn = lib.seam_preprocess_batch_f16 if f16 else lib.seam_preprocess_batch_f32
                launch = lambda y: fn(P(img), stride, P(y), n, in_h, in_w, out_h, out_w, Hp, Wp, st())
            full = torch.zeros(shape, dtype=torch.float64)
            full[..., :3] = ref
        else:
            ch = 16 if f16 else 12
            shape = (n, Hp // 2 + lo + hi, Wp // 2 + lo + hi, ch)
            if kind == "s2d":
                fn = lib.seam_preprocess_s2d_batch_f16 if f16 else lib.seam_preprocess_s2d_batch_f32
                launch = lambda y: fn(P(img), stride, P(y), n, in_h, in_w, out_h, out_w, Hp, Wp, st())
            else:
                launch = lambda y: lib.seam_preprocess_s2d_pad_batch_f16(P(img), stride, P(y), n, in_h, in_w, out_h, out_w, Hp, Wp,
                                                                        lo, hi, st())
            full = s2d(ref, lo, hi, ch)
        y = twice(launch, shape, dt, "preprocess", desc)
        done += 1
        if y is not None:
            pre_check("preprocess", desc, y.double().cpu(), full, dt)
    say(f"SUMMARY preprocess cases {done} seconds {time.time() - t0:.1f}")


FAMILIES = [("maxpool", stress_maxpool), ("upsample_add", stress_upsample), ("avgpool", stress_avgpool),
            ("transpose", stress_transpose), ("roi_align", stress_roi), ("preprocess", stress_preprocess)]


def main(argv):
    global NCASE, SEED, OD, _native, dev, lib, ops
    sys.path.insert(0, ROOT)
    import seam_match_rcnn_amd.ops as ops
    from seam_match_rcnn_amd import _native
    from oracle import detection as OD
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
