"""Plain float64 restatements of the match-head and ranking kernels (``csrc/seam_heads.hip``, ``seam_topk.h``,
``seam_pairmf.hip``, ``seam_narrow.hip``), the error bounds the GPU sweep (``test_gpu_stress_heads.py``) holds them to, the
comparators it uses and its seeded case generators.  Device-agnostic: everything runs where its tensors live, so
``test_heads_references.py`` ties the references to ``oracle/heads.py`` / ``oracle/evaluator.py`` / ``heads_golden.npz`` on the
CPU, proves that every comparator rejects a planted error, and proves that no tolerance is tighter than fp32 itself (the fp32
oracle, a different summation order from any kernel, must pass every continuous case of the sweep).

Bounds.  Sums use ``train_refs.bound(maj, L) = C_ERR * 2^-24 * L * sum|terms|`` with the chain length L given where it is used.

Scores ``e1 / (e0 + e1)`` with ``e_i = expf(x_i - max(x0, x1))``: one exponential is exactly 1, the other is ``e = exp(t)``,
``t = fl(x_lo - x_hi)``.  The rounding of t (relative u = 2^-24) moves e by ``|t| u`` relative; expf is taken as 1 ulp
(<= 2 u relative; the ROCm installation carries no accuracy table for the device math library, so the bound is derived from a
1-ulp expf and a correctly rounded division, which is what hipcc's default fp32 division is); the sum ``1 + e`` and the division
round once each.  For x1 < x0 the score is ``e / (1 + e)``: relative error ``(|t| + 2) u (1 - e / (1 + e)) + 2 u <= (|t| + 4) u``;
for x1 >= x0 it is ``1 / (1 + e)``: ``2 u + e (|t| + 2) u / (1 + e) <= 3.3 u``.  SCORE_C = 6 = 4 + 2 (second-order terms and the
rounding of |t| itself), so a score is allowed ``(|d| + 6) * 2^-24 * ref + FLT_MIN`` (d = x1 - x0; the absolute term covers a
flushed or denormal exponential).  Where the score is not 0, |d| < 104, so the relative part stays below 7e-6: far inside
what ``test_gpu_ops.assert_close`` allows at its defaults (1e-3 relative).

Non-local block + attention pooling, stage by stage (``nlb_attnpool64``; |.| elementwise, every majorant the same expression
over absolute values):
  a, b    L = 266: 256 fma + bias, the product with wc, a 6-level wave tree, the add of the two wave halves (VALU form: 265).
          The MFMA form folds theta / phi into u = fl(W_theta^T wc[:128]) (one rounding per element of u, majorant
          |X| |W_theta|^T |wc[:128]|, the same expression) and sums 4 products per lane + the tree + the constant: 12 <= 266
  G       L = 257: 256 fma (32x32x2 MFMA: 2 roundings per instruction, 128 instructions) + bias
  f       (da_i + db_j) / T + bound((|a_i| + |b_j|) / T, 3): the add, and the division by T or the rounded 1/T and its product;
          ReLU is 1-Lipschitz
  Y       df |G| + f dG + bound(f |G|, T + 1)
  Z       dY |Ww|^T + bound(|Y| |Ww|^T + |bw| + |X|, 130): 128 fma, the bias, the residual
          The stages up to here are worst-case bounds stacked four deep (every majorant sums absolute values, every chain is
          taken at full length), and the result is some 3e4 times what fp32 does: it could not tell 1/T from 1/(T+1) beyond
          T = 17.  So this constant is MEASURED instead, on the CPU: the fp32 evaluation of ``oracle.heads`` against this float64
          reference over all 100 cases of the sweep is at most 3.44e-5 of the propagated bound on Z
          (``test_heads_references.test_tolerance_nlb`` repeats the measurement); the kernels are allowed 4 x that ratio
          (their summation order, FMA use and expf differ from torch's): dZ = NLB_BLOCK_RHO x the expression above,
          NLB_BLOCK_RHO = 4 x 3.44e-5 = 1.376e-4.  Never calibrated on a kernel's output.  The stages below are derived on top of this dZ.
  s       dZ |wa| + bound(|Z| |wa| + |ba|, 12): product(s), the lane tree, the 4 wave partials and the bias
  p       att_ref * (expm1(2 max_t ds_t) + c_soft * 2^-24), c_soft = C_ERR * (2 (R + 3) + T + 3 ceil(T / 16) + 2): R = spread of
          the scores (the rounded argument s_t - m moves each exponential by |s_t - m| u, expf adds 2 u; numerator and
          denominator each), T additions of the denominator, 3 roundings per chunk of the online rescaling, the division
  out     sum_t (dp_t |Z_t| + p_t dZ_t) + bound(sum_t p_t |Z_t|, T + 2)
"""
import math
import random

import numpy as np
import torch
import torch.nn.functional as F

import seam_match_rcnn_amd.synth as synth
import train_refs as TR

U = TR.U
F64, F32 = torch.float64, torch.float32
FLT_MIN = 2.0 ** -126
SCORE_C = 6.0
TOPK_CAP = 256
NLB_BLOCK_RHO = 1.376e-4         # measured constant of the block's propagated bound on Z (module docstring)
SEED = 29                       # the sweep's seed; family i draws from random.Random(SEED * 7919 + i)
FAMILIES = ["pair_logits", "rank", "pair_topk", "pair_topk_mfma", "blockdiag", "score_reduce", "nlb", "linear_narrow"]


def family_rng(name):
    return random.Random(SEED * 7919 + FAMILIES.index(name))


# ------------------------------------------------------------------------------------------------ ranking
def rank_key(d):
    """The evaluator's sort key on the logit difference: NaN as -inf, -0 as +0."""
    d = d.to(F64)
    d = torch.where(torch.isnan(d), torch.full_like(d, -math.inf), d)
    return d + 0.0


def rank_order(d, k):
    """d [..., G] -> the first k indices in descending d, lower index first on equal d, NaN last."""
    return torch.argsort(-rank_key(d), dim=-1, stable=True)[..., :k]


def rank_of(d, target):
    """d [Q,G], target [Q] -> the number of entries ranked before the target (the count form of ``rank_order``); a target
    outside [0, G) gives -1."""
    key = rank_key(d)
    g = key.shape[1]
    t = target.to(torch.int64)
    valid = (t >= 0) & (t < g)
    tc = t.clamp(0, max(g - 1, 0))[:, None]
    kt = key.gather(1, tc)
    ar = torch.arange(g, device=key.device)[None, :]
    cnt = ((key > kt) | ((key == kt) & (ar < tc))).sum(1)
    return torch.where(valid, cnt, torch.full_like(cnt, -1))


def position_in_order(order, target):
    """Position of target[q] in the full permutation order[q] (-1 for a target outside it)."""
    q, g = order.shape
    inv = torch.empty_like(order)
    inv.scatter_(1, order, torch.arange(g, device=order.device)[None, :].expand(q, g).contiguous())
    t = target.to(torch.int64)
    valid = (t >= 0) & (t < g)
    pos = inv.gather(1, t.clamp(0, g - 1)[:, None])[:, 0]
    return torch.where(valid, pos, torch.full_like(pos, -1))


def score64(logits):
    """softmax(x)[..., 1] of [..., 2] in float64, in the max-shifted form (an infinite maximum gives NaN, as fp32 does)."""
    x = logits.to(F64)
    mx = torch.fmax(x[..., 0], x[..., 1])
    e0, e1 = torch.exp(x[..., 0] - mx), torch.exp(x[..., 1] - mx)
    return e1 / (e0 + e1)


def score_tol(logits, ref):
    """(|d| + SCORE_C) * 2^-24 * ref + FLT_MIN on the logits the score was computed from (module docstring)."""
    x = logits.to(F64)
    d = (x[..., 1] - x[..., 0]).abs()
    d = torch.where(torch.isfinite(d), d, torch.zeros_like(d))
    r = torch.where(torch.isfinite(ref), ref, torch.zeros_like(ref))
    return (d + SCORE_C) * U * r + FLT_MIN


# ------------------------------------------------------------------------------------------------ pairwise classifier
def pair_logits64(a, b, w, bias):
    """x[i,j,:] = W (a_i - b_j)^2 + bias in float64 and the majorant sum_k |w_k| (a - b)^2 + |bias| -> ([Q,G,2], [Q,G,2])."""
    a, b, w, bias = a.to(F64), b.to(F64), w.to(F64), bias.to(F64)
    q, g, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty((q, g, 2), dtype=F64, device=a.device)
    maj = torch.empty((q, g, 2), dtype=F64, device=a.device)
    step = max(1, (1 << 24) // max(1, g * d))
    for s in range(0, q, step):
        d2 = (a[s:s + step, None, :] - b[None, :, :]) ** 2
        for c in range(2):                       # elementwise products: 0 * inf is NaN here as in the kernel's fma
            out[s:s + step, :, c] = (d2 * w[c]).sum(-1) + bias[c]
            maj[s:s + step, :, c] = (d2 * w[c].abs()).sum(-1) + bias[c].abs()
    return out, maj


def blockdiag64(x, seg, w, bias):
    """Per group s of rows [seg[s], seg[s+1]): the n_s x n_s scores, flattened and concatenated; also the float64 logits."""
    outs, lgs = [], []
    for s in range(len(seg) - 1):
        xs = x[seg[s]:seg[s + 1]]
        lg, _ = pair_logits64(xs, xs, w, bias)
        lgs.append(lg.reshape(-1, 2))
        outs.append(score64(lg).reshape(-1))
    if not outs:
        return torch.empty((0,), dtype=F64, device=x.device), torch.empty((0, 2), dtype=F64, device=x.device)
    return torch.cat(outs), torch.cat(lgs)


def score_reduce64(score, mode):
    """score [n,G] -> column mean (mode 0) or max (mode 1) with the kernel's documented edge behaviour: no rows gives NaN / -inf,
    a NaN poisons the mean and is ignored by the max (all NaN: -inf)."""
    s = score.to(F64)
    if mode == 0:
        return s.sum(0) / s.shape[0] if s.shape[0] else torch.full((s.shape[1],), math.nan, dtype=F64, device=s.device)
    neg = torch.full((1, s.shape[1]), -math.inf, dtype=F64, device=s.device)
    return torch.cat([neg, torch.where(torch.isnan(s), neg.expand_as(s), s)]).max(0).values


def linear_narrow64(x, w, bias, relu):
    """y = act(x w^T + bias) in float64 and the majorant |x| |w|^T + |bias|."""
    x, w = x.to(F64), w.to(F64)
    y = x @ w.t()
    maj = x.abs() @ w.abs().t()
    if bias is not None:
        y, maj = y + bias.to(F64), maj + bias.to(F64).abs()
    return (F.relu(y) if relu else y), maj


# ------------------------------------------------------------------------------------------------ NLB + attention pooling
def nlb_applies(use_nlb, t):
    return use_nlb == 2 or (use_nlb == 1 and t > 1)


def nlb_attnpool64(seqs, p, use_nlb, _inv_t=None, _softmax_rows=None):
    """seqs = list of [T_s,256] (T_s >= 1), p as ``train_refs.nlb_params`` gives it -> list of dicts out [256], att [T], z [T,256]
    in float64 with the propagated elementwise bounds d_out, d_att, d_z (module docstring).
    _inv_t(T) / _softmax_rows(T): the planted errors of the teeth tests (another 1/T; only the first rows enter the softmax)."""
    bd = TR.bound
    wth, bth = p["newnlb.theta.weight"][:, :, 0], p["newnlb.theta.bias"]
    wph, bph = p["newnlb.phi.weight"][:, :, 0], p["newnlb.phi.bias"]
    wg, bg = p["newnlb.g.weight"][:, :, 0], p["newnlb.g.bias"]
    wc = p["newnlb.concat_project.0.weight"].reshape(-1)
    wo, bo = p["newnlb.W.weight"][:, :, 0], p["newnlb.W.bias"]
    wa, ba = p["attention_scorer.weight"].reshape(-1), p["attention_scorer.bias"].reshape(())
    res = []
    for x in seqs:
        x = x.to(F64)
        t = x.shape[0]
        ax = x.abs()
        if nlb_applies(use_nlb, t):
            a = (x @ wth.t() + bth) @ wc[:128]
            b = (x @ wph.t() + bph) @ wc[128:]
            g = x @ wg.t() + bg
            da = bd((ax @ wth.abs().t() + bth.abs()) @ wc[:128].abs(), 266)
            db = bd((ax @ wph.abs().t() + bph.abs()) @ wc[128:].abs(), 266)
            dg = bd(ax @ wg.abs().t() + bg.abs(), 257)
            inv_t = 1.0 / t if _inv_t is None else _inv_t(t)
            f = F.relu(a[:, None] + b[None, :]) * inv_t
            df = (da[:, None] + db[None, :]) / t + bd((a.abs()[:, None] + b.abs()[None, :]) / t, 3)
            y = f @ g
            dy = df @ g.abs() + f @ dg + bd(f @ g.abs(), t + 1)
            z = y @ wo.t() + bo + x
            dz = NLB_BLOCK_RHO * (dy @ wo.abs().t() + bd(y.abs() @ wo.abs().t() + bo.abs() + ax, 130))
        else:
            z, dz = x, torch.zeros_like(x)
        s = z @ wa + ba
        ds = dz @ wa.abs() + bd(z.abs() @ wa.abs() + ba.abs(), 12)
        n = t if _softmax_rows is None else _softmax_rows(t)
        att = torch.zeros_like(s)
        att[:n] = torch.softmax(s[:n], 0)
        spread = float(s.max() - s.min())
        c_soft = TR.C_ERR * (2 * (spread + 3) + t + 3 * math.ceil(t / 16) + 2)
        d_att = att * (math.expm1(2 * float(ds.max())) + c_soft * U)
        out = att @ z
        d_out = d_att @ z.abs() + att @ dz + bd(att @ z.abs(), t + 2)
        res.append(dict(out=out, att=att, z=z, d_out=d_out, d_att=d_att, d_z=dz))
    return res


# ------------------------------------------------------------------------------------------------ comparators
def cmp_index(got, ref):
    """Exact equality of integer results -> (ok, message)."""
    if got.shape != ref.shape:
        return False, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    bad = got.to(torch.int64) != ref.to(torch.int64)
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        return False, (f"{int(bad.sum())} of {bad.numel()} differ; first at flat {i}: got {int(got.reshape(-1)[i])} "
                       f"want {int(ref.reshape(-1)[i])}")
    return True, ""


def cmp_bounded(got, ref, tol):
    """|got - ref| <= tol elementwise; NaN must meet NaN, an infinity the same infinity (tol 0: bit-exact to the float64 value)
    -> (ok, message, worst err / tol over the elements with a positive tolerance)."""
    got, ref = got.to(F64), ref.to(F64)
    if got.shape != ref.shape:
        return False, f"shape {tuple(got.shape)} vs {tuple(ref.shape)}", math.inf
    tol = torch.as_tensor(tol, dtype=F64, device=got.device).expand_as(ref)
    both_nan = torch.isnan(got) & torch.isnan(ref)
    eq = got == ref
    err = torch.where(eq | both_nan, torch.zeros_like(ref), (got - ref).abs())
    bad = ~(eq | both_nan | (err <= tol))
    pos = (tol > 0) & torch.isfinite(tol) & torch.isfinite(err)
    worst = float((err[pos] / tol[pos]).max()) if bool(pos.any()) else 0.0
    if bool(bad.any()):
        i = int(bad.reshape(-1).nonzero()[0])
        return False, (f"{int(bad.sum())} of {bad.numel()} off; first at flat {i}: got {float(got.reshape(-1)[i])!r} "
                       f"want {float(ref.reshape(-1)[i])!r} tol {float(tol.reshape(-1)[i]):.3g}"), worst
    return True, "", worst


def holds_poison(t, poison):
    """Elementwise: does t still hold the poison value (NaN, a float or an integer pattern)?"""
    if isinstance(poison, float) and poison != poison:
        return torch.isnan(t)
    return t == poison


def cmp_untouched(t, written, poison):
    """Every element outside the boolean mask ``written`` (None: nothing may be written) still holds its poison -> (ok, message)."""
    keep = holds_poison(t, poison)
    bad = ~keep if written is None else (~keep & ~written)
    if bool(bad.any()):
        return False, f"{int(bad.sum())} elements outside the written region changed; first at flat {int(bad.reshape(-1).nonzero()[0])}"
    return True, ""


# ------------------------------------------------------------------------------------------------ data
class Pool:
    """One draw of ``synth.normal`` shared by every continuous case (slices at seeded offsets, wrapping)."""
    def __init__(self, dev, n=1 << 21):
        self.x = torch.from_numpy(synth.normal(synth.stream_id(SEED, "heads_pool"), (n,))).to(dev)
        self.n = n

    def take(self, rng, shape, scale=1.0):
        n = 1
        for d in shape:
            n *= d
        off = rng.randrange(self.n)
        idx = (torch.arange(n, device=self.x.device) + off) % self.n
        return (self.x[idx] * scale).reshape(shape).contiguous()


def ints(rng, shape, lo, hi, dev):
    """Seeded integers in [lo, hi] as fp32 (NumPy's generator: the same values on any device)."""
    r = np.random.RandomState(rng.randrange(1 << 31))
    return torch.from_numpy(r.randint(lo, hi + 1, size=tuple(shape)).astype(np.float32)).to(dev)


def head_weights(dev):
    """The synthetic head weights (``synth.temporal_aggregator_state``) in the kernels' layouts: pk = the flat NLB pack
    (``ops.PackedNLB`` fields), p = its float64 reference layout, last_w [2,256] / last_b [2] the pairwise classifier."""
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth.temporal_aggregator_state(12).items()}
    n = "newnlb."
    pk = dict(
        w_proj_t=torch.cat([sd[n + "theta.weight"][:, :, 0], sd[n + "phi.weight"][:, :, 0], sd[n + "g.weight"][:, :, 0]]).t(),
        b_proj=torch.cat([sd[n + "theta.bias"], sd[n + "phi.bias"], sd[n + "g.bias"]]),
        w_cat=sd[n + "concat_project.0.weight"].reshape(256), w_out_t=sd[n + "W.weight"][:, :, 0].t(), b_out=sd[n + "W.bias"],
        w_att=sd["attention_scorer.weight"].reshape(256), b_att=sd["attention_scorer.bias"].reshape(1))
    pk = {k: v.contiguous().to(dev) for k, v in pk.items()}
    return dict(pk=pk, p=TR.nlb_params(pk), sd={k: v.to(dev) for k, v in sd.items() if v.dtype == torch.float32},
                last_w=sd["last.weight"].contiguous().to(dev), last_b=sd["last.bias"].contiguous().to(dev))


def pair_weights(rng, cls, d, hw, dev):
    """(w [2,D], bias [2]): integers in [-4,4] / [-8,8] (class I) or the synthetic classifier's law (uniform +-sqrt(3/D); its
    own tensors at D = 256)."""
    if cls.startswith("I"):
        return ints(rng, (2, d), -4, 4, dev), ints(rng, (2,), -8, 8, dev)
    if d == 256:
        return hw["last_w"], hw["last_b"]
    b = math.sqrt(3.0 / d)
    w = torch.from_numpy(synth.uniform(synth.stream_id(SEED, f"last_w{d}"), (2, d), -b, b)).to(dev)
    return w, torch.from_numpy(synth.uniform(synth.stream_id(SEED, f"last_b{d}"), (2,), -1 / math.sqrt(d), 1 / math.sqrt(d))).to(dev)


def descriptors(rng, cls, shape, pool, dev):
    return ints(rng, shape, -3, 3, dev) if cls.startswith("I") else pool.take(rng, shape)


# ------------------------------------------------------------------------------------------------ case lists
def pair_logits_specs():
    rng = family_rng("pair_logits")
    ds, qs, gs = [32, 64, 96, 256, 1024], [1, 15, 16, 17, 31, 32, 33, 70], [1, 31, 32, 63, 64, 65, 127, 128, 129, 333]
    specs = []
    for i in range(100):
        q, g = (qs[i % 8], gs[(i // 8) % 10]) if i < 80 else (rng.choice(qs), rng.choice(gs))
        specs.append(dict(Q=q, G=g, D=ds[i % 5], cls="IC"[(i + i // 8) % 2]))
    # both sides of the tile switch at Q * G = 2^20, with full query tiles and with a one-row query tile
    specs += [dict(Q=128, G=8191, D=64, cls="I"), dict(Q=128, G=8192, D=64, cls="I"), dict(Q=128, G=8191, D=32, cls="C"),
              dict(Q=128, G=8192, D=32, cls="C"), dict(Q=1, G=(1 << 20) - 1, D=32, cls="I"), dict(Q=1, G=1 << 20, D=32, cls="I")]
    for s in specs:
        s["seed"] = rng.randrange(1 << 30)
    return specs


def pair_logits_make(s, pool, hw, dev):
    rng = random.Random(s["seed"])
    a = descriptors(rng, s["cls"], (s["Q"], s["D"]), pool, dev)
    b = descriptors(rng, s["cls"], (s["G"], s["D"]), pool, dev)
    w, bias = pair_weights(rng, s["cls"], s["D"], hw, dev)
    return a, b, w, bias


def rank_specs():
    rng = family_rng("rank")
    gs, qs = [1, 2, 255, 256, 257, 511, 513, 1000, 5000], [1, 3, 64]
    specs = []
    for i in range(108):
        g = gs[i % 9]
        ks = sorted({k for k in (1, 2, g, 255, 256) if 1 <= k <= min(g, TOPK_CAP)})
        specs.append(dict(G=g, Q=qs[(i // 9) % 3], k=ks[(i // 27 + i) % len(ks)], cls=["IS", "I", "C", "CS"][i % 4],
                          seed=rng.randrange(1 << 30)))
    return specs


def plant_specials(x, rng):
    """Class (S) into logits [Q,G,2]: NaN in x0 / x1 / both, +-inf, a -0.0 next to a +0.0 difference, constant and all-NaN rows."""
    q, g = x.shape[0], x.shape[1]
    nan, inf = math.nan, math.inf
    for r in range(q):
        u = rng.random()
        if u < 0.15:
            x[r, :, 0], x[r, :, 1] = 1.5, 2.5                      # a whole row constant: the order is the index order
            continue
        if u < 0.3:
            x[r] = nan                                               # a whole row NaN
            continue
        for v0, v1 in ((nan, None), (None, nan), (nan, nan), (None, inf), (None, -inf), (inf, None), (inf, inf), (-inf, -inf)):
            c = rng.randrange(g)
            if v0 is not None:
                x[r, c, 0] = v0
            if v1 is not None:
                x[r, c, 1] = v1
        c = rng.randrange(g)
        x[r, c, 0], x[r, c, 1] = 0.0, -0.0                          # d = -0.0 ...
        x[r, (c + 1) % g, 0], x[r, (c + 1) % g, 1] = 1.0, 1.0       # ... next to d = +0.0: they tie, lower index first
    return x


def rank_make(s, pool, dev):
    """-> logits [Q,G,2] and targets [Q] (0, G - 1, -1, G, then random ones)."""
    rng = random.Random(s["seed"])
    q, g = s["Q"], s["G"]
    x = ints(rng, (q, g, 2), -8, 8, dev) if s["cls"].startswith("I") else pool.take(rng, (q, g, 2), 3.0)
    if s["cls"].endswith("S"):
        x = plant_specials(x.cpu(), rng).to(dev)
    first = [0, g - 1, -1, g]
    rot = rng.randrange(4)
    tg = [first[(i + rot) % 4] if i < 4 else rng.randrange(g) for i in range(q)]
    return x.contiguous(), torch.tensor(tg, dtype=torch.int64, device=dev)


def pair_topk_specs():
    rng = family_rng("pair_topk")
    gs, ks, qs, ds = [1, 5, 255, 256, 257, 258, 300, 511, 513, 1030], [1, 2, 5, 64, 255, 256], [1, 31, 32, 33, 40], [32, 64, 256]
    specs = []
    for i in range(100):
        g = gs[i % 10]
        kk = [k for k in ks if k <= g]
        specs.append(dict(G=g, k=kk[(i // 10 + i) % len(kk)], Q=qs[(i // 10 + i) % 5], D=ds[(i // 5) % 3],
                          cls=["I", "C", "IS", "CS"][(i + i // 10) % 4], seed=rng.randrange(1 << 30)))
    # every difference of query 0 is -inf and every one of query 1 NaN, with a last segment of 2 / 1 columns: the placeholder
    # candidates (index -1) of the short segment must not displace real indices
    specs += [dict(G=258, k=5, Q=3, D=32, cls="IX", seed=rng.randrange(1 << 30)),
              dict(G=257, k=256, Q=3, D=32, cls="IX", seed=rng.randrange(1 << 30))]
    return specs


def pair_topk_make(s, pool, hw, dev):
    rng = random.Random(s["seed"])
    a, b, w, bias = pair_logits_make(dict(s, cls=s["cls"][0], seed=rng.randrange(1 << 30)), pool, hw, dev)
    a, b, w = a.clone(), b.clone(), w.clone()
    q, g, d = s["Q"], s["G"], s["D"]
    if s["cls"].endswith("S"):          # NaN / inf descriptor rows: whole queries and whole bank rows
        a[rng.randrange(q)] = math.nan
        b[rng.randrange(g)] = math.nan
        b[rng.randrange(g), rng.randrange(d)] = math.inf
        if q > 2:
            a[rng.randrange(q), rng.randrange(d)] = -math.inf
    if s["cls"].endswith("X"):
        w[0, 3], w[1, 3] = 1.0, -1.0
        a[0, 3] = math.inf              # x0 = +inf, x1 = -inf for every product
        a[1] = math.nan
    return a, b, w, bias


def pair_topk_mfma_specs():
    rng = family_rng("pair_topk_mfma")
    gs, qs, ks = [8192, 8193, 8447, 9001], [1, 33, 256, 257], [1, 20, 64]
    return [dict(G=gs[i % 4], Q=qs[(i // 4) % 4], k=ks[i % 3], flags=(i // 2) % 2, cls=["I", "C", "CN"][(i // 3) % 3],
                 seed=rng.randrange(1 << 30)) for i in range(16)]


def pair_topk_mfma_make(s, pool, hw, dev):
    rng = random.Random(s["seed"])
    a, b, w, bias = pair_logits_make(dict(s, D=256, cls=s["cls"][0], seed=rng.randrange(1 << 30)), pool, hw, dev)
    b = b.clone()
    if s["cls"] == "I":                 # duplicated bank rows: ties at every rank
        b[500:] = b[torch.arange(500, s["G"], device=dev) % 500]
    if s["cls"] == "CN":
        a = a.clone()
        b[rng.randrange(s["G"])] = math.nan
        b[rng.randrange(s["G"])] = math.nan
        if s["Q"] > 1:
            a[rng.randrange(s["Q"])] = math.nan
    return a, b, w, bias


def blockdiag_specs():
    rng = family_rng("blockdiag")
    sizes = [0, 1, 15, 16, 17, 63, 64, 65, 150]
    specs = []
    for i in range(100):
        n = [sizes[(i + j) % 9] for j in range(3)] + [rng.choice(sizes) for _ in range(rng.randint(0, 5))]
        rng.shuffle(n)
        specs.append(dict(n=n, D=[32, 256][i % 2], extra=[0, rng.randint(1, 40)][(i // 2) % 2], cls="IC"[(i // 4) % 2],
                          seed=rng.randrange(1 << 30)))
    return specs


def blockdiag_make(s, pool, hw, dev):
    rng = random.Random(s["seed"])
    x = descriptors(rng, s["cls"], (max(1, sum(s["n"])), s["D"]), pool, dev)
    w, bias = pair_weights(rng, s["cls"], s["D"], hw, dev)
    seg = [0]
    for n in s["n"]:
        seg.append(seg[-1] + n)
    return x, seg, w, bias


def score_reduce_specs():
    rng = family_rng("score_reduce")
    ns, gs, ps = [1, 2, 7, 100], [1, 255, 256, 257, 1000], [1, 3, 40]
    specs = []
    for i in range(100):
        p = ps[(i // 4) % 3]
        specs.append(dict(rows=[ns[i % 4]] + [rng.randint(1, 9) for _ in range(p - 1)], G=gs[i % 5], mode=(i // 2) % 2,
                          cls="EC"[(i // 20 + i) % 2], seed=rng.randrange(1 << 30)))
    return specs


def score_reduce_make(s, pool, dev):
    """-> score [sum rows, G]: multiples of 1/64 in [0,1] (class E: sums of up to 2^18 of them are exact) or |normal| scores."""
    rng = random.Random(s["seed"])
    n = sum(s["rows"])
    if s["cls"] == "E":
        return ints(rng, (n, s["G"]), 0, 64, dev) / 64.0
    return pool.take(rng, (n, s["G"]), 0.3).abs()


NLB_LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96]


def nlb_specs():
    rng = family_rng("nlb")
    specs = []
    for i in range(100):
        s_n = [1, 2, 5, 37][i % 4]
        long_ = i % 5 == 4                      # lengths 97 and 130: the VALU entry alone, through its global scratch
        lens = [NLB_LENS[(i + j) % 14] for j in range(min(s_n, 3))] + [rng.choice(NLB_LENS) for _ in range(max(0, s_n - 3))]
        if long_:
            lens[rng.randrange(s_n)] = [97, 130][(i // 5) % 2]
        tmax = max(1, max(lens))
        if s_n >= 2:
            j = rng.randrange(s_n)
            lens[j] = tmax + rng.randint(1, 5)                   # above Tmax: must behave as Tmax
            lens[(j + 1) % s_n] = -rng.randint(1, 3)            # negative: must behave as 0
        elif (i // 4) % 4 == 1:
            lens[0] = tmax + 2
        elif (i // 4) % 4 == 3:
            lens[0] = -1
        rng.shuffle(lens)
        specs.append(dict(S=s_n, Tmax=tmax, lens=lens, tm=(i // 2) % 2 == 1, pad=[0, 4, 260][(i // 4) % 3], use_nlb=i % 3,
                          att=(i // 3) % 2 == 0, z=(i // 6) % 2 == 0, seed=rng.randrange(1 << 30)))
    return specs


def nlb_make(s, pool, dev):
    """-> (flat buffer, element offset of sequence 0 / row 0, t_stride, s_stride): sequence-major [S,Tmax,rs], or time-major
    [1 + Tmax, S, rs] behind its dummy row; rs = 256 + pad."""
    rng = random.Random(s["seed"])
    rs = 256 + s["pad"]
    if s["tm"]:
        flat = pool.take(rng, ((1 + s["Tmax"]) * s["S"] * rs,))
        return flat, s["S"] * rs, s["S"] * rs, rs
    flat = pool.take(rng, (s["S"] * s["Tmax"] * rs,))
    return flat, 0, rs, s["Tmax"] * rs


def linear_narrow_specs():
    rng = family_rng("linear_narrow")
    cs, ks, ms = [16, 32, 240, 256], [1, 3, 14, 15, 16], [1, 15, 16, 17, 63, 65, 4097, 40000]
    return [dict(C=cs[i % 4], K=ks[i % 5], M=ms[(i // 4 + i) % 8], relu=(i // 2) % 2, cls="IC"[(i // 8 + i) % 2],
                 bias=i % 7 != 6, seed=rng.randrange(1 << 30)) for i in range(104)]


def linear_narrow_make(s, pool, dev):
    rng = random.Random(s["seed"])
    m, c, k = s["M"], s["C"], s["K"]
    if s["cls"] == "I":                 # |sum| <= 256 * 3 * 3 + 8 < 2^24: exact in any order
        x, w, bias = ints(rng, (m, c), -3, 3, dev), ints(rng, (k, c), -3, 3, dev), ints(rng, (k,), -8, 8, dev)
    else:
        x, w, bias = pool.take(rng, (m, c)), pool.take(rng, (k, c), 1.0 / math.sqrt(c)), pool.take(rng, (k,), 0.1)
    return x, w, (bias if s["bias"] else None)
