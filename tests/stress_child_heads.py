"""The child of ``test_gpu_stress_heads.py``: ``python stress_child_heads.py [family ...]`` runs the sweep on the GPU and prints the
lines ``stress_kit.family_ok`` reads.  Importing it launches nothing."""
import ctypes as C, math, os, sys, time
import torch
import train_refs as TR
from stress_kit import P, fail, fails, refused, say, st, twice

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64, F32, I64, I32 = torch.float64, torch.float32, torch.int64, torch.int32
WORST = {}


def check(name, desc, what, got, ref, tol, track=None):
    ok, msg, worst = HR.cmp_bounded(got, ref, tol)
    if track is not None:
        WORST[track] = max(WORST.get(track, 0.0), worst)
    if not ok:
        fail(name, desc, f"{what}: {msg}")
    return ok


def check_idx(name, desc, what, got, ref):
    ok, msg = HR.cmp_index(got, ref)
    if not ok:
        fail(name, desc, f"{what}: {msg}")
    return ok


def same_bits(name, desc, what, a, b):
    """Two fp32 results of the same arithmetic: equal bit for bit (a NaN must meet a NaN)."""
    ok = a.shape == b.shape and bool(((a.view(torch.int32) == b.view(torch.int32)) | (torch.isnan(a) & torch.isnan(b))).all())
    if not ok:
        fail(name, desc, f"{what}: not bit-identical")
    return ok


def pair_logits_dev(a, b, w, bias):
    out = torch.empty((a.shape[0], b.shape[0], 2), dtype=F32, device=dev)
    rc = lib.seam_pair_logits_f32(P(a), P(b), P(w), P(bias), P(out), a.shape[0], b.shape[0], a.shape[1], st())
    assert rc == 0, rc
    return out


# ------------------------------------------------------------------------------------------------ pair_logits
def stress_pair_logits():
    name = "pair_logits"
    t0 = time.time()
    done = exact = big = 0
    for s in HR.pair_logits_specs():
        q, g, d = s["Q"], s["G"], s["D"]
        tile = "4x4" if q * g >= (1 << 20) else "2x2"
        desc = f"Q{q} G{g} D{d} {s['cls']} tile{tile}"
        say("START", name, desc)
        a, b, w, bias = HR.pair_logits_make(s, pool, hw, dev)
        out = twice(name, desc, [(q, g, 2)], lambda bf: lib.seam_pair_logits_f32(P(a), P(b), P(w), P(bias), P(bf[0].t), q, g, d, st()))
        done += 1
        big += tile == "4x4"
        if out is None:
            continue
        ref, maj = HR.pair_logits64(a, b, w, bias)
        if s["cls"] == "I":
            exact += 1
            check(name, desc, "logits (exact)", out[0], ref, 0.0)
        else:
            # L = D + 3: D fma, the bias, and the two roundings (difference, square) of every term before it enters the chain
            check(name, desc, "logits", out[0], ref, TR.bound(maj, d + 3), track=name)
        del ref, maj
    a, b, w, bias = HR.pair_logits_make(dict(Q=4, G=4, D=64, cls="I", seed=5), pool, hw, dev)
    for desc, (q, g) in (("Q0", (0, 4)), ("G0", (4, 0))):
        say("START", name, desc, "(returns 0, writes nothing)")
        twice(name, desc, [(32,)], lambda bf: lib.seam_pair_logits_f32(P(a), P(b), P(w), P(bias), P(bf[0].t), q, g, 64, st()), live=[False])
    refused(name, "D48", [(4, 4, 2)], lambda bf: lib.seam_pair_logits_f32(P(a), P(b), P(w), P(bias), P(bf[0].t), 4, 4, 48, st()))
    say(f"SUMMARY {name} cases {done} exact {exact} tile4x4 {big} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ ranking kernels
def stress_rank():
    name = "rank"
    t0 = time.time()
    done = exact = 0
    for s in HR.rank_specs():
        q, g, k = s["Q"], s["G"], s["k"]
        desc = f"Q{q} G{g} k{k} {s['cls']}"
        say("START", name, desc)
        x, tg = HR.rank_make(s, pool, dev)

        def launch(bf):
            rc = lib.seam_rank_topk_f32(P(x), P(bf[0].t), P(bf[1].t), q, g, k, st())
            rc = rc or lib.seam_rank_of_f32(P(x), P(tg), P(bf[2].t), q, g, st())
            rc = rc or lib.seam_match_scores_f32(P(x), P(bf[3].t), q * g, st())
            return rc or lib.seam_rank_of_scores_f32(P(bf[3].t), P(tg), P(bf[4].t), q, g, st())
        out = twice(name, desc, [(q, k), (q, k), (q,), (q, g), (q,)], launch, dtypes=[I64, F32, I64, F32, I64])
        done += 1
        exact += s["cls"].startswith("I")
        if out is None:
            continue
        idx, score, rank, sc, rank2 = out
        d = x[..., 1] - x[..., 0]                  # the fp32 difference the kernels rank on (one correctly rounded subtraction)
        order = HR.rank_order(d, g)
        if check_idx(name, desc, "rank_topk idx", idx, order[:, :k]):
            xs = x.gather(1, order[:, :k, None].expand(q, k, 2))
            ref = HR.score64(xs)
            check(name, desc, "rank_topk score", score, ref, HR.score_tol(xs, ref), track=name)
        want = HR.rank_of(d, tg)
        check_idx(name, desc, "rank_of", rank, want)
        check_idx(name, desc, "rank_of vs position in the full order", rank, HR.position_in_order(order, tg))
        ref = HR.score64(x)
        check(name, desc, "match_scores", sc, ref, HR.score_tol(x, ref), track=name)
        check_idx(name, desc, "rank_of_scores", rank2, HR.rank_of(sc, tg))
    assert int(lib.seam_rank_topk_max_k()) == HR.TOPK_CAP
    for desc, (g, k) in (("k>G", (5, 6)), ("k257 G257", (257, 257)), ("k257 G1000", (1000, 257)), ("k5000 G5000", (5000, 5000))):
        x = HR.ints(HR.family_rng(name), (2, g, 2), -8, 8, dev)
        refused(name, desc, [(2, k), (2, k)], lambda bf: lib.seam_rank_topk_f32(P(x), P(bf[0].t), P(bf[1].t), 2, g, k, st()),
                dtypes=[I64, F32])
    say(f"SUMMARY {name} cases {done} exact {exact} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ fused top-k
def stress_pair_topk():
    name = "pair_topk"
    t0 = time.time()
    done = exact = short = 0
    for s in HR.pair_topk_specs():
        q, g, d, k = s["Q"], s["G"], s["D"], s["k"]
        last = g % 256
        desc = f"Q{q} G{g} D{d} k{k} {s['cls']} lastseg{last}"
        say("START", name, desc)
        a, b, w, bias = HR.pair_topk_make(s, pool, hw, dev)
        wsn = int(lib.seam_pair_topk_workspace_floats(q, g, k))
        if wsn < q * ((g + 255) // 256) * k * 3:
            fail(name, desc, f"workspace {wsn} too small")
            continue

        def launch(bf):
            rc = lib.seam_pair_topk_f32(P(a), P(b), P(w), P(bias), P(bf[0].t), P(bf[1].t), q, g, d, k, P(bf[2].t), st())
            rc = rc or lib.seam_pair_logits_f32(P(a), P(b), P(w), P(bias), P(bf[3].t), q, g, d, st())
            return rc or lib.seam_rank_topk_f32(P(bf[3].t), P(bf[4].t), P(bf[5].t), q, g, k, st())
        out = twice(name, desc, [(q, k), (q, k), (wsn,), (q, g, 2), (q, k), (q, k)], launch,
                    live=[True, True, "ws", True, True, True], dtypes=[I64, F32, F32, F32, I64, F32])
        done += 1
        short += 0 < last < k and g > 256
        if out is None:
            continue
        idx, score, _, lg, idx2, score2 = out
        check_idx(name, desc, "fused idx vs pair_logits + rank_topk", idx, idx2)
        same_bits(name, desc, "fused score vs pair_logits + rank_topk", score, score2)
        if s["cls"].startswith("I"):
            exact += 1
            ref, _ = HR.pair_logits64(a, b, w, bias)
            check(name, desc, "logits (exact)", lg, ref, 0.0)
            check_idx(name, desc, "fused idx vs float64", idx, HR.rank_order(ref[..., 1] - ref[..., 0], k))
        else:
            check_idx(name, desc, "idx vs the order of the device logits", idx, HR.rank_order(lg[..., 1] - lg[..., 0], k))
        xs = lg.gather(1, idx2.clamp(0, g - 1)[:, :, None].expand(q, k, 2))
        ref = HR.score64(xs)
        check(name, desc, "score", score, ref, HR.score_tol(xs, ref), track=name)
    a, b, w, bias = HR.pair_logits_make(dict(Q=3, G=300, D=64, cls="I", seed=6), pool, hw, dev)
    for desc, (g, d, k) in (("k257", (300, 64, 257)), ("k>G", (5, 64, 6)), ("D48", (300, 48, 5))):
        wsn = int(lib.seam_pair_topk_workspace_floats(3, g, k))
        refused(name, desc, [(3, k), (3, k), (wsn,)],
                lambda bf: lib.seam_pair_topk_f32(P(a), P(b), P(w), P(bias), P(bf[0].t), P(bf[1].t), 3, g, d, k, P(bf[2].t), st()),
                dtypes=[I64, F32, F32])
    say(f"SUMMARY {name} cases {done} exact {exact} shortseg {short} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ matrix-core top-k
def stress_pair_topk_mfma():
    name = "pair_topk_mfma"
    t0 = time.time()
    done = exact = 0
    for s in HR.pair_topk_mfma_specs():
        q, g, k, flags = s["Q"], s["G"], s["k"], s["flags"]
        desc = f"Q{q} G{g} k{k} flags{flags} {s['cls']}"
        say("START", name, desc)
        a, b, w, bias = HR.pair_topk_mfma_make(s, pool, hw, dev)
        wsn = int(lib.seam_pair_topk_mfma_workspace_floats(q, g, k))

        def launch(bf):
            rc = lib.seam_pair_topk_mfma_f32(P(a), P(b), P(w), P(bias), P(bf[0].t), P(bf[1].t), q, g, 256, k, P(bf[2].t), flags,
                                             P(bf[3].t), st())
            rc = rc or lib.seam_pair_logits_f32(P(a), P(b), P(w), P(bias), P(bf[4].t), q, g, 256, st())
            return rc or lib.seam_rank_topk_f32(P(bf[4].t), P(bf[5].t), P(bf[6].t), q, g, k, st())
        out = twice(name, desc, [(q, k), (q, k), (wsn,), (4,), (q, g, 2), (q, k), (q, k)], launch,
                    live=[True, True, "ws", "ws", True, True, True], dtypes=[I64, F32, F32, I32, F32, I64, F32])
        done += 1
        if out is None:
            continue
        idx, score, _, stats, lg, idx2, score2 = out
        sv = stats.tolist()
        say("STATS", name, desc, sv)
        if not (0 <= sv[0] <= q and 0 <= sv[2] <= sv[0] and sv[1] >= 0 and sv[3] == 0):
            fail(name, desc, f"stats inconsistent: {sv}")
        check_idx(name, desc, "idx vs pair_logits + rank_topk", idx, idx2)
        same_bits(name, desc, "score vs pair_logits + rank_topk", score, score2)
        if s["cls"] == "I":
            exact += 1
            ref, _ = HR.pair_logits64(a, b, w, bias)
            check(name, desc, "logits (exact)", lg, ref, 0.0)
            check_idx(name, desc, "idx vs float64", idx, HR.rank_order(ref[..., 1] - ref[..., 0], k))
            del ref
    a, b, w, bias = HR.pair_topk_mfma_make(dict(Q=2, G=8192, k=5, flags=0, cls="C", seed=7), pool, hw, dev)
    a2 = torch.cat([a.reshape(-1), a.reshape(-1)[:4]])[1:1 + 512].view(2, 256)             # 4 bytes off a 16-byte boundary
    wsn = int(lib.seam_pair_topk_mfma_workspace_floats(2, 8192, 64))
    for desc, (aa, g, d, k) in (("G8191", (a, 8191, 256, 5)), ("k65", (a, 8192, 256, 65)), ("D128", (a, 8192, 128, 5)),
                                ("a misaligned", (a2, 8192, 256, 5))):
        refused(name, desc, [(2, k), (2, k), (wsn,), (4,)],
                lambda bf: lib.seam_pair_topk_mfma_f32(P(aa), P(b), P(w), P(bias), P(bf[0].t), P(bf[1].t), 2, g, d, k, P(bf[2].t), 0,
                                                       P(bf[3].t), st()), dtypes=[I64, F32, F32, I32])
    say(f"SUMMARY {name} cases {done} exact {exact} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ block-diagonal scores
def stress_blockdiag():
    name = "blockdiag"
    t0 = time.time()
    done = exact = 0
    for s in HR.blockdiag_specs():
        x, seg, w, bias = HR.blockdiag_make(s, pool, hw, dev)
        n = s["n"]
        mx = max(n) + s["extra"]
        desc = f"n{n} D{s['D']} max_rows{mx} {s['cls']}"
        say("START", name, desc)
        off = [0]
        for v in n:
            off.append(off[-1] + v * v)
        seg_d = torch.tensor(seg, dtype=I32, device=dev)
        off_d = torch.tensor(off, dtype=I64, device=dev)
        out = twice(name, desc, [(off[-1],)],
                    lambda bf: lib.seam_pair_scores_blockdiag_f32(P(x), P(seg_d), P(off_d), P(w), P(bias), P(bf[0].t), len(n), mx, s["D"], st()))
        done += 1
        if out is None:
            continue
        parts, lgs = [], []
        for i, v in enumerate(n):                  # the same blocks one by one: pair_logits + match_scores
            if v == 0:
                continue
            xs = x[seg[i]:seg[i + 1]]
            lg = pair_logits_dev(xs, xs, w, bias)
            sc = torch.empty((v * v,), dtype=F32, device=dev)
            assert lib.seam_match_scores_f32(P(lg), P(sc), v * v, st()) == 0
            parts.append(sc)
            lgs.append(lg.reshape(-1, 2))
        same_bits(name, desc, "vs match_scores(pair_logits) per group", out[0], torch.cat(parts))
        if s["cls"] == "I":
            exact += 1
            ref, lg64 = HR.blockdiag64(x, seg, w, bias)
            check(name, desc, "logits of the groups (exact)", torch.cat(lgs), lg64, 0.0)
            check(name, desc, "scores", out[0], ref, HR.score_tol(lg64, ref), track=name)
    x, seg, w, bias = HR.blockdiag_make(dict(n=[3, 0, 2], D=32, cls="I", seed=8), pool, hw, dev)
    seg_d, off_d = torch.tensor(seg, dtype=I32, device=dev), torch.tensor([0, 9, 9, 13], dtype=I64, device=dev)
    for desc, (ns, mr) in (("n_seg0", (0, 3)), ("max_rows0", (3, 0))):
        say("START", name, desc, "(returns 0, writes nothing)")
        twice(name, desc, [(13,)], lambda bf: lib.seam_pair_scores_blockdiag_f32(P(x), P(seg_d), P(off_d), P(w), P(bias), P(bf[0].t), ns, mr, 32, st()),
              live=[False])
    for desc, (ns, dd) in (("D48", (3, 48)), ("n_seg65536", (65536, 32))):
        refused(name, desc, [(13,)], lambda bf: lib.seam_pair_scores_blockdiag_f32(P(x), P(seg_d), P(off_d), P(w), P(bias), P(bf[0].t), ns, 3, dd, st()))
    say(f"SUMMARY {name} cases {done} exact {exact} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ score reductions
def stress_score_reduce():
    name = "score_reduce"
    t0 = time.time()
    done = exact = 0

    def run(desc, sc, rows, g, mode):
        p = len(rows)
        seg = [0]
        for r in rows:
            seg.append(seg[-1] + r)
        seg_d = torch.tensor(seg, dtype=I32, device=dev)

        def launch(bf):
            rc = lib.seam_score_reduce_seg_f32(P(sc), P(seg_d), P(bf[0].t), p, g, mode, st())
            for i, r in enumerate(rows):          # the same segments one by one (n = 0 is refused there: skipped)
                if r > 0:
                    rc = rc or lib.seam_score_reduce_f32(P(sc[seg[i]:]), P(bf[1].t[i]), r, g, mode, st())
            return rc
        live1 = torch.tensor([r > 0 for r in rows], device=dev)[:, None].expand(p, g)
        out = twice(name, desc, [(p, g), (p, g)], launch, live=[True, live1])
        if out is None:
            return None
        same_bits(name, desc, "_seg vs per-segment calls", out[0][live1], out[1][live1])
        return out[0], seg

    for s in HR.score_reduce_specs():
        rows, g, mode = s["rows"], s["G"], s["mode"]
        desc = f"rows{rows[:5]}{'..' if len(rows) > 5 else ''} P{len(rows)} G{g} mode{mode} {s['cls']}"
        say("START", name, desc)
        sc = HR.score_reduce_make(s, pool, dev)
        r = run(desc, sc, rows, g, mode)
        done += 1
        if r is None:
            continue
        got, seg = r
        for i, n in enumerate(rows):
            part = sc[seg[i]:seg[i + 1]]
            ref = HR.score_reduce64(part, mode)
            if mode == 1:
                check(name, desc, f"max of segment {i} (exact)", got[i], ref, 0.0)
            elif s["cls"] == "E":
                # the sum of multiples of 1/64 is exact; the division is correctly rounded, and rounding the float64 quotient
                # to fp32 gives the same number (53 >= 2 * 24 + 2 bits: double rounding is innocuous for a quotient)
                check(name, desc, f"mean of segment {i} (exact)", got[i], ref.to(F32), 0.0)
            else:
                # L = n + 1: n additions and the division
                check(name, desc, f"mean of segment {i}", got[i], ref, TR.bound(part.to(F64).abs().sum(0) / n, n + 1), track=name)
        exact += s["cls"] == "E" or mode == 1
    # what the header says about an empty segment (mean NaN, max -inf) and a NaN score (poisons the mean, ignored by the max)
    sc = HR.ints(HR.family_rng(name), (7, 257), 0, 64, dev) / 64.0
    sc[2, 5] = math.nan
    sc[3:, 6] = math.nan
    for mode in (0, 1):
        desc = f"empty segment and NaN scores, mode{mode}"
        say("START", name, desc)
        r = run(desc, sc, [3, 0, 4], 257, mode)
        done += 1
        if r is not None:
            for i, (lo, hi) in enumerate(((0, 3), (3, 3), (3, 7))):
                check(name, desc, f"segment {i}", r[0][i], HR.score_reduce64(sc[lo:hi], mode).to(F32), 0.0)
    seg_d = torch.tensor([0, 3, 7], dtype=I32, device=dev)
    refused(name, "mode2", [(257,)], lambda bf: lib.seam_score_reduce_f32(P(sc), P(bf[0].t), 7, 257, 2, st()))
    refused(name, "n0", [(257,)], lambda bf: lib.seam_score_reduce_f32(P(sc), P(bf[0].t), 0, 257, 0, st()))
    refused(name, "seg mode2", [(2, 257)], lambda bf: lib.seam_score_reduce_seg_f32(P(sc), P(seg_d), P(bf[0].t), 2, 257, 2, st()))
    refused(name, "seg P65536", [(2, 257)], lambda bf: lib.seam_score_reduce_seg_f32(P(sc), P(seg_d), P(bf[0].t), 65536, 257, 0, st()))
    say(f"SUMMARY {name} cases {done} exact {exact} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ NLB + attention pooling
def nlb_mfma_pack(pk):
    wp, bp, wc = pk["w_proj_t"].double(), pk["b_proj"].double(), pk["w_cat"].double()
    u = (wp[:, :128] @ wc[:128]).float().contiguous()
    v = (wp[:, 128:256] @ wc[128:]).float().contiguous()
    cd = torch.stack([bp[:128] @ wc[:128], bp[128:256] @ wc[128:]]).float().contiguous()
    wg_frag = pk["w_proj_t"][:, 256:].reshape(32, 2, 4, 4, 32).permute(3, 0, 1, 4, 2).contiguous()
    wo_frag = pk["w_out_t"].reshape(16, 2, 4, 8, 32).permute(3, 0, 1, 4, 2).contiguous()
    return wg_frag, pk["b_proj"][256:].contiguous(), u, v, cd, wo_frag


def stress_nlb():
    name = "nlb"
    t0 = time.time()
    done = both = scratch = 0
    pk = hw["pk"]
    mf = nlb_mfma_pack(pk)
    tmf = int(lib.seam_nlb_mfma_max_len())

    def valu(seq_ptr, t_st, s_st, lens_d, S, Tmax, out, att, z, ws, use):
        return lib.seam_nlb_attnpool_f32(seq_ptr, t_st, s_st, P(lens_d), S, Tmax, P(pk["w_proj_t"]), P(pk["b_proj"]), P(pk["w_cat"]),
                                         P(pk["w_out_t"]), P(pk["b_out"]), P(pk["w_att"]), P(pk["b_att"]), P(out), P(att), P(z), P(ws),
                                         use, st())

    def mfma(seq_ptr, t_st, s_st, lens_d, S, Tmax, out, att, z, use):
        return lib.seam_nlb_attnpool_mfma_f32(seq_ptr, t_st, s_st, P(lens_d), S, Tmax, P(mf[0]), P(mf[1]), P(mf[2]), P(mf[3]), P(mf[4]),
                                              P(mf[5]), P(pk["b_out"]), P(pk["w_att"]), P(pk["b_att"]), P(out), P(att), P(z), use, st())

    for s in HR.nlb_specs():
        S, Tmax, lens, use = s["S"], s["Tmax"], s["lens"], s["use_nlb"]
        flat, off, t_st, s_st = HR.nlb_make(s, pool, dev)
        eff = [max(0, min(l, Tmax)) for l in lens]
        do_mf = Tmax <= tmf
        desc = (f"S{S} Tmax{Tmax} use{use} {'tm' if s['tm'] else 'bm'} rs{256 + s['pad']} att{int(s['att'])} z{int(s['z'])} "
                f"mfma{int(do_mf)} lens{lens[:6]}{'..' if S > 6 else ''}")
        say("START", name, desc)
        lens_d = torch.tensor(lens, dtype=I32, device=dev)
        seq_ptr = flat.data_ptr() + 4 * off
        wsn = int(lib.seam_nlb_workspace_floats(S, Tmax))
        if wsn < S * Tmax * 130:
            fail(name, desc, f"workspace {wsn} too small")
            continue
        tmask = torch.arange(Tmax, device=dev)[None, :] < torch.tensor(eff, device=dev)[:, None]           # [S,Tmax]: t < len[s]
        zmask = tmask[:, :, None].expand(S, Tmax, 256)
        live = [True, tmask if s["att"] else False, zmask if s["z"] else False]
        att_of = lambda bf: bf[1].t if s["att"] else None
        z_of = lambda bf: bf[2].t if s["z"] else None
        shapes = [(S, 256), (S, Tmax), (S, Tmax, 256)]
        runs = [("valu", twice(name, desc + " [valu]", shapes + [(wsn,)],
                               lambda bf: valu(seq_ptr, t_st, s_st, lens_d, S, Tmax, bf[0].t, att_of(bf), z_of(bf), bf[3].t, use),
                               live=live + ["ws"]))]
        if do_mf:
            runs.append(("mfma", twice(name, desc + " [mfma]", shapes,
                                       lambda bf: mfma(seq_ptr, t_st, s_st, lens_d, S, Tmax, bf[0].t, att_of(bf), z_of(bf), use), live=live)))
            both += 1
        scratch += any(e > 96 for e in eff)
        done += 1
        if any(o is None for _, o in runs):
            continue
        if any(l > Tmax for l in lens):            # a length above Tmax == a length of exactly Tmax, bit for bit
            lc = torch.tensor([min(l, Tmax) for l in lens], dtype=I32, device=dev)
            o2 = twice(name, desc + " [valu clamped]", shapes + [(wsn,)],
                       lambda bf: valu(seq_ptr, t_st, s_st, lc, S, Tmax, bf[0].t, att_of(bf), z_of(bf), bf[3].t, use), live=live + ["ws"])
            if o2 is not None:
                same_bits(name, desc, "len > Tmax vs len == Tmax", runs[0][1][0], o2[0])
        rows = TR.seq_rows(flat[off:].clone(), t_st, s_st, lens, S, Tmax)
        lv = [i for i in range(S) if eff[i] > 0]
        ref = HR.nlb_attnpool64([rows[i] for i in lv], hw["p"], use)
        r_out = torch.zeros((S, 256), dtype=F64, device=dev)            # rows of len <= 0: exact zeros (tolerance 0)
        d_out = torch.zeros((S, 256), dtype=F64, device=dev)
        r_att = torch.zeros((S, Tmax), dtype=F64, device=dev)
        d_att = torch.zeros((S, Tmax), dtype=F64, device=dev)
        r_z = torch.zeros((S, Tmax, 256), dtype=F64, device=dev)
        d_z = torch.zeros((S, Tmax, 256), dtype=F64, device=dev)
        for i, r in zip(lv, ref):
            t = eff[i]
            r_out[i], d_out[i] = r["out"], r["d_out"]
            r_att[i, :t], d_att[i, :t] = r["att"], r["d_att"]
            r_z[i, :t], d_z[i, :t] = r["z"], r["d_z"]               # bypassed sequences: d_z = 0, Z must be X bit for bit
        for kind, o in runs:
            check(name, desc, f"{kind} out", o[0], r_out, d_out, track=name)
            if s["att"]:
                check(name, desc, f"{kind} att", o[1][tmask], r_att[tmask], d_att[tmask], track=name)
            if s["z"]:
                check(name, desc, f"{kind} z", o[2][zmask], r_z[zmask], d_z[zmask], track=name)
        if do_mf:                                   # the two forms agree within the sum of their bounds
            check(name, desc, "valu vs mfma out", runs[0][1][0], runs[1][1][0].to(F64), 2 * d_out)
            if s["att"]:
                check(name, desc, "valu vs mfma att", runs[0][1][1][tmask], runs[1][1][1][tmask].to(F64), 2 * d_att[tmask])
            if s["z"]:
                check(name, desc, "valu vs mfma z", runs[0][1][2][zmask], runs[1][1][2][zmask].to(F64), 2 * d_z[zmask])
    # refusals of the MFMA entry (nothing written), and S = 0
    flat = pool.take(HR.family_rng(name), (2 * 97 * 260 + 8,))
    lens_d = torch.tensor([5, 7], dtype=I32, device=dev)
    shapes = [(2, 256), (2, 97), (2, 97, 256)]
    for desc, (ptr, t_st, s_st, Tmax) in (("Tmax97", (flat.data_ptr(), 256, 97 * 256, 97)), ("t_stride%4", (flat.data_ptr(), 258, 96 * 258, 96)),
                                          ("s_stride%4", (flat.data_ptr(), 256, 96 * 256 + 2, 96)),
                                          ("seq misaligned", (flat.data_ptr() + 4, 256, 96 * 256, 96))):
        refused(name, desc, shapes, lambda bf: mfma(ptr, t_st, s_st, lens_d, 2, Tmax, bf[0].t, bf[1].t, bf[2].t, 1))
    wsn = int(lib.seam_nlb_workspace_floats(2, 96))
    say("START", name, "S0 (returns 0, writes nothing)")
    twice(name, "S0 valu", shapes + [(wsn,)], lambda bf: valu(flat.data_ptr(), 256, 96 * 256, lens_d, 0, 96, bf[0].t, bf[1].t, bf[2].t, bf[3].t, 1),
          live=[False, False, False, False])
    twice(name, "S0 mfma", shapes, lambda bf: mfma(flat.data_ptr(), 256, 96 * 256, lens_d, 0, 96, bf[0].t, bf[1].t, bf[2].t, 1),
          live=[False, False, False])
    say(f"SUMMARY {name} cases {done} both_forms {both} scratch_path {scratch} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


# ------------------------------------------------------------------------------------------------ narrow linear
def stress_linear_narrow():
    name = "linear_narrow"
    t0 = time.time()
    done = exact = 0
    for s in HR.linear_narrow_specs():
        m, c, k, relu = s["M"], s["C"], s["K"], s["relu"]
        desc = f"M{m} C{c} K{k} relu{relu} bias{int(s['bias'])} {s['cls']}"
        say("START", name, desc)
        x, w, bias = HR.linear_narrow_make(s, pool, dev)
        if int(lib.seam_linear_narrow_supported(c, k)) != 1:
            fail(name, desc, "seam_linear_narrow_supported says no")
            continue

        def launch(bf):
            rc = lib.seam_pack_linear_narrow_f32(P(w), P(bf[1].t), k, c, st())
            return rc or lib.seam_linear_narrow_f32(P(x), P(bf[1].t), P(bias), P(bf[0].t), m, c, k, relu, st())
        # the header sizes w_packed at 64 * C floats; the pack writes (and the kernel reads) [C / 16][64 lanes][4] = the first
        # 16 * C of them, the rest must keep its poison
        packed = torch.arange(64 * c, device=dev) < 16 * c
        out = twice(name, desc, [(m, k), (64 * c,)], launch, live=[True, packed])
        done += 1
        if out is None:
            continue
        ref, maj = HR.linear_narrow64(x, w, bias, relu)
        if s["cls"] == "I":
            exact += 1
            check(name, desc, "y (exact)", out[0], ref, 0.0)
        else:
            # L = C + 2: C MFMA accumulations, the bias, the stored result
            check(name, desc, "y", out[0], ref, TR.bound(maj, c + 2), track=name)
    x, w, bias = HR.linear_narrow_make(dict(M=20, C=256, K=16, cls="I", bias=True, seed=9), pool, dev)
    wp = torch.zeros((64 * 272,), device=dev)
    for desc, (m, c, k) in (("C8", (20, 8, 4)), ("C272", (15, 272, 4)), ("K17", (15, 256, 17)), ("M0", (0, 256, 16))):
        refused(name, desc, [(20, 17)], lambda bf: lib.seam_linear_narrow_f32(P(x), P(wp), P(bias), P(bf[0].t), m, c, k, 0, st()))
        if desc != "M0":
            refused(name, desc + " pack", [(64 * 272,)], lambda bf: lib.seam_pack_linear_narrow_f32(P(w), P(bf[0].t), k, c, st()))
            if int(lib.seam_linear_narrow_supported(c, k)) != 0:
                fail(name, desc, "seam_linear_narrow_supported says yes")
    say(f"SUMMARY {name} cases {done} exact {exact} worst {WORST.get(name, 0.0):.4f} seconds {time.time() - t0:.1f}")


FAMILIES = [("pair_logits", stress_pair_logits), ("rank", stress_rank), ("pair_topk", stress_pair_topk),
            ("pair_topk_mfma", stress_pair_topk_mfma), ("blockdiag", stress_blockdiag), ("score_reduce", stress_score_reduce),
            ("nlb", stress_nlb), ("linear_narrow", stress_linear_narrow)]


def main(argv):
    global HR, dev, lib, pool, hw
    sys.path.insert(0, ROOT)                   # heads_refs imports the package
    import heads_refs as HR
    from seam_match_rcnn_amd import _native
    assert [n for n, _ in FAMILIES] == HR.FAMILIES
    dev = torch.device("cuda:0")
    lib = _native.lib()
    pool = HR.Pool(dev)
    hw = HR.head_weights(dev)
    for name, fn in FAMILIES:
        if argv and name not in argv:
            continue
        before = len(fails)
        fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        say("KERNEL", name, "failures", len(fails) - before)
    say("DONE failures", len(fails))
    for f in fails[:40]:
        say("FAILED", *f)
    return 1 if fails else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
