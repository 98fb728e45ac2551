"""The float64 references, bounds, comparators and case generators of ``heads_refs.py`` (used by the GPU sweep
``test_gpu_stress_heads.py``) on the CPU: tied to ``oracle/heads.py`` / ``oracle/evaluator.py`` and the reference vectors of
``heads_golden.npz`` (a wrong reference must neither pass nor fail the sweep); every comparator rejects a planted error
(teeth); and the fp32 CPU evaluation of the same expression -- ``oracle.heads`` in fp32, a different summation order from any
kernel -- is accepted on every continuous case of the sweep at its seeds (no tolerance is tighter than fp32 itself)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import heads_refs as HR
import seam_match_rcnn_amd.synth as synth
import train_refs as TR
from oracle import evaluator as OE
from oracle import heads as OH

F64, F32 = torch.float64, torch.float32
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def pool():
    return HR.Pool(CPU)


@pytest.fixture(scope="module")
def hw():
    return HR.head_weights(CPU)


def _gen(seed):
    g = torch.Generator()
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------ references
def test_rank_order_matches_oracle_on_nan_free_input():
    g = _gen(1)
    for q, n, k in [(3, 1, 1), (4, 40, 7), (2, 300, 256), (5, 17, 17)]:
        x5 = torch.randint(-3, 4, (q, n, 2), generator=g).to(F32)           # full of ties
        d = x5[..., 1] - x5[..., 0]
        idx, _ = OH.rank_topk(x5, k)
        assert torch.equal(HR.rank_order(d, k), idx)
        full = HR.rank_order(d, n)
        tg = torch.randint(-1, n + 1, (q,), generator=g)
        want = HR.rank_of(d, tg)
        assert torch.equal(HR.position_in_order(full, tg), want)
        sc = HR.score64(x5).numpy()
        for r in range(q):
            t = int(tg[r])
            if 0 <= t < n:                       # the evaluator's own ranking of a score row
                assert OE._rank_of(sc[r], t) == int(HR.rank_of(torch.from_numpy(sc[r:r + 1]), tg[r:r + 1])[0])
                assert OE._rank_of(d[r].numpy(), t) == int(want[r])
            else:
                assert int(want[r]) == -1


def test_rank_order_special_values():
    nan, inf = math.nan, math.inf
    d = torch.tensor([[0.0, nan, -0.0, inf, -inf, 2.0, nan, 0.0, 2.0]])
    assert HR.rank_order(d, 9).tolist() == [[3, 5, 8, 0, 2, 7, 1, 4, 6]]       # NaN ties with -inf: lower index first among them
    assert HR.rank_of(d, torch.tensor([2])).tolist() == [4]
    assert HR.rank_of(d, torch.tensor([1])).tolist() == [6]
    assert HR.rank_of(d, torch.tensor([9])).tolist() == [-1] and HR.rank_of(d, torch.tensor([-1])).tolist() == [-1]
    # torch's descending argsort -- what oracle.heads.rank_topk uses -- puts NaN FIRST: it cannot be the reference here
    assert int(torch.argsort(d, dim=1, descending=True, stable=True)[0, 0]) in (1, 6)


def test_pair_logits64_matches_oracle_and_golden(golden, hw):
    g = _gen(2)
    a, b = torch.randn((5, 96), generator=g, dtype=F64), torch.randn((9, 96), generator=g, dtype=F64)
    w, bias = torch.randn((2, 96), generator=g, dtype=F64), torch.randn((2,), generator=g, dtype=F64)
    lg, maj = HR.pair_logits64(a, b, w, bias)
    torch.testing.assert_close(lg, OH.pair_logits(a, b, w, bias), rtol=1e-12, atol=1e-12)
    assert bool((maj >= lg.abs()).all())
    ai, bi = HR.ints(HR.family_rng("rank"), (4, 64), -3, 3, CPU), HR.ints(HR.family_rng("rank"), (6, 64), -3, 3, CPU)
    wi = HR.ints(HR.family_rng("rank"), (2, 64), -4, 4, CPU)
    li, _ = HR.pair_logits64(ai, bi, wi, torch.tensor([3.0, -8.0]))
    assert torch.equal(li, torch.round(li)) and torch.equal(li.to(F32).to(F64), li)
    assert torch.equal(li.to(F32), OH.pair_logits(ai, bi, wi, torch.tensor([3.0, -8.0])))     # exact in any order, fp32 too
    # the reference's own fp32 vectors: Mode-B descriptors against the 16-product gallery
    x = torch.from_numpy(golden["taB_x3_1b"])
    gal = torch.from_numpy(synth.gallery(34, 16))
    lg, maj = HR.pair_logits64(x, gal, hw["last_w"], hw["last_b"])
    ok, msg, _ = HR.cmp_bounded(torch.from_numpy(golden["taB_x5"]), lg, TR.bound(maj, 256 + 3))
    assert ok, msg


def _mode_b_seqs(golden):
    seq = torch.from_numpy(synth.normal(synth.stream_id(33, "seq"), (11, 4, 256)))
    return [seq[1:n + 1, i] for i, n in enumerate(golden["taB_lens"].tolist())]


def test_nlb_attnpool64_matches_oracle_and_golden(golden, hw):
    g = _gen(3)
    p = hw["p"]
    seqs = [torch.randn((t, 256), generator=g, dtype=F64) for t in (1, 2, 5, 17, 40)]
    for use in (0, 1, 2):
        res = HR.nlb_attnpool64(seqs, p, use)
        if use < 2:
            out, atts = OH.aggregate_sequences(seqs, p, bool(use))
        else:
            zs = [OH.nlb_closed_form(x, p) for x in seqs]
            po = [OH.attention_pool(z, p) for z in zs]
            out, atts = torch.stack([o for o, _ in po]), [s for _, s in po]
        for i, r in enumerate(res):
            torch.testing.assert_close(r["out"], out[i], rtol=1e-11, atol=1e-12)
            torch.testing.assert_close(r["att"], atts[i][:, 0], rtol=1e-11, atol=1e-13)
            z = OH.nlb_closed_form(seqs[i], p) if HR.nlb_applies(use, seqs[i].shape[0]) else seqs[i]
            torch.testing.assert_close(r["z"], z, rtol=1e-11, atol=1e-12)
            assert bool((r["d_z"] == 0).all()) == (not HR.nlb_applies(use, seqs[i].shape[0]))
    # the reference's own fp32 vectors lie inside the propagated bounds
    seqs = _mode_b_seqs(golden)
    res = HR.nlb_attnpool64(seqs, p, 1)
    for i, r in enumerate(res):
        ok, msg, _ = HR.cmp_bounded(torch.from_numpy(golden["taB_x3_1b"][i]), r["out"], r["d_out"])
        assert ok, (i, msg)
        ok, msg, _ = HR.cmp_bounded(torch.from_numpy(golden[f"taB_att{i}"][:, 0]), r["att"], r["d_att"])
        assert ok, (i, msg)
    for t in (2, 3, 10):
        x = torch.from_numpy(synth.normal(synth.stream_id(21, f"nlb_x{t}"), (t, 256)))
        r = HR.nlb_attnpool64([x], p, 1)[0]
        ok, msg, _ = HR.cmp_bounded(torch.from_numpy(golden[f"nlb_T{t}_z"]), r["z"], r["d_z"])
        assert ok, (t, msg)


def test_plain_references():
    g = _gen(4)
    s = torch.rand((7, 13), generator=g, dtype=F64)
    torch.testing.assert_close(HR.score_reduce64(s, 0), s.mean(0), rtol=1e-15, atol=0)
    assert torch.equal(HR.score_reduce64(s, 1), s.max(0).values)
    s[2, 5] = math.nan
    s[:, 6] = math.nan
    m0, m1 = HR.score_reduce64(s, 0), HR.score_reduce64(s, 1)
    assert math.isnan(float(m0[5])) and math.isnan(float(m0[6]))
    assert float(m1[5]) == float(torch.cat([s[:2, 5], s[3:, 5]]).max()) and float(m1[6]) == -math.inf
    e0, e1 = HR.score_reduce64(s[:0], 0), HR.score_reduce64(s[:0], 1)
    assert bool(torch.isnan(e0).all()) and bool((e1 == -math.inf).all())
    x = torch.randn((9, 32), generator=g, dtype=F64)
    w, bias = torch.randn((2, 32), generator=g, dtype=F64), torch.randn((2,), generator=g, dtype=F64)
    sc, lg = HR.blockdiag64(x, [0, 4, 4, 9], w, bias)
    want = [OH.match_scores(OH.pair_logits(x[a:b], x[a:b], w, bias)).reshape(-1) for a, b in ((0, 4), (4, 9))]
    torch.testing.assert_close(sc, torch.cat(want), rtol=1e-12, atol=1e-14)
    assert sc.numel() == 16 + 25 and lg.shape == (41, 2)
    torch.testing.assert_close(HR.score64(lg), sc, rtol=0, atol=0)
    wn, bn = torch.randn((5, 32), generator=g, dtype=F64), torch.randn((5,), generator=g, dtype=F64)
    y, maj = HR.linear_narrow64(x, wn, bn, 1)
    torch.testing.assert_close(y, F.relu(F.linear(x, wn, bn)), rtol=1e-13, atol=1e-14)
    assert bool((maj >= y.abs()).all())
    # the score bound stays inside what test_gpu_ops.assert_close allows at its defaults (1e-3 relative) wherever fp32 has a score
    d = torch.linspace(-104, 104, 417, dtype=F64)
    lgd = torch.stack([torch.zeros_like(d), d], 1)
    ref = HR.score64(lgd)
    assert bool((HR.score_tol(lgd, ref) <= 1e-3 * ref + HR.FLT_MIN).all())


# ------------------------------------------------------------------------------------------------ teeth
def test_teeth_ranking():
    rng = HR.family_rng("rank")
    x = HR.ints(rng, (2, 600, 2), -8, 8, CPU)
    d = x[..., 1] - x[..., 0]
    ref = HR.rank_order(d, 20)
    assert HR.cmp_index(ref.clone(), ref)[0]
    # two tied indices swapped
    r = 0
    j = next(j for j in range(19) if d[r, ref[r, j]] == d[r, ref[r, j + 1]])
    bad = ref.clone()
    bad[r, j], bad[r, j + 1] = ref[r, j + 1], ref[r, j]
    assert float(d[r, bad[r, j]]) == float(d[r, ref[r, j]])              # the same values: only the tie rule tells them apart
    assert not HR.cmp_index(bad, ref)[0]
    # the NaN entry ranked first (what a descending sort does with NaN)
    d2 = d.clone()
    d2[1, 77] = math.nan
    ref2 = HR.rank_order(d2, 20)
    nan_first = torch.argsort(d2, dim=1, descending=True, stable=True)[:, :20]
    assert int(nan_first[1, 0]) == 77 and 77 not in ref2[1].tolist()
    assert not HR.cmp_index(nan_first, ref2)[0]
    tg = torch.tensor([5, 77])
    assert not HR.cmp_index(torch.tensor([int(HR.rank_of(d2, tg)[0]), 0]), HR.rank_of(d2, tg))[0]
    # one 256-column segment's candidates dropped: its winners are missing from the merged top k
    seg = int(ref[0, 0]) // 256
    dd = d.clone()
    dd[:, 256 * seg:256 * (seg + 1)] = -math.inf
    assert not HR.cmp_index(HR.rank_order(dd, 20), ref)[0]


def test_teeth_bounded_and_untouched(pool, hw):
    s = [c for c in HR.pair_logits_specs() if c["cls"] == "C"][3]
    a, b, w, bias = HR.pair_logits_make(s, pool, hw, CPU)
    lg, maj = HR.pair_logits64(a, b, w, bias)
    tol = TR.bound(maj, s["D"] + 3)
    assert HR.cmp_bounded(lg.to(F32), lg, tol)[0]
    moved = lg.clone()
    moved[0, 0, 1] += 2 * tol[0, 0, 1]                                    # a logit moved by twice its bound
    ok, _, worst = HR.cmp_bounded(moved, lg, tol)
    assert not ok and worst >= 1.9
    assert not HR.cmp_bounded(torch.tensor([math.nan, 1.0]), torch.tensor([1.0, 1.0]), 1.0)[0]
    assert not HR.cmp_bounded(torch.tensor([math.inf]), torch.tensor([-math.inf]), 1.0)[0]
    assert HR.cmp_bounded(torch.tensor([math.nan, math.inf]), torch.tensor([math.nan, math.inf]), 0.0)[0]
    # an element past len[s] overwritten
    for poison in (math.nan, 3.0e4, 0x5B5B5B5B5B5B5B5B):
        t = torch.full((3, 8), poison, dtype=torch.int64 if isinstance(poison, int) else F32)
        written = torch.zeros((3, 8), dtype=torch.bool)
        written[:, :5] = True
        t[:, :5] = 1
        assert HR.cmp_untouched(t, written, poison)[0]
        t[1, 6] = 0
        assert not HR.cmp_untouched(t, written, poison)[0]
        assert not HR.cmp_untouched(t, None, poison)[0]


def test_teeth_nlb(pool, hw):
    p = hw["p"]
    rng = HR.family_rng("nlb")
    for t in (2, 17, 96, 130):
        x = pool.take(rng, (t, 256))
        ref = HR.nlb_attnpool64([x], p, 1)[0]
        got = {k: ref[k].to(F32) for k in ("out", "att", "z")}          # rounding the exact values passes
        for k in got:
            assert HR.cmp_bounded(got[k], ref[k], ref["d_" + k])[0], (t, k)
        off = HR.nlb_attnpool64([x], p, 1, _inv_t=lambda n: 1.0 / (n + 1))[0]          # 1/T replaced by 1/(T+1) in the block
        assert not HR.cmp_bounded(off["z"], ref["z"], ref["d_z"])[0], t
        assert not HR.cmp_bounded(off["out"], ref["out"], ref["d_out"])[0], t
        cut = HR.nlb_attnpool64([x], p, 1, _softmax_rows=lambda n: n - 1)[0]            # one row left out of the softmax
        assert not HR.cmp_bounded(cut["att"], ref["att"], ref["d_att"])[0], t
        assert not HR.cmp_bounded(cut["out"], ref["out"], ref["d_out"])[0], t


# ------------------------------------------------------------------------------------------------ tolerances vs fp32
def test_tolerance_pair_logits_and_scores(pool, hw):
    worst_l = worst_s = 0.0
    specs = [s for s in HR.pair_logits_specs() if s["cls"] == "C"]
    assert len(specs) >= 40
    for s in specs:
        a, b, w, bias = HR.pair_logits_make(s, pool, hw, CPU)
        lg, maj = HR.pair_logits64(a, b, w, bias)
        got = OH.pair_logits(a, b, w, bias)
        assert got.dtype == F32
        ok, msg, r = HR.cmp_bounded(got, lg, TR.bound(maj, s["D"] + 3))
        assert ok, (s, msg)
        worst_l = max(worst_l, r)
        ref = HR.score64(got)                               # the score of the fp32 logits themselves: no logit error enters
        ok, msg, r = HR.cmp_bounded(OH.match_scores(got), ref, HR.score_tol(got, ref))
        assert ok, (s, msg)
        worst_s = max(worst_s, r)
    print(f"fp32 oracle / bound: logits {worst_l:.3f} scores {worst_s:.3f}")
    assert 0 < worst_l < 1 and 0 < worst_s < 1


def test_tolerance_rank_scores(pool):
    specs = [s for s in HR.rank_specs() if s["cls"].startswith("C")]
    assert len(specs) >= 50
    worst = 0.0
    for s in specs:
        x, _ = HR.rank_make(s, pool, CPU)
        ref = HR.score64(x)
        got = OH.match_scores(x)
        # torch's softmax gives NaN for a row that holds an infinity of either sign; the kernels' max-shifted form (and the
        # reference) only for +inf: compare where the fp32 oracle is defined
        m = ~torch.isnan(got) | torch.isnan(ref)
        ok, msg, r = HR.cmp_bounded(got[m], ref[m], HR.score_tol(x, ref)[m])
        assert ok, (s, msg)
        worst = max(worst, r)
    assert 0 < worst < 1


def test_tolerance_score_reduce_and_linear_narrow(pool):
    specs = [s for s in HR.score_reduce_specs() if s["cls"] == "C" and s["mode"] == 0]
    assert len(specs) >= 20
    for s in specs:
        sc = HR.score_reduce_make(s, pool, CPU)
        lo = 0
        for n in s["rows"]:
            part = sc[lo:lo + n]
            ok, msg, _ = HR.cmp_bounded(part.mean(0), HR.score_reduce64(part, 0), TR.bound(part.to(F64).abs().sum(0) / n, n + 1))
            assert ok, (s, msg)
            assert torch.equal(part.max(0).values.to(F64), HR.score_reduce64(part, 1))
            lo += n
    specs = [s for s in HR.linear_narrow_specs() if s["cls"] == "C"]
    assert len(specs) >= 40
    for s in specs:
        x, w, bias = HR.linear_narrow_make(s, pool, CPU)
        y, maj = HR.linear_narrow64(x, w, bias, s["relu"])
        got = F.linear(x, w, bias)
        ok, msg, _ = HR.cmp_bounded(F.relu(got) if s["relu"] else got, y, TR.bound(maj, s["C"] + 2))
        assert ok, (s, msg)


def test_tolerance_nlb(pool, hw):
    p32 = {k: v.to(F32) for k, v in hw["p"].items()}
    worst = dict(out=0.0, att=0.0, z=0.0)
    specs = HR.nlb_specs()
    assert len(specs) >= 100
    seen = set()
    for s in specs:
        flat, off, t_st, s_st = HR.nlb_make(s, pool, CPU)
        rows = [r for r in TR.seq_rows(flat[off:].clone(), t_st, s_st, s["lens"], s["S"], s["Tmax"]) if r.shape[0] > 0]
        seen.update(r.shape[0] for r in rows)
        res = HR.nlb_attnpool64(rows, hw["p"], s["use_nlb"])
        for x, r in zip(rows, res):
            z = OH.nlb_closed_form(x, p32) if HR.nlb_applies(s["use_nlb"], x.shape[0]) else x
            o, a = OH.attention_pool(z, p32)
            for k, got in (("out", o), ("att", a[:, 0]), ("z", z)):
                assert got.dtype == F32
                ok, msg, ratio = HR.cmp_bounded(got, r[k], r["d_" + k])
                assert ok, (s, k, msg)
                worst[k] = max(worst[k], ratio)
    assert seen >= set(HR.NLB_LENS[1:]) | {97, 130}, sorted(seen)        # every edge length occurs as a live sequence
    print("fp32 oracle / bound:", worst)
    assert all(0 < v < 1 for v in worst.values()), worst
    # the measured constant of the block stage: fp32 was at most 3.44e-5 of the propagated worst-case bound on Z when it was
    # measured, and the sweep allows 4 x that (another BLAS may sum in another order: only "inside the allowance" is asserted)
    assert HR.NLB_BLOCK_RHO == 4 * 3.44e-5
    print(f"fp32 oracle error / propagated bound on Z: {worst['z'] * HR.NLB_BLOCK_RHO:.3e}")


def test_case_lists_cover_the_edges():
    ps = HR.pair_logits_specs()
    assert {s["D"] for s in ps} == {32, 64, 96, 256, 1024}
    assert {(s["Q"], s["G"]) for s in ps} >= {(q, g) for q in (1, 15, 16, 17, 31, 32, 33, 70)
                                              for g in (1, 31, 32, 63, 64, 65, 127, 128, 129, 333)}
    assert {s["Q"] * s["G"] for s in ps} >= {(1 << 20) - 128, 1 << 20, (1 << 20) - 1}
    rs = HR.rank_specs()
    assert {s["G"] for s in rs} == {1, 2, 255, 256, 257, 511, 513, 1000, 5000} and {s["Q"] for s in rs} == {1, 3, 64}
    assert {s["k"] for s in rs} >= {1, 2, 255, 256} and all(1 <= s["k"] <= min(s["G"], 256) for s in rs)
    fs = HR.pair_topk_specs()
    assert {s["G"] for s in fs} == {1, 5, 255, 256, 257, 258, 300, 511, 513, 1030} and {s["k"] for s in fs} == {1, 2, 5, 64, 255, 256}
    assert any(s["G"] % 256 and s["G"] % 256 < s["k"] and s["G"] > 256 for s in fs)      # a last segment shorter than k
    ms = HR.pair_topk_mfma_specs()
    assert len(ms) >= 16 and {s["G"] for s in ms} == {8192, 8193, 8447, 9001} and {s["Q"] for s in ms} == {1, 33, 256, 257}
    assert {s["k"] for s in ms} == {1, 20, 64} and {s["flags"] for s in ms} == {0, 1} and {s["cls"] for s in ms} == {"I", "C", "CN"}
    bs = HR.blockdiag_specs()
    assert {n for s in bs for n in s["n"]} == {0, 1, 15, 16, 17, 63, 64, 65, 150} and {s["D"] for s in bs} == {32, 256}
    ss = HR.score_reduce_specs()
    assert {s["rows"][0] for s in ss} == {1, 2, 7, 100} and {len(s["rows"]) for s in ss} == {1, 3, 40}
    ns = HR.nlb_specs()
    assert {s["S"] for s in ns} == {1, 2, 5, 37} and {s["pad"] for s in ns} == {0, 4, 260} and {s["use_nlb"] for s in ns} == {0, 1, 2}
    assert {(s["att"], s["z"]) for s in ns} == {(a, z) for a in (False, True) for z in (False, True)}
    assert any(max(s["lens"]) > s["Tmax"] for s in ns) and any(min(s["lens"]) < 0 for s in ns)
    assert any(s["S"] == 1 and s["lens"][0] > s["Tmax"] for s in ns) and any(s["S"] == 1 and s["lens"][0] < 0 for s in ns)
    ls = HR.linear_narrow_specs()
    assert {s["C"] for s in ls} == {16, 32, 240, 256} and {s["K"] for s in ls} == {1, 3, 14, 15, 16}
    assert {s["M"] for s in ls} == {1, 15, 16, 17, 63, 65, 4097, 40000}
    for lst in (ps, rs, fs, bs, ss, ns, ls):
        assert len(lst) >= 100


# ------------------------------------------------------------------------------------------------ the top-k capacity (host side)
def test_topk_capacity_is_refused_before_any_launch():
    """k above seam_rank_topk_max_k(): refused by the C ABI with nothing written, and a ValueError naming the cap from every
    Python entry before anything is allocated or launched (all of it host code: no GPU here)."""
    import ctypes as C
    from seam_match_rcnn_amd import _native, ops, retrieval
    lib = _native.lib()
    cap = int(lib.seam_rank_topk_max_k())
    assert cap == 256 == HR.TOPK_CAP and int(lib.seam_pair_topk_mfma_max_k()) <= cap
    idx = np.full((2, 300), 0x5B5B5B5B5B5B5B5B, dtype=np.int64)
    sc = np.full((2, 300), 3.0e4, dtype=np.float32)
    lg = np.zeros((2, 300, 2), dtype=np.float32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    for g, k in ((300, 257), (300, 300), (5, 6)):                         # host pointers: a refusal never reads them
        assert lib.seam_rank_topk_f32(ptr(lg), ptr(idx), ptr(sc), 2, g, k, None) != 0
        assert lib.seam_pair_topk_f32(ptr(lg), ptr(lg), ptr(lg), ptr(lg), ptr(idx), ptr(sc), 2, g, 32, k, ptr(lg), None) != 0
    assert bool((idx == 0x5B5B5B5B5B5B5B5B).all()) and bool((sc == 3.0e4).all())

    class Agg:                                                              # an aggregator whose kernels must not be reached
        class last:
            weight, bias = torch.zeros((2, 256)), torch.zeros((2,))

        def pair(self, *a):
            raise AssertionError("match_sequences computed the logits before refusing k")

    x, bank = torch.zeros((3, 256)), torch.zeros((1000, 256))
    big = torch.zeros((9000, 256))
    calls = [lambda: ops.rank_topk(torch.zeros((3, 1000, 2)), 500),
             lambda: ops.pair_topk(x, bank, Agg.last.weight, Agg.last.bias, 257),
             lambda: ops.pair_topk(x, bank, Agg.last.weight, Agg.last.bias, 257, fused=True),
             lambda: ops.pair_topk(x, big, Agg.last.weight, Agg.last.bias, 300, mfma=True),
             lambda: ops.pair_topk(x, big, Agg.last.weight, Agg.last.bias, 9000),
             lambda: retrieval.match_sequences(Agg(), x, bank, k=500),
             lambda: retrieval.match_sequences_topk(Agg(), x, bank, k=500)]
    for i, call in enumerate(calls):
        with pytest.raises(ValueError, match=r"capacity of 256 \(seam_rank_topk_max_k\(\)\)"):
            call()
    assert ops._topk_k(500, 200, "x") == 200 and ops._topk_k(256, 1000, "x") == 256        # min(k, G) is what counts
    for fn in (retrieval.match_sequences, retrieval.match_sequences_topk, ops.rank_topk, ops.pair_topk):
        assert "seam_rank_topk_max_k()" in fn.__doc__
