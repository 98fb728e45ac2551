"""Launch wrappers of the match head and the ranking kernels: the non-local block with attention pooling, pair logits and
scores, top-k ranking, tracklets and the score reductions."""
from __future__ import annotations

import ctypes as C
import os as _os
from dataclasses import dataclass
from typing import Optional

import torch

from . import _native
from ._ops_common import F32, _ptr, _req, _stream

__all__ = ["PackedNLB", "nlb_attnpool", "pair_logits", "rank_topk", "match_scores", "pair_scores_blockdiag", "blockdiag_offsets",
           "pair_scores_blockdiag_device", "build_tracklets_max_rows", "build_tracklets", "rank_of", "score_reduce",
           "score_reduce_segments", "rank_of_scores", "pair_topk"]


# ------------------------------------------------------------------------------ SEAM heads
@dataclass
class PackedNLB:
    w_proj_t: torch.Tensor   # [256,384]
    b_proj: torch.Tensor     # [384]
    w_cat: torch.Tensor      # [256]
    w_out_t: torch.Tensor    # [128,256]
    b_out: torch.Tensor      # [256]
    w_att: torch.Tensor      # [256]
    b_att: torch.Tensor      # [1]


NLB_MFMA = _os.environ.get("SEAM_NLB_MFMA", "1") != "0"      # 0: the VALU form of the block for every sequence length


def _nlb_mfma_pack(pk: PackedNLB):
    """Weights of ``seam_nlb_attnpool_mfma_f32`` derived (once per PackedNLB) from the plain pack:
    MFMA B-fragment order of the g and W projections -- element e of lane (h = lane >> 5, n = lane & 31) of fragment
    [n_tile][k / 8] is W[k = 8 j + 4 h + e][32 n_tile + n] -- and the folded theta / phi projections: theta and phi enter the
    block only through a_i = theta_i . wc[:128], b_j = phi_j . wc[128:] (ref models/nlb.py:80-90), i.e. a_i = X_i . u + c with
    u = W_theta^T wc[:128] (folded in fp64, rounded once)."""
    m = getattr(pk, "_mfma", None)
    if m is None:
        wp, bp, wc = pk.w_proj_t.double(), pk.b_proj.double(), pk.w_cat.double()       # [256,384], [384], [256]
        u = (wp[:, :128] @ wc[:128]).float().contiguous()
        v = (wp[:, 128:256] @ wc[128:]).float().contiguous()
        cd = torch.stack([bp[:128] @ wc[:128], bp[128:256] @ wc[128:]]).float().contiguous()
        wg = pk.w_proj_t[:, 256:]                                                        # [256 k, 128 n]
        wg_frag = wg.reshape(32, 2, 4, 4, 32).permute(3, 0, 1, 4, 2).contiguous()       # [nt, j, h, n, e]
        wo_frag = pk.w_out_t.reshape(16, 2, 4, 8, 32).permute(3, 0, 1, 4, 2).contiguous()   # [128 k, 256 n] -> [nt, j, h, n, e]
        m = pk._mfma = (wg_frag, pk.b_proj[256:].contiguous(), u, v, cd, wo_frag)
    return m


def nlb_attnpool(seq: torch.Tensor, t_stride: int, s_stride: int, lens: torch.Tensor, n_seq: int, t_max: int,
                 pk: PackedNLB, use_nlb: bool = True, want_att: bool = False, want_z: bool = False):
    """Batched non-local block + attention pooling.
    Returns (out[S,256], att[S,Tmax] | None) and additionally z[S,Tmax,256] when want_z.
    Sequences of up to ``seam_nlb_mfma_max_len()`` (96) rows run the block's GEMMs on the matrix cores
    (``seam_nlb_attnpool_mfma_f32``); longer ones take the VALU kernel with its global scratch."""
    lib = _native.lib()
    seq = _req(seq, name="seq")
    lens = _req(lens, torch.int32, "lens")
    out = torch.empty((n_seq, 256), dtype=F32, device=seq.device)
    att = torch.zeros((n_seq, t_max), dtype=F32, device=seq.device) if want_att else None
    z = torch.zeros((n_seq, t_max, 256), dtype=F32, device=seq.device) if want_z else None
    if n_seq == 0:
        return (out, att, z) if want_z else (out, att)
    if (NLB_MFMA and t_max <= int(lib.seam_nlb_mfma_max_len()) and t_stride % 4 == 0 and s_stride % 4 == 0
            and seq.data_ptr() % 16 == 0):
        wg_frag, b_g, u, v, cd, wo_frag = _nlb_mfma_pack(pk)
        _native.check(lib.seam_nlb_attnpool_mfma_f32(_ptr(seq), t_stride, s_stride, _ptr(lens), n_seq, t_max, _ptr(wg_frag), _ptr(b_g),
                                                     _ptr(u), _ptr(v), _ptr(cd), _ptr(wo_frag), _ptr(pk.b_out), _ptr(pk.w_att),
                                                     _ptr(pk.b_att), _ptr(out), _ptr(att), _ptr(z), int(use_nlb), _stream()),
                      "seam_nlb_attnpool_mfma_f32")
        return (out, att, z) if want_z else (out, att)
    ws = torch.empty((int(lib.seam_nlb_workspace_floats(n_seq, t_max)),), dtype=F32, device=seq.device)
    _native.check(lib.seam_nlb_attnpool_f32(_ptr(seq), t_stride, s_stride, _ptr(lens), n_seq, t_max, _ptr(pk.w_proj_t),
                                            _ptr(pk.b_proj), _ptr(pk.w_cat), _ptr(pk.w_out_t), _ptr(pk.b_out),
                                            _ptr(pk.w_att), _ptr(pk.b_att), _ptr(out), _ptr(att), _ptr(z), _ptr(ws),
                                            int(use_nlb), _stream()), "seam_nlb_attnpool_f32")
    return (out, att, z) if want_z else (out, att)


def pair_logits(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """a[Q,D], b[G,D], w[2,D], bias[2] -> [Q,G,2]."""
    a, b, w, bias = _req(a), _req(b), _req(w.detach()), _req(bias.detach())
    q, g, d = a.shape[0], b.shape[0], a.shape[1]
    out = torch.empty((q, g, 2), dtype=F32, device=a.device)
    _native.check(_native.lib().seam_pair_logits_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(bias), _ptr(out), q, g, d,
                                                     _stream()), "seam_pair_logits_f32")
    return out


def _topk_k(k: int, g: int, what: str) -> int:
    """min(k, G), refused above the selection's capacity (``seam_rank_topk_max_k()``: the kernels keep their winners on chip).
    Raised before anything is allocated or launched; there is no silent clamp -- a full ranking is what ``rank_of`` gives."""
    k = min(int(k), int(g))
    cap = int(_native.lib().seam_rank_topk_max_k())
    if k > cap:
        raise ValueError(f"{what}: k = {k} exceeds the top-k capacity of {cap} (seam_rank_topk_max_k()); "
                         "use rank_of for positions in the full ranking")
    return k


def rank_topk(logits: torch.Tensor, k: int):
    """logits[Q,G,2] -> (idx int64 [Q,k], score [Q,k]) by descending softmax(x)[...,1].
    min(k, G) <= seam_rank_topk_max_k() (256), else ValueError."""
    k = _topk_k(k, logits.shape[1], "rank_topk")
    logits = _req(logits)
    q, g = logits.shape[0], logits.shape[1]
    idx = torch.empty((q, k), dtype=torch.int64, device=logits.device)
    sc = torch.empty((q, k), dtype=F32, device=logits.device)
    _native.check(_native.lib().seam_rank_topk_f32(_ptr(logits), _ptr(idx), _ptr(sc), q, g, k, _stream()),
                  "seam_rank_topk_f32")
    return idx, sc


def match_scores(logits: torch.Tensor) -> torch.Tensor:
    """logits [...,2] -> softmax(logits)[...,1]."""
    logits = _req(logits)
    out = torch.empty(logits.shape[:-1], dtype=F32, device=logits.device)
    _native.check(_native.lib().seam_match_scores_f32(_ptr(logits), _ptr(out), out.numel(), _stream()),
                  "seam_match_scores_f32")
    return out


def pair_scores_blockdiag(x: torch.Tensor, seg, w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """Self-similarity of every group of rows of ``x`` [rows, D] (groups = consecutive row ranges, boundaries ``seg`` [n_seg + 1]):
    the flat concatenation of the n_s x n_s score blocks, softmax(W (x_i - x_j)^2 + b)[1].  One launch for all groups
    (``seam_pair_scores_blockdiag_f32``); bit-identical to ``match_scores(pair_logits(x_s, x_s))`` per group
    (ref evaluate_movingfashion.py:102-121 ``compute_selfdist``)."""
    import numpy as np
    x = _req(x, name="x")
    seg = np.asarray(seg, dtype=np.int64)
    n = np.diff(seg)
    if len(n) == 0 or int(n.max()) == 0:
        return torch.empty((0,), dtype=F32, device=x.device)
    if seg[0] != 0 or int(seg[-1]) > x.shape[0] or (n < 0).any():
        raise ValueError("pair_scores_blockdiag: seg must be non-decreasing row offsets inside x, starting at 0")
    off = np.concatenate([[0], np.cumsum(n * n)])
    out = torch.empty((int(off[-1]),), dtype=F32, device=x.device)
    seg_d = torch.as_tensor(seg, dtype=torch.int32, device=x.device)
    off_d = torch.as_tensor(off, dtype=torch.int64, device=x.device)
    _native.check(_native.lib().seam_pair_scores_blockdiag_f32(_ptr(x), _ptr(seg_d), _ptr(off_d), _ptr(_req(w, name="w")), _ptr(_req(bias, name="bias")),
                                                               _ptr(out), len(n), int(n.max()), x.shape[1], _stream()),
                  "seam_pair_scores_blockdiag_f32")
    return out


def blockdiag_offsets(seg, device):
    """The two offset tables ``seam_pair_scores_blockdiag_f32`` and ``seam_build_tracklets_f32`` share, from host row offsets
    ``seg`` [n_seg + 1]: (seg int32 [n_seg + 1], out_off int64 [n_seg + 1] = running sum of n_s^2) on ``device``."""
    import numpy as np
    seg = np.asarray(seg, dtype=np.int64)
    n = np.diff(seg)
    off = np.concatenate([[0], np.cumsum(n * n)])
    return torch.as_tensor(seg, dtype=torch.int32, device=device), torch.as_tensor(off, dtype=torch.int64, device=device)


def pair_scores_blockdiag_device(x: torch.Tensor, seg: torch.Tensor, out_off: torch.Tensor, n_out: int, max_rows: int,
                                 w: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """``pair_scores_blockdiag`` with the offset tables already on the device (int32 ``seg``, int64 ``out_off``, as
    ``blockdiag_offsets`` forms them) and nothing read back: ``n_out`` floats are allocated (>= out_off[-1]; what lies behind
    out_off[-1] is not written) and ``max_rows`` bounds every group from above."""
    x = _req(x, name="x")
    seg, out_off = _req(seg, torch.int32, "seg"), _req(out_off, torch.int64, "out_off")
    out = torch.empty((int(n_out),), dtype=F32, device=x.device)
    if seg.numel() > 1 and max_rows > 0:
        _native.check(_native.lib().seam_pair_scores_blockdiag_f32(_ptr(x), _ptr(seg), _ptr(out_off), _ptr(_req(w, name="w")),
                                                                   _ptr(_req(bias, name="bias")), _ptr(out), seg.numel() - 1,
                                                                   int(max_rows), x.shape[1], _stream()),
                      "seam_pair_scores_blockdiag_f32")
    return out


def build_tracklets_max_rows() -> int:
    return int(_native.lib().seam_build_tracklets_max_rows())


def build_tracklets(blocks: torch.Tensor, out_off, seg, imgs: torch.Tensor, scores: torch.Tensor, threshold: float,
                    max_rows: Optional[int] = None):
    """Greedy tracklet linking of every segment in one launch (``seam_build_tracklets_f32``; the device twin of
    ``evaluator.build_tracklets_batch``): ``blocks`` as ``pair_scores_blockdiag`` returns them, ``imgs`` int32 [rows] frame labels
    (compared for equality only), ``scores`` fp32 [rows] confidences, all on the device.
    -> (members, track_len, n_tracks, track_of) int32 device tensors in the host helper's layout ([rows], [rows], [n_seg], [rows]).

    ``seg`` / ``out_off``: the host row offsets ``pair_scores_blockdiag`` took (``out_off`` may then be None: it is their running
    sum of squares), or the device tables of ``blockdiag_offsets``.  With device tables nothing here knows the segment sizes, so
    ``max_rows`` (an upper bound of every segment) must be passed; a longer segment then comes back with n_tracks[s] = -1.  With
    host offsets an oversized segment raises ValueError before anything is launched.  No host synchronisation either way."""
    import numpy as np
    cap = build_tracklets_max_rows()
    blocks, imgs, scores = _req(blocks, name="blocks"), _req(imgs, torch.int32, "imgs"), _req(scores, name="scores")
    dev = blocks.device
    if isinstance(seg, torch.Tensor) and seg.is_cuda:
        if max_rows is None or not isinstance(out_off, torch.Tensor):
            raise ValueError("build_tracklets: device offset tables need out_off on the device and max_rows (reading the segment "
                             "sizes back would be a host synchronisation)")
        seg_d, off_d = _req(seg, torch.int32, "seg"), _req(out_off, torch.int64, "out_off")
        max_rows = int(max_rows)
    else:
        seg_h = np.asarray(seg.numpy() if isinstance(seg, torch.Tensor) else seg, dtype=np.int64)
        n = np.diff(seg_h)
        if len(seg_h) < 1 or (len(n) and (seg_h[0] != 0 or (n < 0).any())):
            raise ValueError("build_tracklets: seg must be non-decreasing row offsets starting at 0")
        if len(n) and int(seg_h[-1]) != imgs.numel():
            raise ValueError(f"build_tracklets: seg ends at {int(seg_h[-1])} but imgs holds {imgs.numel()} detections")
        max_rows = int(n.max()) if len(n) else 0
        seg_d, off_d = blockdiag_offsets(seg_h, dev)
        if isinstance(out_off, torch.Tensor) and out_off.is_cuda:
            off_d = _req(out_off, torch.int64, "out_off")
        if len(n) and blocks.numel() != int((n * n).sum()):
            raise ValueError(f"build_tracklets: blocks holds {blocks.numel()} scores, the segments need {int((n * n).sum())}")
    if max_rows > cap:
        raise ValueError(f"build_tracklets: a segment of {max_rows} detections exceeds the linker's cap of {cap} "
                         "(seam_build_tracklets_max_rows())")
    rows, n_seg = imgs.numel(), seg_d.numel() - 1
    if scores.numel() != rows:
        raise ValueError("build_tracklets: scores must hold one confidence per detection")
    out = torch.empty((3 * rows + max(n_seg, 0),), dtype=torch.int32, device=dev)
    members, track_len, track_of, n_tracks = out[:rows], out[rows:2 * rows], out[2 * rows:3 * rows], out[3 * rows:]
    if n_seg > 0:
        _native.check(_native.lib().seam_build_tracklets_f32(_ptr(blocks), _ptr(off_d), _ptr(seg_d), _ptr(imgs), _ptr(scores), n_seg,
                                                             max_rows, float(threshold), _ptr(members), _ptr(track_len), _ptr(n_tracks),
                                                             _ptr(track_of), _stream()), "seam_build_tracklets_f32")
    return members, track_len, n_tracks, track_of


def rank_of(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """logits [Q,G,2], target int64 [Q] -> rank int64 [Q] of the target product in each query's ranking."""
    logits, target = _req(logits), _req(target, torch.int64, "target")
    q, g = logits.shape[0], logits.shape[1]
    out = torch.empty((q,), dtype=torch.int64, device=logits.device)
    _native.check(_native.lib().seam_rank_of_f32(_ptr(logits), _ptr(target), _ptr(out), q, g, _stream()), "seam_rank_of_f32")
    return out


def score_reduce(score: torch.Tensor, mode: str) -> torch.Tensor:
    """score [n,G] -> [G]: column mean (``"mean"``) or max (``"max"``)."""
    score = _req(score)
    n, g = score.shape
    out = torch.empty((g,), dtype=F32, device=score.device)
    _native.check(_native.lib().seam_score_reduce_f32(_ptr(score), _ptr(out), n, g, {"mean": 0, "max": 1}[mode], _stream()),
                  "seam_score_reduce_f32")
    return out


def score_reduce_segments(score: torch.Tensor, seg: torch.Tensor, mode: str) -> torch.Tensor:
    """score [N,G], seg [P+1] int32 row offsets (device) -> [P,G]: ``score_reduce`` of the rows seg[p]:seg[p+1] of every segment in
    ONE launch (the same sequential row order per column: bit-identical to P separate calls)."""
    score = _req(score)
    seg = _req(seg, torch.int32, "seg")
    n, g = score.shape
    p = seg.numel() - 1
    out = torch.empty((p, g), dtype=F32, device=score.device)
    _native.check(_native.lib().seam_score_reduce_seg_f32(_ptr(score), _ptr(seg), _ptr(out), p, g, {"mean": 0, "max": 1}[mode], _stream()),
                  "seam_score_reduce_seg_f32")
    return out


def rank_of_scores(score: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """score [Q,G], target int64 [Q] -> rank int64 [Q] of the target in each row's descending order."""
    score, target = _req(score), _req(target, torch.int64, "target")
    q, g = score.shape
    out = torch.empty((q,), dtype=torch.int64, device=score.device)
    _native.check(_native.lib().seam_rank_of_scores_f32(_ptr(score), _ptr(target), _ptr(out), q, g, _stream()),
                  "seam_rank_of_scores_f32")
    return out


PAIR_MFMA = True       # large banks: candidates on the fp32 matrix cores (seam_pair_topk_mfma_f32); False: the chunked VALU path


def pair_topk(a: torch.Tensor, b: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, k: int, fused: bool = False,
              q_chunk: int = 64, mfma: Optional[bool] = None, stats: Optional[torch.Tensor] = None, force_exact: bool = False):
    """a13+a14 without materialising the full [Q,G,2] logits -> (idx int64 [Q,k], score [Q,k]).  Three implementations with
    bit-identical results:

    * ``mfma`` (default when the bank has >= seam_pair_topk_mfma_min_gallery() rows, D == 256, k <= 64): seam_pair_topk_mfma_f32 --
      the logit-difference GEMM on the fp32 matrix cores finds candidates, the winners are re-scored with the direct form and a
      per-query error bound proves the top k (``stats``: optional int32[4] device tensor that receives [queries redone with the
      direct form, largest candidate list, overflowed lists, 0]; ``force_exact``: test hook, every query takes the direct form);
    * query chunks of ``q_chunk`` through seam_pair_logits_f32 + seam_rank_topk_f32 with one reused logits buffer (small banks);
    * ``fused=True``: seam_pair_topk_f32, the single-pass VALU kernel.

    Every branch: min(k, G) <= seam_rank_topk_max_k() (256), else ValueError before anything is allocated or launched."""
    lib = _native.lib()
    k = _topk_k(k, b.shape[0], "pair_topk")
    a, b, w, bias = _req(a), _req(b), _req(w.detach()), _req(bias.detach())
    q, g, d = a.shape[0], b.shape[0], a.shape[1]
    idx = torch.empty((q, k), dtype=torch.int64, device=a.device)
    sc = torch.empty((q, k), dtype=F32, device=a.device)
    can_mfma = d == 256 and g >= lib.seam_pair_topk_mfma_min_gallery() and 0 < k <= lib.seam_pair_topk_mfma_max_k() and q > 0
    if mfma is None:
        mfma = PAIR_MFMA and can_mfma and not fused
    if mfma:
        if not can_mfma:
            raise ValueError(f"pair_topk(mfma=True) needs D == 256, G >= {lib.seam_pair_topk_mfma_min_gallery()} and "
                             f"k <= {lib.seam_pair_topk_mfma_max_k()} (got D={d}, G={g}, k={k})")
        ws = torch.empty((int(lib.seam_pair_topk_mfma_workspace_floats(q, g, k)),), dtype=F32, device=a.device)
        if stats is not None:
            stats = _req(stats, torch.int32, "stats")
        _native.check(lib.seam_pair_topk_mfma_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(bias), _ptr(idx), _ptr(sc), q, g, d, k, _ptr(ws),
                                                  1 if force_exact else 0, _ptr(stats) if stats is not None else None, _stream()),
                      "seam_pair_topk_mfma_f32")
        return idx, sc
    if fused:
        ws = torch.empty((int(lib.seam_pair_topk_workspace_floats(q, g, k)),), dtype=F32, device=a.device)
        _native.check(lib.seam_pair_topk_f32(_ptr(a), _ptr(b), _ptr(w), _ptr(bias), _ptr(idx), _ptr(sc), q, g, d, k,
                                             _ptr(ws), _stream()), "seam_pair_topk_f32")
        return idx, sc
    buf = torch.empty((min(q, q_chunk), g, 2), dtype=F32, device=a.device)
    for s0 in range(0, q, q_chunk):
        n = min(q_chunk, q - s0)
        _native.check(lib.seam_pair_logits_f32(C.c_void_p(a[s0:].data_ptr()), _ptr(b), _ptr(w), _ptr(bias), _ptr(buf), n, g, d,
                                               _stream()), "seam_pair_logits_f32")
        _native.check(lib.seam_rank_topk_f32(_ptr(buf), C.c_void_p(idx[s0:].data_ptr()), C.c_void_p(sc[s0:].data_ptr()), n, g,
                                             k, _stream()), "seam_rank_topk_f32")
    return idx, sc
