"""seam_build_tracklets_f32 (the device linker, one block per segment) against the two host forms of the same greedy linking:
``evaluator.build_tracklets`` (pinned to the reference's loops by tests/test_evaluator.py) and ``evaluator.build_tracklets_batch``
(the native host helper).  Exact list equality: the decisions are comparisons only.  Every launch writes into buffers pre-filled
with a poison value, with guard words in front and behind."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

POISON = -7777
GUARD = 8


def _dev():
    return torch.device("cuda:0")


def _P(t):
    return C.c_void_p(t.data_ptr())


def _pack(segments):
    """[(sim [n,n], imgs [n], scores [n])] -> blocks, seg, imgs, scores as flat host arrays."""
    seg = np.concatenate([[0], np.cumsum([len(i) for _, i, _ in segments])]).astype(np.int64)
    blocks = np.concatenate([np.asarray(s, np.float32).reshape(-1) for s, _, _ in segments] + [np.zeros(0, np.float32)])
    imgs = np.concatenate([np.asarray(i, np.int64) for _, i, _ in segments] + [np.zeros(0, np.int64)])
    scores = np.concatenate([np.asarray(c, np.float32) for _, _, c in segments] + [np.zeros(0, np.float32)])
    return blocks, seg, imgs, scores


def _lists(members, lens, ntr, seg):
    out = []
    for s in range(len(seg) - 1):
        o, tracks, mo = int(seg[s]), [], 0
        for k in range(int(ntr[s])):
            ln = int(lens[o + k])
            tracks.append([int(m) for m in members[o + mo:o + mo + ln]])
            mo += ln
        out.append(tracks)
    return out


def launch(segments, thr, max_rows=None):
    """One raw launch into poisoned, guarded buffers -> (rc, members, track_len, n_tracks, track_of) as host arrays (guards
    checked and stripped)."""
    from seam_match_rcnn_amd import _native, ops
    dev = _dev()
    blocks, seg, imgs, scores = _pack(segments)
    rows, n_seg = int(seg[-1]), len(seg) - 1
    seg_d, off_d = ops.blockdiag_offsets(seg, dev)
    b_d = torch.from_numpy(blocks).to(dev)
    i_d = torch.from_numpy(imgs.astype(np.int32)).to(dev)
    s_d = torch.from_numpy(scores).to(dev)
    bufs = [torch.full((n + 2 * GUARD,), POISON, dtype=torch.int32, device=dev) for n in (rows, rows, n_seg, rows)]
    ptr = [C.c_void_p(b.data_ptr() + 4 * GUARD) for b in bufs]
    if max_rows is None:
        max_rows = int(np.diff(seg).max()) if n_seg else 0
    rc = _native.lib().seam_build_tracklets_f32(_P(b_d), _P(off_d), _P(seg_d), _P(i_d), _P(s_d), n_seg, max_rows, float(thr),
                                                ptr[0], ptr[1], ptr[2], ptr[3], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = [b.cpu().numpy() for b in bufs]
    for h in host:
        assert (h[:GUARD] == POISON).all() and (h[len(h) - GUARD:] == POISON).all(), "a guard word was overwritten"
    return (rc,) + tuple(h[GUARD:len(h) - GUARD] for h in host)


def check(segments, thr, references=("python", "native")):
    """Device lists == both host forms; every output element written; track_of consistent with the lists."""
    from seam_match_rcnn_amd import evaluator as EV
    blocks, seg, imgs, scores = _pack(segments)
    rc, members, lens, ntr, track_of = launch(segments, thr)
    assert rc == 0
    assert (members != POISON).all() and (lens != POISON).all() and (ntr != POISON).all() and (track_of != POISON).all()
    got = _lists(members, lens, ntr, seg)
    if "python" in references:
        want = [EV.build_tracklets(np.asarray(s, np.float32).reshape(len(i), len(i)), np.asarray(i), np.asarray(c, np.float32), thr)
                for s, i, c in segments]
        assert got == want
    if "native" in references:
        assert got == EV.build_tracklets_batch(blocks, seg, imgs, scores, thr)
    for s, tracks in enumerate(got):
        o, n = int(seg[s]), int(seg[s + 1] - seg[s])
        assert sorted(m for t in tracks for m in t) == list(range(n))                  # a partition
        assert lens[o:o + n].tolist() == [len(t) for t in tracks] + [0] * (n - len(tracks))
        for k, t in enumerate(tracks):
            assert all(track_of[o + m] == k for m in t)
    return got


KNOWN_IMGS = [0, 0, 1, 2]
KNOWN_SCORES = [0.9, 0.4, 0.5, 0.6]
KNOWN_SIM = [[1, .1, .8, .2], [.1, 1, .1, .7], [.8, .1, 1, .1], [.2, .7, .1, 1]]


def test_one_detection():
    assert check([([[1.0]], [0], [0.5])], 0.3) == [[[0]]]


def test_two_detections_in_one_frame_are_two_tracklets():
    assert check([([[1, .9], [.9, 1]], [4, 4], [0.2, 0.8])], 0.3) == [[[1], [0]]]


@pytest.mark.parametrize("thr,want", [(0.3, [[0, 2], [3, 1]]), (0.9, [[0], [3], [2], [1]])])
def test_known_answer(thr, want):
    assert check([(KNOWN_SIM, KNOWN_IMGS, KNOWN_SCORES)], thr) == [want]


def test_chain_links_through_a_later_member():
    # 0 seeds; 2 is only similar to 1, which is only similar to 0: similarity to ANY member
    sim = np.full((3, 3), 0.1, np.float32)
    sim[0, 1] = sim[1, 0] = 0.8
    sim[1, 2] = sim[2, 1] = 0.7
    assert check([(sim, [0, 1, 2], [0.9, 0.5, 0.4])], 0.3) == [[[0, 1, 2]]]


def test_tie_is_broken_by_ascending_member_row_not_link_order():
    # 3 seeds, 0 links next: members in link order [3, 0].  sim[0][2] == sim[3][1] is the maximum over the candidates 1, 2:
    # rows in ascending detection order put row 0 first, so detection 2 is picked (link order would pick 1).
    sim = np.zeros((4, 4), np.float32)
    sim[3, 0] = 0.9
    sim[0, 2] = sim[3, 1] = 0.6
    got = check([(sim, [0, 1, 2, 3], [0.1, 0.2, 0.3, 0.9])], 0.3)
    assert got[0][0][:3] == [3, 0, 2]


def test_similarity_equal_to_the_threshold_does_not_link():
    assert check([([[1, .5], [.5, 1]], [0, 1], [0.9, 0.1])], 0.5) == [[[0], [1]]]


def test_float32_of_the_threshold_links_in_fp64():
    """np.float32(0.3) = 0.300000011920929 exceeds the double 0.3: the device linker compares in fp64 and links.  The Python form
    takes that decision on the same VALUES held in a float64 matrix; on a float32 matrix NumPy 2 rounds the threshold to fp32 first
    (as the native host helper does with ``(float)threshold``), and those two forms do not link -- that difference is the one this
    case exists for, so the native helper is not consulted here."""
    from seam_match_rcnn_amd import evaluator as EV
    v = float(np.float32(0.3))
    assert v > 0.3
    sim = np.array([[1, v], [v, 1]], np.float32)
    assert float(sim[0, 1]) == v
    assert check([(sim, [0, 1], [0.9, 0.1])], 0.3, references=()) == [[[0, 1]]]
    assert EV.build_tracklets(sim.astype(np.float64), np.array([0, 1]), np.array([0.9, 0.1], np.float32), 0.3) == [[0, 1]]


def test_equal_confidences_seed_the_lowest_index():
    sim = np.eye(3, dtype=np.float32)
    assert check([(sim, [0, 1, 2], [0.5, 0.5, 0.5])], 0.3) == [[[0], [1], [2]]]


def test_empty_segment_between_two():
    z = (np.zeros((0, 0), np.float32), [], [])
    got = check([(KNOWN_SIM, KNOWN_IMGS, KNOWN_SCORES), z, ([[1, .9], [.9, 1]], [0, 1], [0.3, 0.6])], 0.3)
    assert got == [[[0, 2], [3, 1]], [], [[1, 0]]]


def test_sparse_frame_labels():
    sim = np.array([[1, .8, .7, .6], [.8, 1, .9, .5], [.7, .9, 1, .4], [.6, .5, .4, 1]], np.float32)
    assert check([(sim, [0, 7, 7, 1000], [0.9, 0.8, 0.7, 0.6])], 0.3) == [[[0, 1, 3], [2]]]


def test_asymmetric_matrix_reads_member_row_candidate_column():
    # sim[0][1] links, sim[1][0] would not
    sim = np.array([[1, .8], [.1, 1]], np.float32)
    assert check([(sim, [0, 1], [0.9, 0.1])], 0.3) == [[[0, 1]]]
    assert check([(sim.T.copy(), [0, 1], [0.9, 0.1])], 0.3) == [[[0], [1]]]


def _seeded_segments():
    rng = np.random.default_rng(2024)
    segs = []
    for n in (1, 2, 17, 64, 65, 300):
        imgs = rng.integers(0, 12, n)
        sim = np.round(rng.uniform(0, 1, (n, n)) * 8) / 8
        sc = np.round(rng.uniform(0, 1, n) * 8) / 8
        segs.append((sim.astype(np.float32), imgs, sc.astype(np.float32)))
    return segs


@pytest.mark.parametrize("thr", [0.3, 0.7])
def test_seeded_segments_in_one_launch(thr):
    got = check(_seeded_segments(), thr)
    assert [sum(len(t) for t in tr) for tr in got] == [1, 2, 17, 64, 65, 300]


def test_oversized_segment_is_refused_with_the_poison_intact():
    from seam_match_rcnn_amd import ops
    cap = ops.build_tracklets_max_rows()
    assert cap >= 1024
    n = cap + 1
    dev = _dev()
    segs = [(np.zeros((n, n), np.float32), np.arange(n) % 7, np.zeros(n, np.float32))]
    rc, members, lens, ntr, track_of = launch(segs, 0.3)
    assert rc != 0
    for a in (members, lens, ntr, track_of):
        assert (a == POISON).all()
    # the launcher's other refusals, and a segment above max_rows inside an accepted launch
    rc, members, lens, ntr, track_of = launch([(KNOWN_SIM, KNOWN_IMGS, KNOWN_SCORES), ([[1.0]], [0], [0.5])], 0.3, max_rows=3)
    assert rc == 0 and ntr.tolist() == [-1, 1]
    assert (members[:4] == POISON).all() and (lens[:4] == POISON).all() and (track_of[:4] == POISON).all()
    assert members[4] == 0 and lens[4] == 1 and track_of[4] == 0
    blocks = torch.zeros(n * n, device=dev)
    seg = np.array([0, n])
    with pytest.raises(ValueError, match=rf"{n} detections.*cap of {cap}"):
        ops.build_tracklets(blocks, None, seg, torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev), 0.3)
    from seam_match_rcnn_amd import _native
    with pytest.raises(_native.SeamNativeError):
        ops.build_tracklets(torch.zeros(1), None, [0, 1], torch.zeros(1, dtype=torch.int32), torch.zeros(1), 0.3)
    lib = _native.lib()
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, -1, 0, 0.3, None, None, None, None, None) != 0
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, 0, 0, 0.3, None, None, None, None, None) == 0
    assert lib.seam_build_tracklets_f32(None, None, None, None, None, 1, 1, 0.3, None, None, None, None, None) != 0
    torch.cuda.synchronize()


def test_blockdiag_into_linker_equals_the_host_route_and_repeats_bit_for_bit():
    """ops.pair_scores_blockdiag -> ops.build_tracklets on seeded descriptors == the evaluator's route (blocks copied to the host,
    build_tracklets_batch) on the same blocks; a second launch on the same inputs gives the same bits."""
    from seam_match_rcnn_amd import evaluator as EV
    from seam_match_rcnn_amd import ops
    dev = _dev()
    rng = np.random.default_rng(9)
    sizes = [5, 0, 23, 1, 70]
    seg = np.concatenate([[0], np.cumsum(sizes)])
    rows = int(seg[-1])
    centres = rng.standard_normal((6, 256))
    x = (centres[rng.integers(0, 6, rows)] + 0.2 * rng.standard_normal((rows, 256))).astype(np.float32)
    w = (rng.standard_normal((2, 256)) * 0.05).astype(np.float32)
    w[1] = -np.abs(w[1])                # a larger distance lowers the match logit
    b = np.array([-1.0, 1.0], np.float32)
    imgs = np.concatenate([rng.integers(0, 10, n) for n in sizes])
    scores = (np.round(rng.uniform(0, 1, rows) * 16) / 16).astype(np.float32)
    x_d, w_d, b_d = (torch.from_numpy(a).to(dev) for a in (x, w, b))
    i_d = torch.from_numpy(imgs.astype(np.int32)).to(dev)
    s_d = torch.from_numpy(scores).to(dev)
    blocks = ops.pair_scores_blockdiag(x_d, seg, w_d, b_d)
    first = ops.build_tracklets(blocks, None, seg, i_d, s_d, 0.3)
    second = ops.build_tracklets(blocks, None, seg, i_d, s_d, 0.3)
    for a, c in zip(first, second):
        assert torch.equal(a, c)
    members, lens, ntr, track_of = (t.cpu().numpy() for t in first)
    got = _lists(members, lens, ntr, seg)
    want = EV.build_tracklets_batch(blocks.cpu().numpy(), seg, imgs, scores, 0.3)
    assert got == want
    assert any(len(t) > 1 for tr in got for t in tr) and any(len(tr) > 1 for tr in got)       # links and splits both occur
    # the device tables of the first launch feed the second form with no conversion
    seg_d, off_d = ops.blockdiag_offsets(seg, dev)
    third = ops.build_tracklets(blocks, off_d, seg_d, i_d, s_d, 0.3, max_rows=max(sizes))
    for a, c in zip(first, third):
        assert torch.equal(a, c)
