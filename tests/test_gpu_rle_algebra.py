"""GPU: the RLE algebra on bitmaps (csrc/seam_rle.hip: bits from runs, combine, count from bits, pair intersections) and what is
built on it -- ``mask_utils.merge`` / ``frPyObjects`` / ``iou`` and ``evaluator_det.evaluate_results`` -- against the host
restatements (tests/rle_algebra_refs.py, mask_refs.py, rle_refs.py).  Everything is exact equality.  Raw C-ABI launches write
into buffers poisoned with 0xA5 behind 1 MiB guards, run twice and must repeat themselves; the tables are packed by this file's
own loops."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_refs as MR                                                  # noqa: E402
import rle_algebra_refs as A                                            # noqa: E402
import rle_refs as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 1 << 20
SHAPES = [(h, w) for h in (1, 31, 32, 33, 65) for w in (1, 2, 7)]


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def poisoned(nbytes):
    raw = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD:GUARD + nbytes]


def untouched(raw, nbytes):
    return bool((raw[:GUARD] == 0xA5).all()) and bool((raw[GUARD + nbytes:] == 0xA5).all())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def cells_of(h, w):
    return ((h + 31) // 32) * w


def pack_bits(mask):
    """uint8 [h,w] -> the bitmap's words, [ceil(h/32)][w], bit r&31 of word [r>>5][c], by plain loops"""
    h, w = mask.shape
    words = np.zeros(cells_of(h, w), np.uint32)
    for r in range(h):
        for c in range(w):
            if mask[r, c]:
                words[(r >> 5) * w + c] |= np.uint32(1 << (r & 31))
    return words


def run_lists(h, w, rng):
    """name -> counts for one shape"""
    n = h * w
    out = {"zeros": [n], "ones": [0, n]}
    if n >= 3:
        out["one_run_across_columns"] = [1, n - 2, 1]                   # starts in column 0, ends in the last one
        out["interior_zero_runs"] = [1, 0, 1, n - 2] if n == 3 else [1, 0, 1, 0, 0, n - 3, 0, 1]
        out["leading_zero_run_and_more"] = [0, 1, 0, 0, n - 1]
    for k in range(3):
        out[f"random_{k}"] = MR.random_counts(rng, h, w, max_runs=10, zero_runs=False)
        out[f"random_zero_runs_{k}"] = MR.random_counts(rng, h, w, max_runs=10, zero_runs=True)
    return out


@pytest.fixture(scope="module")
def objects():
    """(names, counts, (h, w), decoded masks, canonical counts) of every shape x every run list"""
    rng = np.random.default_rng(41)
    names, counts, hws = [], [], []
    for h, w in SHAPES:
        for name, c in run_lists(h, w, rng).items():
            names.append(f"{h}x{w} {name}")
            counts.append(c)
            hws.append((h, w))
    order = rng.permutation(len(names))                                  # sizes mixed within one call
    names, counts, hws = [names[i] for i in order], [counts[i] for i in order], [hws[i] for i in order]
    masks = [MR.rle_decode(c, h, w) for c, (h, w) in zip(counts, hws)]
    return names, counts, hws, masks, [R.rle_encode(m) for m in masks]


class Tables:
    """This file's own packing of a batch of objects: run tables and the bitmap layout."""

    def __init__(self, counts, hws):
        starts, run_off, cell_off = [], [0], [0]
        for c, (h, w) in zip(counts, hws):
            pos = 0
            for v in c:
                starts.append(pos)
                pos += v
            run_off.append(len(starts))
            cell_off.append(cell_off[-1] + cells_of(h, w))
        self.n, self.n_runs, self.cells, self.cell_off = len(hws), len(starts), cell_off[-1], cell_off
        self.hw_host = np.ascontiguousarray(np.asarray(hws, np.int32).reshape(-1, 2))
        self.run_start, self.run_off = up(np.asarray(starts, np.int32)), up(np.asarray(run_off, np.int32))
        self.hw, self.cell = up(self.hw_host), up(np.asarray(cell_off, np.int64))
        self.H = self.hw_host.ctypes.data

    def bits(self, lib):
        ws_raw, ws = poisoned(4 * self.cells)
        rc = lib.seam_rle_bits_from_runs(self.run_start.data_ptr(), self.run_off.data_ptr(), self.n_runs, self.H, self.hw.data_ptr(),
                                         self.cell.data_ptr(), ws.data_ptr(), 4 * self.cells, self.n, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(ws_raw, 4 * self.cells), "wrote outside the workspace"
        return ws_raw, ws

    def to_counts(self, lib, ws, hws):
        """count from bits -> scan -> positions -> counts, every buffer poisoned"""
        ct_raw, ct = poisoned(4 * self.cells)
        rc = lib.seam_rle_count_bits(self.H, self.hw.data_ptr(), self.cell.data_ptr(), ws.data_ptr(), 4 * self.cells, ct.data_ptr(),
                                     self.n, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(ct_raw, 4 * self.cells), "wrote outside the counts"
        scan = torch.cumsum(ct.view(torch.int32), 0)
        ends = [int(v) for v in scan[torch.as_tensor([c - 1 for c in self.cell_off[1:]], device=DEV)].cpu()]
        total = ends[-1]
        ps_raw, ps = poisoned(4 * total)
        rc = lib.seam_rle_positions_masks(self.H, self.hw.data_ptr(), self.cell.data_ptr(), ws.data_ptr(), 4 * self.cells,
                                          scan.data_ptr(), ps.data_ptr() if total else None, total, self.n, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(ps_raw, 4 * total), "wrote outside the positions"
        pos, out, lo = ps.cpu().numpy().view(np.int32), [], 0
        for hi, (h, w) in zip(ends, hws):
            edges = [0] + [int(v) for v in pos[lo:hi]] + [h * w]
            out.append([b - a for a, b in zip(edges, edges[1:])])
            lo = hi
        return out, ct.cpu().numpy().tobytes() + pos.tobytes()


# ------------------------------------------------------------------------------------------------ bits from runs
def test_bits_from_runs_every_shape_and_list_in_one_call(lib, objects):
    names, counts, hws, masks, canon = objects
    t = Tables(counts, hws)
    runs = []
    for _ in range(2):
        _, ws = t.bits(lib)
        got, raw = t.to_counts(lib, ws, hws)
        runs.append((got, ws.cpu().numpy().tobytes() + raw))
    assert runs[0][1] == runs[1][1], "two launches differ"
    bad = [names[i] for i in range(t.n) if runs[0][0][i] != canon[i]]
    assert not bad, bad[:10]
    words = np.frombuffer(runs[0][1][:4 * t.cells], np.uint32)
    for i, (m, (h, w)) in enumerate(zip(masks, hws)):                    # the words themselves; rows at or past h are zero bits
        mine = words[t.cell_off[i]:t.cell_off[i + 1]]
        assert np.array_equal(mine, pack_bits(m)), names[i]
        if h & 31:
            assert not (mine[-w:] >> np.uint32(h & 31)).any(), names[i]


def test_bits_from_runs_every_object_singly(lib, objects):
    names, counts, hws, _, canon = objects
    bad = []
    for i in range(0, len(names), 3):
        t = Tables([counts[i]], [hws[i]])
        _, ws = t.bits(lib)
        if t.to_counts(lib, ws, [hws[i]])[0] != [canon[i]]:
            bad.append(names[i])
    assert not bad, bad[:10]


# ------------------------------------------------------------------------------------------------ merge
def as_rle(counts, h, w, k):
    """an RLE dict in one of the three input forms"""
    if k % 3 == 0:
        return {"size": [h, w], "counts": list(counts)}
    s = MR.rle_to_string(counts)
    return {"size": [h, w], "counts": s if k % 3 == 1 else s.encode("ascii")}


@pytest.mark.parametrize("intersect", [False, True], ids=["union", "intersection"])
def test_merge_equals_the_restated_rle_merge_byte_for_byte(intersect):
    from seam_match_rcnn_amd import mask_utils as M
    rng = np.random.default_rng(5 + intersect)
    for h, w in SHAPES + [(800, 1216)]:
        for n in (1, 2, 9):
            dense = rng.random() < 0.5
            lists = [MR.random_counts(rng, h, w, max_runs=40 if h > 100 else 9, zero_runs=False) for _ in range(n)]
            if dense:                                                    # the other polarity: a leading zero-length run
                lists = [[0] + c if len(c) % 2 else c for c in lists]
            want, wh, ww = A.rle_merge([(c, h, w) for c in lists], intersect)
            if h * w <= 500:                                             # the property the device route relies on, held here too
                m = MR.rle_decode(lists[0], h, w)
                for c in lists[1:]:
                    m = (m & MR.rle_decode(c, h, w)) if intersect else (m | MR.rle_decode(c, h, w))
                assert want == R.rle_encode(m)
            got = M.merge([as_rle(c, h, w, k) for k, c in enumerate(lists)], intersect=intersect)
            assert got == {"size": [wh, ww], "counts": MR.rle_to_string(want).encode("ascii")}, (h, w, n, lists)
            assert isinstance(got["counts"], bytes) and all(v > 0 for v in want[1:])


def test_merge_of_lists_with_zero_runs_is_the_canonical_form_of_the_combined_mask():
    from seam_match_rcnn_amd import mask_utils as M
    rng = np.random.default_rng(77)
    for h, w in [(33, 7), (65, 2), (1, 7)]:
        for intersect in (False, True):
            lists = [MR.random_counts(rng, h, w, max_runs=8, zero_runs=True) for _ in range(4)] + [[1, 0, 1, 0, 0, h * w - 2]]
            m = MR.rle_decode(lists[0], h, w)
            for c in lists[1:]:
                m = (m & MR.rle_decode(c, h, w)) if intersect else (m | MR.rle_decode(c, h, w))
            got = M.merge([as_rle(c, h, w, k) for k, c in enumerate(lists)], intersect)
            assert got == {"size": [h, w], "counts": MR.rle_to_string(R.rle_encode(m)).encode("ascii")}


def test_merge_edges():
    from seam_match_rcnn_amd import mask_utils as M
    assert M.merge([]) == {"size": [0, 0], "counts": b""} == M.merge([], intersect=True)
    with pytest.raises(ValueError):
        M.merge([{"size": [2, 3], "counts": [6]}, {"size": [3, 2], "counts": [6]}])
    with pytest.raises(ValueError):
        M.merge([{"size": [2, 3], "counts": [5]}])                       # counts that do not sum to h*w
    one = {"size": [2, 3], "counts": [1, 0, 1, 4]}                       # one input comes back re-encoded
    assert M.merge([one]) == {"size": [2, 3], "counts": MR.rle_to_string([2, 4]).encode("ascii")} == M.merge(one)


# ------------------------------------------------------------------------------------------------ frPyObjects
def test_fr_py_objects_every_input_form():
    from seam_match_rcnn_amd import mask_utils as M
    h, w = 45, 38
    rng = np.random.default_rng(11)
    boxes = [[2.0, 3.0, 10.0, 20.0], [0.5, 0.25, 7.75, 9.5], [3.3, 7.7, 20.2, 30.9],            # whole and fractional corners
             [-4.0, -2.5, 10.0, 12.0], [30.0, 40.0, 20.0, 20.0], [-6.0, 10.0, 60.0, 5.5],       # partly outside
             [50.0, 60.0, 5.0, 5.0], [-20.0, -20.0, 10.0, 10.0], [0.0, 0.0, 38.0, 45.0], [5.0, 5.0, 0.0, 0.0]]     # outside, all, empty
    polys = [MR.random_polygon(rng, h, w, max_pts=7) for _ in range(6)]
    polys = [p if len(p) > 4 else p + [float(w), float(h), 0.0, float(h)] for p in polys]        # a 4-list would be a box
    uncs = [{"size": [h, w], "counts": MR.random_counts(rng, h, w, zero_runs=z)} for z in (False, True, False)]

    def same(got, want_counts):
        return got["size"] == [h, w] and isinstance(got["counts"], bytes) and M.rle_from_string(got["counts"]) == [int(v) for v in want_counts]

    forms = [np.asarray(boxes, np.float64), [list(b) for b in boxes], [list(p) for p in polys], list(uncs)]
    for form in forms:
        got, want = M.frPyObjects(form, h, w), A.fr_py_objects(form, h, w)
        assert isinstance(got, list) and len(got) == len(want) == len(form)
        assert all(same(g, c) for g, c in zip(got, want)), [i for i, (g, c) in enumerate(zip(got, want)) if not same(g, c)]
    for single in (boxes[1], polys[0], uncs[0]):
        got = M.frPyObjects(single, h, w)
        assert isinstance(got, dict) and same(got, A.fr_py_objects(single, h, w))
    areas = M.area(M.frPyObjects(np.asarray(boxes), h, w)).tolist()
    assert areas[0] == 200 and areas[6] == 0 and areas[7] == 0 and areas[8] == h * w and areas[9] == 0 and 0 < areas[3] < 120
    two = M.frPyObjects([polys[0], polys[1]], h, w)                      # polygons are not merged
    assert len(two) == 2 and [M.rle_from_string(r["counts"]) for r in two] == [A.rle_fr_poly(polys[0], h, w), A.rle_fr_poly(polys[1], h, w)]
    with pytest.raises(ValueError):
        M.frPyObjects("nothing", h, w)
    with pytest.raises(ValueError):
        M.frPyObjects([{"size": [h, w + 1], "counts": [h * (w + 1)]}], h, w)
    m = MR.poly_mask([polys[2]], h, w)
    assert M.annToRLE({"segmentation": [polys[2]]}, [h, w]) == M.encode(m) == M.frPyObjects(polys[2], h, w)     # annToRLE keeps its results


# ------------------------------------------------------------------------------------------------ iou
@pytest.mark.parametrize("dg", [(0, 3), (3, 0), (1, 1), (5, 4)], ids=lambda v: f"{v[0]}x{v[1]}")
def test_iou_equals_the_restatement_and_the_dense_route(dg):
    from seam_match_rcnn_amd import mask_utils as M
    nd, ng = dg
    h, w = 33, 7
    rng = np.random.default_rng(100 + 10 * nd + ng)
    dt = [MR.random_counts(rng, h, w, max_runs=9, zero_runs=bool(k % 2)) for k in range(nd)]
    gt = [MR.random_counts(rng, h, w, max_runs=9, zero_runs=bool(k % 2)) for k in range(ng)]
    if nd == 5:
        dt[0] = [5, 100, h * w - 105]
        dt[3], gt[1], gt[2] = [h * w], [0, h * w], list(dt[0])           # an empty detection, a full and an identical ground truth
    crowd = [(k % 2) for k in range(ng)]
    got = M.iou([as_rle(c, h, w, k) for k, c in enumerate(dt)], [as_rle(c, h, w, k + 1) for k, c in enumerate(gt)], crowd)
    want = A.mask_iou(dt, gt, h, w, crowd)
    assert got.dtype == np.float64 and got.shape == (nd, ng) and np.array_equal(got, want)
    if nd and ng:                                                        # the dense route: torch on decoded masks
        dm = torch.from_numpy(np.stack([MR.rle_decode(c, h, w) for c in dt])).to(DEV) != 0
        gm = torch.from_numpy(np.stack([MR.rle_decode(c, h, w) for c in gt])).to(DEV) != 0
        inter = (dm[:, None] & gm[None]).sum((2, 3)).to(torch.float64)
        da, ga = dm.sum((1, 2)).to(torch.float64)[:, None], gm.sum((1, 2)).to(torch.float64)[None]
        den = torch.where(torch.tensor(crowd, device=DEV, dtype=torch.bool)[None], da.expand_as(inter), da + ga - inter)
        dense = torch.where(den == 0, torch.zeros_like(inter), inter / den).cpu().numpy()
        assert np.array_equal(got, dense)
    if nd == 5:
        assert got[0, 2] == 1.0 and not got[3].any()
        with pytest.raises(ValueError):
            M.iou([as_rle(dt[0], h, w, 0)], [{"size": [w, h], "counts": [h * w]}], [0])


def test_iou_in_chunks_gives_the_same_table(monkeypatch):
    from seam_match_rcnn_amd import mask_utils as M
    from seam_match_rcnn_amd import ops, ops_masks
    h, w = 65, 7
    rng = np.random.default_rng(8)
    dt = [{"size": [h, w], "counts": MR.random_counts(rng, h, w, zero_runs=False)} for _ in range(7)]
    gt = [{"size": [h, w], "counts": MR.random_counts(rng, h, w, zero_runs=False)} for _ in range(3)]
    whole = M.iou(dt, gt, [0, 1, 0])
    monkeypatch.setattr(ops_masks, "RLE_BITS_BUDGET_BYTES", 4 * cells_of(h, w) * 5)      # two detections per chunk beside the ground truths
    assert ops.budget_chunks([10, 10, 10, 50, 10], 25) == [(0, 2), (2, 3), (3, 4), (4, 5)]
    assert np.array_equal(M.iou(dt, gt, [0, 1, 0]), whole) and whole.any()


# ------------------------------------------------------------------------------------------------ the pair kernel through the ABI
def test_pair_intersections_span_two_images_and_refusals_leave_the_poison(lib):
    rng = np.random.default_rng(3)
    hws = [(33, 7)] * 4 + [(65, 2)] * 3                                  # image 0: objects 0..3, image 1: objects 4..6
    counts = [MR.random_counts(rng, h, w, max_runs=7, zero_runs=True) for h, w in hws]
    counts[1], counts[5], counts[4], counts[6] = [0, 33 * 7], [65 * 2], [50, 60, 20], [3, 100, 27]
    masks = [MR.rle_decode(c, h, w) != 0 for c, (h, w) in zip(counts, hws)]
    pairs = [(0, 1), (0, 2), (3, 0), (1, 1), (2, 3), (4, 5), (4, 6), (6, 4), (6, 6), (1, 2)]
    want = [int((masks[a] & masks[b]).sum()) for a, b in pairs]
    t = Tables(counts, hws)
    _, ws = t.bits(lib)
    d_pairs, P = up(np.asarray(pairs, np.int32)), len(pairs)
    runs = []
    for _ in range(2):
        in_raw, inter = poisoned(8 * P)
        ar_raw, area = poisoned(8 * t.n)
        rc = lib.seam_rle_bits_inter(d_pairs.data_ptr(), P, t.H, t.hw.data_ptr(), t.cell.data_ptr(), ws.data_ptr(), 4 * t.cells, t.n,
                                     inter.data_ptr(), stream())
        assert rc == 0, rc
        rc = lib.seam_rle_bits_area(t.H, t.hw.data_ptr(), t.cell.data_ptr(), ws.data_ptr(), 4 * t.cells, t.n, area.data_ptr(), stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(in_raw, 8 * P) and untouched(ar_raw, 8 * t.n), "wrote outside the outputs"
        runs.append((inter.cpu().numpy().view(np.int64).tolist(), area.cpu().numpy().view(np.int64).tolist()))
    assert runs[0] == runs[1] and runs[0][0] == want and runs[0][1] == [int(m.sum()) for m in masks]
    assert want[3] == 33 * 7 and want[5] == 0 and want[6] == want[7] == 53 and want[8] == 100
    # a pair of two shapes, an index out of range: -1, nothing else disturbed
    odd = up(np.asarray([(0, 4), (0, 7), (-1, 0), (2, 2)], np.int32))
    o_raw, o = poisoned(8 * 4)
    assert lib.seam_rle_bits_inter(odd.data_ptr(), 4, t.H, t.hw.data_ptr(), t.cell.data_ptr(), ws.data_ptr(), 4 * t.cells, t.n, o.data_ptr(), stream()) == 0
    torch.cuda.synchronize()
    assert untouched(o_raw, 32) and o.cpu().numpy().view(np.int64).tolist() == [-1, -1, -1, int(masks[2].sum())]

    # refusals: nothing launched, nothing written
    out_raw, out = poisoned(8 * P)
    ws2_raw, ws2 = poisoned(4 * t.cells)
    ct_raw, ct = poisoned(4 * t.cells)
    grp_off, grp_obj = up(np.asarray([0, 2], np.int32)), up(np.asarray([0, 1], np.int32))
    one_hw = np.asarray([[33, 7]], np.int32)
    d_one_hw, d_one_cell = up(one_hw), up(np.zeros(2, np.int64))
    Pp, Hh, Cc, W, O, B, s = d_pairs.data_ptr(), t.hw.data_ptr(), t.cell.data_ptr(), ws.data_ptr(), out.data_ptr(), 4 * t.cells, stream()
    RS, RO = t.run_start.data_ptr(), t.run_off.data_ptr()
    inter, area, runs_, cnt, comb = lib.seam_rle_bits_inter, lib.seam_rle_bits_area, lib.seam_rle_bits_from_runs, lib.seam_rle_count_bits, \
        lib.seam_rle_bits_combine
    G = (grp_off.data_ptr(), grp_obj.data_ptr(), 2)
    D1 = (one_hw.ctypes.data, d_one_hw.data_ptr(), d_one_cell.data_ptr())
    refused = [
        inter(None, P, t.H, Hh, Cc, W, B, t.n, O, s), inter(Pp, P, None, Hh, Cc, W, B, t.n, O, s), inter(Pp, P, t.H, None, Cc, W, B, t.n, O, s),
        inter(Pp, P, t.H, Hh, None, W, B, t.n, O, s), inter(Pp, P, t.H, Hh, Cc, None, B, t.n, O, s), inter(Pp, P, t.H, Hh, Cc, W, B, t.n, None, s),
        inter(Pp, -1, t.H, Hh, Cc, W, B, t.n, O, s), inter(Pp, P, t.H, Hh, Cc, W, B, -1, O, s), inter(Pp, P, t.H, Hh, Cc, W, B - 4, t.n, O, s),
        inter(Pp, P, t.H, Hh, Cc, W, B + 2, t.n, O, s), inter(Pp, P, t.H, Hh, Cc, W, B, 0, O, s),
        area(None, Hh, Cc, W, B, t.n, O, s), area(t.H, None, Cc, W, B, t.n, O, s), area(t.H, Hh, None, W, B, t.n, O, s),
        area(t.H, Hh, Cc, None, B, t.n, O, s), area(t.H, Hh, Cc, W, B, t.n, None, s), area(t.H, Hh, Cc, W, B, -1, O, s),
        area(t.H, Hh, Cc, W, B - 4, t.n, O, s),
        runs_(None, RO, t.n_runs, t.H, Hh, Cc, ws2.data_ptr(), B, t.n, s), runs_(RS, None, t.n_runs, t.H, Hh, Cc, ws2.data_ptr(), B, t.n, s),
        runs_(RS, RO, t.n_runs, None, Hh, Cc, ws2.data_ptr(), B, t.n, s), runs_(RS, RO, t.n_runs, t.H, None, Cc, ws2.data_ptr(), B, t.n, s),
        runs_(RS, RO, t.n_runs, t.H, Hh, None, ws2.data_ptr(), B, t.n, s), runs_(RS, RO, t.n_runs, t.H, Hh, Cc, None, B, t.n, s),
        runs_(RS, RO, -1, t.H, Hh, Cc, ws2.data_ptr(), B, t.n, s), runs_(RS, RO, t.n_runs, t.H, Hh, Cc, ws2.data_ptr(), B, -1, s),
        runs_(RS, RO, t.n_runs, t.H, Hh, Cc, ws2.data_ptr(), B - 4, t.n, s), runs_(RS, RO, t.n_runs, t.H, Hh, Cc, ws2.data_ptr(), B + 1, t.n, s),
        cnt(None, Hh, Cc, W, B, ct.data_ptr(), t.n, s), cnt(t.H, None, Cc, W, B, ct.data_ptr(), t.n, s), cnt(t.H, Hh, None, W, B, ct.data_ptr(), t.n, s),
        cnt(t.H, Hh, Cc, None, B, ct.data_ptr(), t.n, s), cnt(t.H, Hh, Cc, W, B, None, t.n, s), cnt(t.H, Hh, Cc, W, B, ct.data_ptr(), -1, s),
        cnt(t.H, Hh, Cc, W, B - 4, ct.data_ptr(), t.n, s),
        comb(None, G[1], 2, Hh, Cc, W, B, t.n, *D1, ws2.data_ptr(), B, 1, 0, s), comb(G[0], None, 2, Hh, Cc, W, B, t.n, *D1, ws2.data_ptr(), B, 1, 0, s),
        comb(*G, None, Cc, W, B, t.n, *D1, ws2.data_ptr(), B, 1, 0, s), comb(*G, Hh, None, W, B, t.n, *D1, ws2.data_ptr(), B, 1, 0, s),
        comb(*G, Hh, Cc, None, B, t.n, *D1, ws2.data_ptr(), B, 1, 0, s), comb(*G, Hh, Cc, W, B, t.n, None, D1[1], D1[2], ws2.data_ptr(), B, 1, 0, s),
        comb(*G, Hh, Cc, W, B, t.n, D1[0], None, D1[2], ws2.data_ptr(), B, 1, 0, s), comb(*G, Hh, Cc, W, B, t.n, D1[0], D1[1], None, ws2.data_ptr(), B, 1, 0, s),
        comb(*G, Hh, Cc, W, B, t.n, *D1, None, B, 1, 0, s), comb(*G, Hh, Cc, W, B, t.n, *D1, ws2.data_ptr(), B, -1, 0, s),
        comb(*G, Hh, Cc, W, B, -1, *D1, ws2.data_ptr(), B, 1, 0, s), comb(G[0], G[1], -1, Hh, Cc, W, B, t.n, *D1, ws2.data_ptr(), B, 1, 0, s),
        comb(*G, Hh, Cc, W, B, t.n, *D1, ws2.data_ptr(), 4 * 2 * 7 - 4, 1, 0, s), comb(*G, Hh, Cc, W, B + 2, t.n, *D1, ws2.data_ptr(), B, 1, 0, s),
    ]
    for bad in ([[0, 7]], [[33, 0]], [[16385, 1]], [[1, 16385]], [[16384 * 8, 16384]]):
        b = np.asarray(bad * t.n, np.int32)
        refused += [inter(Pp, P, b.ctypes.data, Hh, Cc, W, B, t.n, O, s), area(b.ctypes.data, Hh, Cc, W, B, t.n, O, s),
                    runs_(RS, RO, t.n_runs, b.ctypes.data, Hh, Cc, ws2.data_ptr(), B, t.n, s), cnt(b.ctypes.data, Hh, Cc, W, B, ct.data_ptr(), t.n, s),
                    comb(*G, Hh, Cc, W, B, t.n, b.ctypes.data, D1[1], D1[2], ws2.data_ptr(), B, 1, 0, s)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    # n == 0 / P == 0 are no-ops that return 0, whatever else is passed
    assert inter(None, 0, None, None, None, None, 0, 0, None, s) == 0 and area(None, None, None, None, 0, 0, None, s) == 0
    assert runs_(None, None, 0, None, None, None, None, 0, 0, s) == 0 and cnt(None, None, None, None, 0, None, 0, s) == 0
    assert comb(None, None, 0, None, None, None, 0, 0, None, None, None, None, 0, 0, 0, s) == 0
    torch.cuda.synchronize()
    for raw in (out_raw, ws2_raw, ct_raw):
        assert bool((raw == 0xA5).all()), "a refused or empty call wrote something"


def test_combine_through_the_abi_groups_of_one_two_and_nine(lib):
    rng = np.random.default_rng(19)
    hws = [(33, 7)] * 9 + [(65, 2)] * 2 + [(31, 1)]
    counts = [MR.random_counts(rng, h, w, max_runs=6, zero_runs=True) for h, w in hws]
    masks = [MR.rle_decode(c, h, w) for c, (h, w) in zip(counts, hws)]
    src = Tables(counts, hws)
    _, ws = src.bits(lib)
    groups, dst_hws = [list(range(9)), [9, 10], [11], [10, 9, 10], [3]], [(33, 7), (65, 2), (31, 1), (65, 2), (33, 7)]
    dst = Tables([[h * w] for h, w in dst_hws], dst_hws)
    g_off = up(np.cumsum([0] + [len(g) for g in groups]).astype(np.int32))
    g_obj = up(np.asarray([i for g in groups for i in g], np.int32))
    for intersect in (0, 1):
        out_raw, out = poisoned(4 * dst.cells)
        rc = lib.seam_rle_bits_combine(g_off.data_ptr(), g_obj.data_ptr(), int(g_obj.numel()), src.hw.data_ptr(), src.cell.data_ptr(),
                                       ws.data_ptr(), 4 * src.cells, src.n, dst.H, dst.hw.data_ptr(), dst.cell.data_ptr(), out.data_ptr(),
                                       4 * dst.cells, dst.n, intersect, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(out_raw, 4 * dst.cells)
        words = out.cpu().numpy().view(np.uint32)
        for k, g in enumerate(groups):
            m = masks[g[0]]
            for i in g[1:]:
                m = (m & masks[i]) if intersect else (m | masks[i])
            assert np.array_equal(words[dst.cell_off[k]:dst.cell_off[k + 1]], pack_bits(m)), (intersect, k)


# ------------------------------------------------------------------------------------------------ evaluate_results
def quad(rng, h, w):
    """a seeded four-corner polygon inside the image, and its xyxy box"""
    x0, y0 = float(rng.integers(0, w // 2)), float(rng.integers(0, h // 2))
    x1, y1 = x0 + float(rng.integers(12, w // 2)), y0 + float(rng.integers(12, h // 2))
    j = rng.uniform(0.0, 5.0, size=4)
    return [x0 + j[0], y0, x1, y0 + j[1], x1 - j[2], y1, x0, y1 - j[3]], [x0, y0, x1, y1]


def test_evaluate_results_equals_update_on_the_same_outputs(tmp_path):
    from seam_match_rcnn_amd import evaluator_det as E
    from seam_match_rcnn_amd import mask_utils as M
    rng = np.random.default_rng(2024)
    sizes = [(96, 128), (64, 80), (96, 128), (64, 80), (96, 128), (64, 80)]
    n_gt, n_dt = [4, 3, 2, 0, 4, 1], [12, 7, 0, 5, 9, 3]                  # image 2 has no detections, image 3 no ground truth
    outputs, targets, images, annotations = [], [], [], []
    yy, xx = np.mgrid[0:28, 0:28]
    for i, ((h, w), ng, nd) in enumerate(zip(sizes, n_gt, n_dt)):
        quads = [quad(rng, h, w) for _ in range(ng)]
        polys, gboxes = [[q[0]] for q in quads], np.asarray([q[1] for q in quads], np.float32).reshape(-1, 4)
        masks = M.masks_from_annotations([polys], [(h, w)], DEV)[0]
        glabels = rng.integers(1, 4, size=ng)
        crowd = np.zeros(ng, np.int64)
        if i == 0:
            crowd[2] = 1                                                 # the one crowd ground truth
        area = masks.sum((1, 2)).to(torch.float32).cpu()
        targets.append(dict(boxes=torch.from_numpy(gboxes), labels=torch.from_numpy(glabels), masks=masks, area=area,
                            iscrowd=torch.from_numpy(crowd)))
        src = gboxes[rng.integers(0, ng, size=nd)] if ng else np.tile(np.asarray([[10.0, 10.0, 50.0, 50.0]], np.float32), (nd, 1))
        dboxes = (src + rng.uniform(-6.0, 6.0, size=(nd, 4))).astype(np.float32).reshape(-1, 4)
        r = rng.uniform(8.0, 16.0, size=nd)
        probs = np.stack([np.clip(1.2 - np.hypot(yy - 13.5, xx - 13.5) / rr, 0.0, 1.0) for rr in r]) if nd else np.zeros((0, 28, 28))
        probs = (probs * rng.uniform(0.6, 1.0, size=probs.shape)).astype(np.float32)
        dlabels = np.where(rng.random(nd) < 0.7, glabels[rng.integers(0, ng, size=nd)] if ng else 1, rng.integers(1, 4, size=nd))
        outputs.append(dict(boxes=torch.from_numpy(dboxes).to(DEV), labels=torch.from_numpy(dlabels.astype(np.int64)).to(DEV),
                            scores=torch.from_numpy(rng.uniform(0.05, 1.0, size=nd).astype(np.float32)).to(DEV),
                            mask_probs=torch.from_numpy(probs)[:, None].to(DEV)))
        images.append({"id": 100 + i, "height": h, "width": w})
        x, y, bw, bh = E._xywh(gboxes)                                   # the fp32 values `update` derives, widened
        for k in range(ng):
            segm = polys[k]
            if k == 1:                                                   # the three annotation forms
                segm = {"size": [h, w], "counts": R.rle_encode(masks[k].cpu().numpy())}
            elif k == 3:
                segm = {"size": [h, w], "counts": M.encode(masks[k])["counts"].decode("ascii")}
            annotations.append({"id": len(annotations) + 1, "image_id": 100 + i, "category_id": int(glabels[k]), "iscrowd": int(crowd[k]),
                                "bbox": [float(x[k]), float(y[k]), float(bw[k]), float(bh[k])], "area": float(area[k]), "segmentation": segm})
    want = E.DetectionEvaluator()
    want.update(outputs, targets)
    want_stats = want.summarize(verbose=False)
    results = E.coco_results(outputs, [im["id"] for im in images], sizes)
    gt_text, res_text = json.dumps({"images": images, "annotations": annotations}), json.dumps(results)
    stats, ev = E.evaluate_results(json.loads(gt_text), json.loads(res_text), verbose=False, return_report=True)
    assert len(results) == sum(n_dt) and sorted(stats) == ["bbox", "segm"] and len(stats["bbox"]) == len(stats["segm"]) == 12
    assert stats == want_stats, (stats, want_stats)
    assert any(v not in (-1.0, 0.0, 1.0) for v in stats["segm"]) and any(v not in (-1.0, 0.0, 1.0) for v in stats["bbox"])
    for t in ("bbox", "segm"):
        assert np.array_equal(ev.precision[t], want.precision[t]) and np.array_equal(ev.recall[t], want.recall[t])
    assert ev.categories == want.categories and len(ev.images) == 6
    # from paths, and in several chunks
    (tmp_path / "gt.json").write_text(gt_text)
    (tmp_path / "dt.json").write_text(res_text)
    from seam_match_rcnn_amd import ops, ops_masks
    old = ops_masks.RLE_BITS_BUDGET_BYTES
    ops_masks.RLE_BITS_BUDGET_BYTES = 40000
    try:
        assert len(ops.budget_chunks([4 * cells_of(h, w) * (a + b) + h * w * a for (h, w), a, b in zip(sizes, n_gt, n_dt)])) > 2
        assert E.evaluate_results(str(tmp_path / "gt.json"), str(tmp_path / "dt.json"), verbose=False) == want_stats
    finally:
        ops_masks.RLE_BITS_BUDGET_BYTES = old
    assert E.evaluate_results(json.loads(gt_text), json.loads(res_text), iou_types=("bbox",), verbose=False) == {"bbox": want_stats["bbox"]}
    with pytest.raises(ValueError):
        E.evaluate_results(json.loads(gt_text), json.loads(res_text) + [dict(results[0], image_id=7)], verbose=False)
