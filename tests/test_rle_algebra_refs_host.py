"""CPU: the restatement of rleMerge / rleFrBbox (tests/rle_algebra_refs.py) pinned against itself.  The device route combines
bitmaps and encodes the result, so it relies on one property: for canonical run lists the folded run merge IS ``rle_encode`` of the
OR / AND of the decoded masks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rle_algebra_refs as A                                            # noqa: E402

SHAPES = [(1, 1), (1, 7), (31, 2), (32, 1), (33, 7), (65, 2), (5, 9)]


def combined(rles, h, w, intersect):
    m = A.rle_decode(rles[0], h, w)
    for c in rles[1:]:
        d = A.rle_decode(c, h, w)
        m = (m & d) if intersect else (m | d)
    return m


@pytest.mark.parametrize("intersect", [False, True], ids=["union", "intersection"])
def test_folded_merge_of_canonical_lists_is_the_encoding_of_the_combined_mask(intersect):
    rng = np.random.default_rng(17)
    checked = 0
    for h, w in SHAPES:
        fixed = [[h * w], [0, h * w]] + ([[1, h * w - 1]] if h * w > 1 else [])
        for n in (1, 2, 3, 9):
            for trial in range(12):
                rles = [A.random_counts(rng, h, w, max_runs=1 + trial, zero_runs=False) for _ in range(n)]
                if trial < len(fixed):
                    rles[trial % n] = fixed[trial]
                for c in rles:                                           # canonical: only the first count may be 0
                    assert all(v > 0 for v in c[1:]) and sum(c) == h * w
                got, gh, gw = A.rle_merge([(c, h, w) for c in rles], intersect)
                assert (gh, gw) == (h, w)
                assert got == A.rle_encode(combined(rles, h, w, intersect)), (h, w, rles)
                checked += 1
    assert checked == len(SHAPES) * 4 * 12


@pytest.mark.parametrize("intersect", [False, True], ids=["union", "intersection"])
def test_folded_merge_of_lists_with_zero_runs_decodes_to_the_combined_mask(intersect):
    """Only the masks are compared: rleMerge may keep an interior zero-length run.  One more difference shows here: the pair
    walk ends when both lists have nothing left in hand (``ct == 0``), which also happens when both stand on a zero-length run
    at once with runs still to come.  The merged list then stops short of h*w; what it holds up to there is still the combined
    mask.  The device route (bitmaps) has no such case and always returns the whole mask."""
    rng = np.random.default_rng(23)
    whole = short = 0
    for h, w in SHAPES:
        for n in (2, 3, 9):
            for _ in range(12):
                rles = [A.random_counts(rng, h, w, max_runs=8, zero_runs=True) for _ in range(n)]
                cur, cur_mask, stopped = rles[0], A.rle_decode(rles[0], h, w), False
                for c in rles[1:]:                                       # the fold, every pair step checked
                    step = A.rle_merge_pair(cur, c, intersect)
                    want = (cur_mask & A.rle_decode(c, h, w)) if intersect else (cur_mask | A.rle_decode(c, h, w))
                    s = sum(step)
                    assert s <= h * w
                    flat, pos = np.zeros(s, np.uint8), 0                 # column-major, as far as the list goes
                    for j, v in enumerate(step):
                        flat[pos:pos + v] = j & 1
                        pos += v
                    assert np.array_equal(flat, want.T.reshape(-1)[:s]), (h, w, cur, c)
                    whole += s == h * w
                    short += s < h * w
                    stopped |= s < h * w
                    cur, cur_mask = (step if s == h * w else A.rle_encode(want)), want
                assert np.array_equal(cur_mask, combined(rles, h, w, intersect))
                if not stopped:
                    assert A.rle_merge([(c, h, w) for c in rles], intersect) == (cur, h, w)
    assert whole > 0 and short > 0, (whole, short)


def test_merge_of_nothing_one_and_mismatched_sizes():
    assert A.rle_merge([]) == ([], 0, 0)
    assert A.rle_merge([([3, 2, 1], 2, 3)]) == ([3, 2, 1], 2, 3)
    assert A.rle_merge([([6], 2, 3), ([6], 3, 2)]) == ([], 0, 0)


def test_box_as_polygon_is_the_mask_of_its_four_corners():
    h, w = 33, 21
    boxes = [[2.0, 3.0, 10.0, 20.0], [0.5, 0.25, 7.75, 9.5], [-4.0, -2.0, 10.0, 12.0], [15.0, 28.0, 30.0, 30.0],
             [40.0, 50.0, 5.0, 5.0], [3.0, 4.0, 0.0, 0.0], [0.0, 0.0, 21.0, 33.0]]
    for x, y, bw, bh in boxes:
        corners = [x, y, x, y + bh, x + bw, y + bh, x + bw, y]
        assert A.bbox_polygon([x, y, bw, bh]) == corners
        want = A.poly_mask([corners], h, w)
        assert A.rle_fr_bbox([x, y, bw, bh], h, w) == A.rle_encode(want)
        assert np.array_equal(A.rle_decode(A.rle_fr_bbox([x, y, bw, bh], h, w), h, w), want)
    assert A.poly_mask([A.bbox_polygon(boxes[0])], h, w).sum() == 10 * 20
    assert A.poly_mask([A.bbox_polygon(boxes[4])], h, w).sum() == 0 and A.poly_mask([A.bbox_polygon(boxes[6])], h, w).all()


def test_dispatch_forms():
    h, w = 12, 10
    box, poly = [1.0, 2.0, 5.0, 6.0], [1.0, 1.0, 8.0, 2.0, 5.0, 9.0]
    unc = {"size": [h, w], "counts": [3, 7, 110]}
    assert A.fr_py_objects(np.asarray([box, box]), h, w) == [A.rle_fr_bbox(box, h, w)] * 2 == A.fr_py_objects([box, box], h, w)
    assert A.fr_py_objects([poly, poly + [2.0, 7.0]], h, w) == [A.rle_fr_poly(poly, h, w), A.rle_fr_poly(poly + [2.0, 7.0], h, w)]
    assert A.fr_py_objects([unc], h, w) == [[3, 7, 110]] and A.fr_py_objects(unc, h, w) == [3, 7, 110]
    assert A.fr_py_objects(box, h, w) == A.rle_fr_bbox(box, h, w) and A.fr_py_objects(poly, h, w) == A.rle_fr_poly(poly, h, w)
    with pytest.raises(Exception):
        A.fr_py_objects("nothing", h, w)
