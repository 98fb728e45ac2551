"""CPU: the host restatement of the COCO mask procedure (tests/mask_refs.py) gives the hand answers, its per-column fill equals
the sorted linear form (no image column carries an odd number of crossings -- what csrc/seam_masks.hip's scan relies on), the RLE
string codec round-trips, and the host side of the product (ops packing, mask_utils validation) is right.  No GPU needed: every
ValueError is raised before the device is touched."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_refs as R                                                   # noqa: E402


def box(x, y, bw, bh):
    return [x, y, x, y + bh, x + bw, y + bh, x + bw, y]


# ------------------------------------------------------------------------------------------------ the reference itself
@pytest.mark.parametrize("x,y,bw,bh", [(0, 0, 2, 3), (2, 1, 3, 2), (3, 3, 1, 1), (4, 3, 2, 2), (0, 0, 6, 5)])
def test_integer_box_fills_exactly_its_pixels(x, y, bw, bh):
    want = np.zeros((5, 6), np.uint8)
    want[y:y + bh, x:x + bw] = 1
    assert np.array_equal(R.poly_mask([box(x, y, bw, bh)], 5, 6), want)


def test_hand_answers():
    m = R.poly_mask([[1, 1, 4, 1, 4, 3, 1, 3]], 5, 6)
    want = np.zeros((5, 6), np.uint8)
    want[1:3, 1:4] = 1
    assert np.array_equal(m, want)
    m = R.poly_mask([[0.5, 0.5, 4.5, 0.5, 2.5, 4.5]], 5, 6)
    assert m.tolist() == [[0] * 6, [0, 1, 1, 1, 0, 0], [0, 0, 1, 1, 0, 0], [0, 0, 1, 0, 0, 0], [0] * 6]
    assert int(R.poly_mask([[-1, -1, -1, 9, 9, 9, 9, -1]], 5, 6).sum()) == 30          # encloses the whole image
    assert int(R.poly_mask([[2, 2]], 5, 6).sum()) == 0 and int(R.poly_mask([[1, 1, 4, 3]], 5, 6).sum()) == 0
    assert int(R.poly_mask([], 5, 6).sum()) == 0
    two = R.poly_mask([box(0, 0, 2, 2), box(1, 1, 3, 2)], 5, 6)                          # parts are OR-ed, not XOR-ed
    assert int(two.sum()) == 4 + 6 - 1 and two[1, 1] == 1
    assert R.c_int(-0.75) == 0 and R.upsample([-0.25, -0.3])[0][0] == 0 and R.upsample([-0.25, -0.3])[1][0] == -1


def test_column_fill_equals_linear_fill_and_no_column_is_odd():
    rng = np.random.default_rng(20250)
    for i in range(3000):
        h, w = int(rng.choice([1, 2, 3, 7, 16, 33])), int(rng.choice([1, 2, 5, 8, 31]))
        xy = R.random_polygon(rng, h, w, small_steps=(i % 4 == 3))
        assert not (R.column_counts(xy, h, w) & 1).any(), (h, w, xy)
        assert np.array_equal(R.part_mask(xy, h, w), R.part_mask_by_columns(xy, h, w)), (h, w, xy)


def test_rle_decode_hand_cases():
    assert R.rle_decode([2, 3, 1, 1], 7, 1)[:, 0].tolist() == [0, 0, 1, 1, 1, 0, 1]
    assert R.rle_decode([0, 6, 1], 7, 1)[:, 0].tolist() == [1, 1, 1, 1, 1, 1, 0]
    m = R.rle_decode([3, 2, 1], 2, 3)                                                   # column-major: (r, c) = a % h, a // h
    assert m.tolist() == [[0, 0, 1], [0, 1, 0]]
    assert int(R.rle_decode([6], 2, 3).sum()) == 0 and int(R.rle_decode([0, 6], 2, 3).sum()) == 6
    assert R.rle_decode([1, 0, 2, 3], 2, 3).tolist() == [[0, 0, 1], [0, 1, 1]]            # a zero-length run of ones


# ------------------------------------------------------------------------------------------------ the string codec
CODEC_CASES = [[0, 5, 3, 22], [30], [3, 4, 2, 1, 20], [5, 1, 5, 1, 5, 1, 5, 1, 6], [100000, 5, 70000, 3], [16, 31, 32, 1023, 1024],
               [7, 900, 3, 2, 500, 1, 9]]


@pytest.mark.parametrize("counts", CODEC_CASES)
def test_string_codec_round_trips(counts):
    from seam_match_rcnn_amd import mask_utils as M
    s = M.rle_to_string(counts)
    assert s == R.rle_to_string(counts)
    assert M.rle_from_string(s) == counts == R.rle_from_string(s) == M.rle_from_string(s.encode())


def test_string_codec_hand_cases():
    from seam_match_rcnn_amd import mask_utils as M
    assert M.rle_from_string("U1") == [37] == R.rle_from_string("U1")                  # 37 = 5 | 1 << 5: 'U' = 48 + (5 | 0x20), '1'
    assert M.rle_from_string("`0") == [16] and M.rle_to_string([16]) == "`0"            # 16 needs a second character (0x10 is the sign)
    assert M.rle_to_string([0, 5]) == "05" and M.rle_from_string("05") == [0, 5]        # a zero first run
    s = M.rle_to_string([3, 4, 2, 1])                                                  # fourth count: 1 - 4 = -3 -> one character, sign bit
    assert s[3] == chr(48 + (-3 & 0x1F)) and M.rle_from_string(s) == [3, 4, 2, 1]
    rng = np.random.default_rng(3)
    for _ in range(200):
        counts = R.random_counts(rng, int(rng.integers(1, 400)), int(rng.integers(1, 400)), max_runs=40)
        assert M.rle_from_string(M.rle_to_string(counts)) == counts
    for bad in ("U", "0\x7f", 5):
        with pytest.raises(ValueError):
            M.rle_from_string(bad)


# ------------------------------------------------------------------------------------------------ ops: host packing
def test_poly_packing_hand_case():
    from seam_match_rcnn_amd import ops
    polys = [[[[1, 1, 4, 1, 4, 3, 1, 3], [0, 0, 2, 0]], None, []], [[[0.5, 0.5]]]]
    lay, t = ops.pack_poly_masks(polys, [(5, 6), (33, 8)])
    assert t["pts"].tolist() == [[5, 5], [20, 5], [20, 15], [5, 15], [0, 0], [10, 0], [3, 3]] and t["pts"].dtype == np.int32
    assert t["part_off"].tolist() == [0, 4, 6, 7] and t["part_obj"].tolist() == [0, 0, 2]
    assert t["edge_pt_off"].tolist() == [0, 16, 27, 43, 54, 65, 76, 77]                 # max(dx, dy) + 1 per ring edge
    assert t["part_ws_off"].tolist() == [0, 6, 12, 28] and t["part_ws_off"].dtype == np.int64   # w * ceil((h+1)/32) words
    assert (t["P"], t["V"], t["T"], t["n"]) == (3, 7, 77, 3)
    assert t["obj_hw"].tolist() == [[5, 6], [5, 6], [33, 8]] and t["obj_out_off"].tolist() == [0, 60, 90]   # the None object keeps its slot
    assert lay.img_off == [0, 90, 90 + 264] and lay.total == 354 and lay.counts == [3, 1]
    _, t = ops.pack_poly_masks([[[[-0.25, -0.3, -0.1, 7.5]]]], [(4, 4)])                # C truncation toward zero
    assert t["pts"].tolist() == [[0, -1], [0, 38]]
    lay, t = ops.pack_poly_masks([[], []], [(4, 4), (2, 2)])
    assert (t["P"], t["V"], t["T"], t["n"], lay.total) == (0, 0, 0, 0, 0)


def test_rle_packing_hand_case():
    from seam_match_rcnn_amd import ops
    lay, t = ops.pack_rle_masks([[[3, 2, 1], None], [[0, 4], [1, 0, 2, 1]]], [(2, 3), (2, 2)])
    assert t["run_start"].tolist() == [0, 3, 5, 0, 0, 0, 1, 1, 3] and t["obj_run_off"].tolist() == [0, 3, 5, 9]
    assert t["obj_hw"].tolist() == [[2, 3], [2, 2], [2, 2]] and t["obj_out_off"].tolist() == [0, 12, 16] and t["n"] == 3
    assert lay.total == 20


def test_workspace_bytes_of_the_abi():
    from seam_match_rcnn_amd import _native
    f = _native.lib().seam_poly_masks_ws_bytes
    assert f(5, 6) == 24 and f(31, 7) == 28 and f(32, 7) == 56 and f(63, 1) == 8 and f(64, 1) == 12 and f(800, 1216) == 26 * 1216 * 4
    assert f(0, 5) == 0 and f(5, 0) == 0 and f(16385, 5) == 0 and f(16384, 16384) == 513 * 16384 * 4


# ------------------------------------------------------------------------------------------------ every refusal
def test_value_errors_name_the_object():
    from seam_match_rcnn_amd import mask_utils as M
    from seam_match_rcnn_amd import ops
    ok = [[1, 1, 4, 1, 4, 3]]
    bad = [
        ([[ok, [[1, 1, 4]]]], "image 0 object 1"),                                        # odd-length part
        ([[ok], [[[]]]], "image 1 object 0"),                                             # empty part
        ([[[[1, float("nan"), 2, 2]]]], "image 0 object 0"),
        ([[[[1, float("inf"), 2, 2]]]], "image 0 object 0"),
        ([[[[1, 2.0 ** 31 / 5, 2, 2]]]], "image 0 object 0"),                             # |5x + 0.5| >= 2^31
        ([[ok, ok, {"counts": [3, 2], "size": [5, 6]}]], "image 0 object 2"),             # counts do not sum to h*w
        ([[{"counts": [30], "size": [6, 5]}]], "image 0 object 0"),                       # the dict's size disagrees
        ([[{"counts": M.rle_to_string([10, 19]), "size": [5, 6]}]], "image 0 object 0"),
        ([[{"counts": [-1, 31], "size": [5, 6]}]], "image 0 object 0"),
        ([[{"counts": [1.5, 28.5], "size": [5, 6]}]], "image 0 object 0"),
        ([[{"size": [5, 6]}]], "image 0 object 0"),
        ([[7]], "image 0 object 0"),
        ([[[1, 1, 4, 1, 4, 3]]], "image 0 object 0"),                                     # a flat polygon, not a list of parts
    ]
    for annos, who in bad:
        sizes = [(5, 6)] * len(annos)
        with pytest.raises(ValueError, match=who):
            M.masks_from_annotations(annos, sizes, "cuda")
    with pytest.raises(ValueError, match="image 0 object 0"):
        M.annToMask({"segmentation": [[1, 2, 3]]}, [5, 6])
    with pytest.raises(ValueError, match="image 0 object 1"):
        ops.pack_poly_masks([[[ok[0]], [[1, 2, 3]]]], [(5, 6)])
    with pytest.raises(ValueError, match="image 1 object 0"):
        ops.pack_rle_masks([[], [[29]]], [(5, 6), (5, 6)])
    for sizes in ([(0, 6)], [(5, 16385)], [(5,)], [(5.5, 6)], []):
        with pytest.raises(ValueError):
            ops.pack_poly_masks([[]], sizes)
    with pytest.raises(ValueError, match="no 'size'"):
        M.targets_to_device([{"segmentation": [ok]}], "cuda")
    with pytest.raises(ValueError, match="boundary points"):                               # 2^31 points or more in one call
        ops.pack_poly_masks([[[[0, 0, 4e8, 0]]] * 2], [(5, 6)])
    with pytest.raises(ValueError):
        ops.poly_masks([[None]], [(5, 6)], "cuda")


def test_no_cpu_path():
    from seam_match_rcnn_amd import _native
    from seam_match_rcnn_amd import mask_utils as M
    with pytest.raises(_native.SeamNativeError):
        M.masks_from_annotations([[[[1, 1, 4, 1, 4, 3]]]], [(5, 6)], "cpu")


def test_public_signatures():
    from seam_match_rcnn_amd import mask_utils as M
    from seam_match_rcnn_amd import ops
    assert list(inspect.signature(M.annToMask).parameters) == ["ann", "size"]
    assert list(inspect.signature(M.masks_from_annotations).parameters) == ["annos_per_image", "sizes", "device"]
    assert list(inspect.signature(M.targets_to_device).parameters) == ["targets", "device"]
    assert list(inspect.signature(M.rle_from_string).parameters) == ["s"] and list(inspect.signature(M.rle_to_string).parameters) == ["counts"]
    assert callable(ops.poly_masks) and callable(ops.rle_masks)
    t = M.targets_to_device([{"boxes": torch.zeros(0, 4), "image_id": 3}], "cpu")        # nothing to rasterise: tensors move, the rest passes
    assert set(t[0]) == {"boxes", "image_id"} and t[0]["image_id"] == 3
