"""CPU: the host restatement of rleEncode / rleArea / rleToBbox (tests/rle_refs.py) against three independent witnesses --
``mask_refs.rle_decode`` (decode(encode(m)) == m), the tight box of ``np.nonzero`` and ``m.sum()`` -- then the product's host
parts against it: the vectorised compressed-string writer against ``mask_utils.rle_to_string`` character for character and
through ``rle_from_string``, ``area`` / ``toBbox`` on counts, and ``coco_results`` on CPU tensors through ``json.dumps``."""
import json

import numpy as np
import pytest
import torch

import mask_refs as MR
import rle_refs as R

SHAPES = [(1, 1), (1, 65), (65, 1), (31, 33), (32, 32), (33, 31), (5, 6)]


def masks_of(h, w, rng):
    """name -> uint8 [h,w]: the contents the device tests use, at one shape."""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"zeros": np.zeros((h, w), np.uint8), "ones": np.ones((h, w), np.uint8),
           "checker": ((yy + xx) % 2).astype(np.uint8), "alt_columns": (xx % 2).astype(np.uint8).copy()}
    for name, (y, x) in {"tl": (0, 0), "tr": (0, w - 1), "bl": (h - 1, 0), "br": (h - 1, w - 1)}.items():
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        out["corner_" + name] = m
    carry = np.zeros((h, w), np.uint8)                                   # bottom row + top row of the next column
    carry[h - 1, 0:w:2] = 1
    carry[0, 1:w:2] = 1
    out["carry"] = carry
    for p in (0.02, 0.5, 0.98):
        out[f"random_{p}"] = (rng.random((h, w)) < p).astype(np.uint8)
    out["bytes"] = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(h, w))
    return out


@pytest.fixture(scope="module")
def cases():
    rng = np.random.default_rng(11)
    return [(f"{h}x{w} {name}", m) for h, w in SHAPES for name, m in masks_of(h, w, rng).items()]


def test_restatement_against_independent_witnesses(cases):
    for what, m in cases:
        h, w = m.shape
        c = R.rle_encode(m)
        assert sum(c) == h * w and all(v > 0 for v in c[1:]) and c[0] >= 0, what
        assert np.array_equal(MR.rle_decode(c, h, w), (m != 0).astype(np.uint8)), what
        assert R.rle_area(c) == int((m != 0).sum()), what
        want = R.tight_box(m)
        if R.spans_columns(m):                                         # maskApi's rule: such a run makes the box full height
            want = [want[0], 0.0, want[2], float(h)]
        assert R.rle_to_bbox(c, h, w) == want, what
    assert R.rle_encode(np.zeros((3, 4), np.uint8)) == [12] and R.rle_encode(np.ones((3, 4), np.uint8)) == [0, 12]
    assert R.rle_encode(np.array([[0, 1], [1, 0]], np.uint8)) == [1, 2, 1]
    assert R.rle_to_bbox([1, 2, 1], 2, 2) == [0.0, 0.0, 2.0, 2.0] and R.rle_to_bbox([4], 2, 2) == [0.0, 0.0, 0.0, 0.0]


def test_vectorised_string_writer(cases):
    from seam_match_rcnn_amd import mask_utils as M
    hw = 33 * 65
    by_length = [[0, 31 - 16], [0, 15, 16], [3, 2 ** 9 - 1, 2 ** 9], [3, 2 ** 14, 2 ** 19 - 1], [3, 2 ** 19, 2 ** 24 - 1],
                 [3, 2 ** 24, 2 ** 29 - 1], [3, 2 ** 29, 2 ** 31 - 1]]           # 1 to 7 characters per count
    negative = [[5, 4, 3, 1, 1, 1, 40, 2, 1, 900, 1, 1], [2 ** 20, 7, 2 ** 20, 1, 5, 2 ** 20, 2 ** 30, 3, 1, 2 ** 30],
                [3, 2 ** 40, 7, 2 ** 33 + 1, 2 ** 40 + 5, 0, 2 ** 62]]           # past 32 bits: the writer's int64 path
    objs = [[0], [0, hw], [hw]] + by_length + negative + [R.rle_encode(m) for _, m in cases]
    lengths = set()
    for c in by_length:
        for v in c[:3]:
            lengths.add(len(M.rle_to_string([v])))
    assert lengths == {1, 2, 3, 4, 5, 6, 7}
    assert any(c[i] - c[i - 2] < 0 for c in negative for i in range(3, len(c)))
    got = M.counts_to_bytes(objs)
    assert len(got) == len(objs)
    for c, g in zip(objs, got):
        assert isinstance(g, bytes) and g.decode("ascii") == M.rle_to_string(c) == MR.rle_to_string(c), c[:8]
        assert M.rle_from_string(g) == [int(v) for v in c]
    assert got[:3] == [M.rle_to_string([0]).encode(), M.rle_to_string([0, hw]).encode(), M.rle_to_string([hw]).encode()]
    assert M.counts_to_bytes([]) == [] and M.counts_to_bytes([np.zeros(0, np.int64), [7]]) == [b"", b"7"]
    one_by_one = [M.counts_to_bytes([c])[0] for c in objs]              # a batch and single calls agree
    assert one_by_one == got


def test_area_and_bbox_from_counts(cases):
    from seam_match_rcnn_amd import mask_utils as M
    rles = []
    for _, m in cases:
        c = R.rle_encode(m)
        rles.append({"size": list(m.shape), "counts": c if len(rles) % 2 else M.rle_to_string(c)})
    areas, boxes = M.area(rles), M.toBbox(rles)
    assert areas.dtype == np.uint32 and boxes.dtype == np.float64 and boxes.shape == (len(rles), 4)
    for (what, m), r, a, b in zip(cases, rles, areas, boxes):
        c = R.rle_encode(m)
        assert int(a) == R.rle_area(c) and list(b) == R.rle_to_bbox(c, *m.shape), what
    assert int(M.area(rles[3])) == int(areas[3]) and list(M.toBbox(rles[3])) == list(boxes[3])
    same = {"size": [3, 4], "counts": "anything"}
    assert M.annToRLE({"segmentation": same}, [3, 4]) is same
    unc = M.annToRLE({"segmentation": {"size": [3, 4], "counts": [2, 3, 7]}}, [3, 4])
    assert unc == {"size": [3, 4], "counts": M.rle_to_string([2, 3, 7]).encode()}


def test_box_iou_shared_with_the_evaluator():
    from seam_match_rcnn_amd import evaluator_det as E
    from seam_match_rcnn_amd import mask_utils as M
    rng = np.random.default_rng(2)
    d = np.concatenate([rng.uniform(0, 50, (6, 2)), rng.uniform(1, 40, (6, 2))], 1)
    g = np.concatenate([rng.uniform(0, 50, (4, 2)), rng.uniform(1, 40, (4, 2))], 1)
    crowd = [0, 1, 0, 1]
    got = M.iou(d, g.tolist(), crowd)
    want = np.zeros((6, 4))
    for i in range(6):
        for j in range(4):
            iw = min(d[i, 0] + d[i, 2], g[j, 0] + g[j, 2]) - max(d[i, 0], g[j, 0])
            ih = min(d[i, 1] + d[i, 3], g[j, 1] + g[j, 3]) - max(d[i, 1], g[j, 1])
            if iw > 0 and ih > 0:
                da, ga = d[i, 2] * d[i, 3], g[j, 2] * g[j, 3]
                want[i, j] = iw * ih / (da if crowd[j] else da + ga - iw * ih)
    assert got.shape == (6, 4) and np.array_equal(got, want) and (got > 0).sum() > 4
    xyxy = np.concatenate([d[:, :2], d[:, :2] + d[:, 2:]], 1).astype(np.float32)          # the evaluator's own entry still agrees
    gxyxy = np.concatenate([g[:, :2], g[:, :2] + g[:, 2:]], 1).astype(np.float32)
    again = E._box_iou_xywh(*E._xywh(xyxy), *E._xywh(gxyxy), np.asarray(crowd) != 0)
    assert np.array_equal(E._box_iou(xyxy, gxyxy, np.asarray(crowd) != 0), again)
    assert M.iou(np.zeros((0, 4)), g, crowd).shape == (0, 4)


def test_coco_results_bbox_on_cpu_tensors_is_json():
    from seam_match_rcnn_amd import evaluator_det as E
    g = torch.Generator().manual_seed(5)
    outputs = []
    for k in (3, 0, 2):
        xy = torch.rand((k, 2), generator=g) * 50
        boxes = torch.cat([xy, xy + torch.rand((k, 2), generator=g) * 30 + 0.1], 1)
        outputs.append(dict(boxes=boxes, labels=torch.randint(1, 4, (k,), generator=g), scores=torch.rand((k,), generator=g)))
    res = E.coco_results(outputs, [17, torch.tensor(18), "img19"], [(60, 80)] * 3, label_to_category={1: 11, 2: 22, 3: 33},
                         iou_types=("bbox",))
    back = json.loads(json.dumps(res))
    assert back == res and len(res) == 5
    assert [r["image_id"] for r in res] == [17, 17, 17, "img19", "img19"]
    flat = [(o, k) for o in outputs for k in range(len(o["labels"]))]
    for r, (o, k) in zip(res, flat):
        assert set(r) == {"image_id", "category_id", "score", "bbox"}
        assert type(r["category_id"]) is int and type(r["score"]) is float and all(type(v) is float for v in r["bbox"])
        x, y, w, h = (v[k] for v in E._xywh(o["boxes"].numpy()))
        assert r["bbox"] == [x, y, w, h] and r["category_id"] == 11 * int(o["labels"][k]) and r["score"] == float(o["scores"][k])
        assert r["bbox"][2] == float(o["boxes"][k, 2] - o["boxes"][k, 0])            # subtracted in fp32
    plain = E.coco_results(outputs[:1], [0], [(60, 80)], iou_types=("bbox",))
    assert [r["category_id"] for r in plain] == outputs[0]["labels"].tolist()
    with pytest.raises(ValueError):
        E.coco_results(outputs, [1, 2], [(60, 80)] * 3, iou_types=("bbox",))
    with pytest.raises(ValueError):
        E.coco_results(outputs, [1, 2, 3], [(60, 80)] * 3, iou_types=("keypoints",))
