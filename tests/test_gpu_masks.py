"""GPU: csrc/seam_masks.hip against the host restatement of the COCO mask procedure (tests/mask_refs.py), bit for bit, no case
left out.  Raw C-ABI launches go into outputs poisoned with 0xA5 that start at an odd address, with 1 MiB guards in front and
behind; every launch runs twice and must repeat itself.  One half of the cases goes through the raw ABI with tables packed by this
file's own loops, the other through ``ops`` and ``mask_utils``.  The references are computed once per module."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_refs as R                                                   # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 1 << 20
SIZES = [1, 31, 32, 33, 64, 65, 257]


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def box(x, y, bw, bh):
    return [x, y, x, y + bh, x + bw, y + bh, x + bw, y]


# ------------------------------------------------------------------------------------------------ this file's own packing
def pack_poly(objects, hws):
    """objects: list of lists of parts; the tables of seam_poly_masks_u8, by plain loops over the restatement's step 1."""
    pts, part_off, part_obj, edge_off, ws_off, out_off = [], [0], [], [0], [0], []
    pos = 0
    for o, (parts, (h, w)) in enumerate(zip(objects, hws)):
        out_off.append(pos)
        pos += h * w
        for xy in parts:
            X, Y = R.upsample(xy)
            k = len(X) - 1
            for j in range(k):
                pts.append((X[j], Y[j]))
                edge_off.append(edge_off[-1] + max(abs(X[j + 1] - X[j]), abs(Y[j + 1] - Y[j])) + 1)
            part_off.append(part_off[-1] + k)
            part_obj.append(o)
            ws_off.append(ws_off[-1] + w * ((h + 1 + 31) // 32))
    return dict(pts=np.asarray(pts, np.int32).reshape(-1, 2), part_off=np.asarray(part_off, np.int32),
                part_obj=np.asarray(part_obj, np.int32), edge_pt_off=np.asarray(edge_off, np.int32),
                part_ws_off=np.asarray(ws_off, np.int64), obj_hw=np.asarray(hws, np.int32).reshape(-1, 2),
                obj_out_off=np.asarray(out_off, np.int64), total=pos)


def pack_rle(objects, hws):
    starts, run_off, out_off, pos = [], [0], [], 0
    for counts, (h, w) in zip(objects, hws):
        out_off.append(pos)
        pos += h * w
        s = 0
        for c in counts:
            starts.append(s)
            s += c
        run_off.append(len(starts))
    return dict(run_start=np.asarray(starts, np.int32), obj_run_off=np.asarray(run_off, np.int32),
                obj_hw=np.asarray(hws, np.int32).reshape(-1, 2), obj_out_off=np.asarray(out_off, np.int64), total=pos)


def poisoned(total, shift):
    """total output bytes at address base + GUARD + shift, 0xA5 everywhere, guards on both sides."""
    raw = torch.full((GUARD + shift + total + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD + shift:GUARD + shift + total]


def guards_hold(raw, total, shift):
    return bool((raw[:GUARD + shift] == 0xA5).all()) and bool((raw[GUARD + shift + total:] == 0xA5).all())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def ptr(t):
    return t.data_ptr() if t.numel() else None


def abi_poly(lib, objects, hws, shift):
    t = pack_poly(objects, hws)
    d = {k: up(v) for k, v in t.items() if k != "total"}
    ws_bytes = 4 * int(t["part_ws_off"][-1])
    P, V, T = len(t["part_obj"]), len(t["pts"]), int(t["edge_pt_off"][-1])
    runs = []
    for _ in range(2):
        raw, out = poisoned(t["total"], shift)
        ws_raw = torch.full((ws_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = lib.seam_poly_masks_u8(ptr(d["pts"]), ptr(d["part_off"]), ptr(d["part_obj"]), ptr(d["edge_pt_off"]), ptr(d["part_ws_off"]),
                                    ptr(d["obj_hw"]), ptr(d["obj_out_off"]), out.data_ptr(), ws_raw.data_ptr() if ws_bytes else None,
                                    ws_bytes, P, V, T, len(hws), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert guards_hold(raw, t["total"], shift), "wrote outside the output"
        assert bool((ws_raw[ws_bytes:] == 0xA5).all()), "wrote past the workspace"
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]), "two launches differ"
    return [runs[0][o:o + h * w].reshape(h, w) for o, (h, w) in zip(t["obj_out_off"], hws)]


def abi_rle(lib, objects, hws, shift):
    t = pack_rle(objects, hws)
    d = {k: up(v) for k, v in t.items() if k != "total"}
    runs = []
    for _ in range(2):
        raw, out = poisoned(t["total"], shift)
        rc = lib.seam_rle_masks_u8(ptr(d["run_start"]), ptr(d["obj_run_off"]), ptr(d["obj_hw"]), ptr(d["obj_out_off"]), out.data_ptr(),
                                   len(hws), torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert guards_hold(raw, t["total"], shift), "wrote outside the output"
        runs.append(out.cpu().numpy())
    assert np.array_equal(runs[0], runs[1]), "two launches differ"
    return [runs[0][o:o + h * w].reshape(h, w) for o, (h, w) in zip(t["obj_out_off"], hws)]


def ops_poly(polys, sizes):
    """Through ops: the product's packing, a poisoned flat buffer handed to the launch, twice."""
    from seam_match_rcnn_amd import ops
    lay, t = ops.pack_poly_masks(polys, sizes)
    runs = []
    for _ in range(2):
        raw, flat = poisoned(lay.total, 0)
        views = ops.launch_poly_masks(lay, t, DEV, flat)
        torch.cuda.synchronize()
        assert guards_hold(raw, lay.total, 0)
        runs.append([v.cpu().numpy() for v in views])
    assert all(np.array_equal(a, b) for a, b in zip(*runs)), "two launches differ"
    return runs[0]


def check(got, want, what):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g.shape != w.shape or g.dtype != np.uint8 or not np.array_equal(g, w)]
    assert not bad, f"{what}: objects {bad[:10]} of {len(want)} differ from the restatement"


# ------------------------------------------------------------------------------------------------ the cases, made once
def sweep_objects(seed, n):
    """n seeded objects: 0 to 4 parts each (the first always of zero parts), free / half-integer / integer vertices up to 3 px
    outside, every third object integer-only with steps of at most 12 px (slopes whose s*t lands on half cases), repeated
    vertices and repeated edges planted into every fifth."""
    rng = np.random.default_rng(seed)
    objects, hws = [], []
    for i in range(n):
        h, w = int(rng.choice(SIZES)), int(rng.choice(SIZES))
        parts = []
        for _ in range(0 if i == 0 else int(rng.integers(1, 5))):
            xy = R.random_polygon(rng, h, w, small_steps=(i % 3 == 1))
            if i % 5 == 2 and len(xy) >= 4:
                xy = xy[:2] + xy[:2] + xy[2:] + xy[:4]                    # a zero-length edge, then an edge walked again
            parts.append(xy)
        if i % 7 == 3:                                                    # overlapping and disjoint integer boxes as extra parts
            parts = parts[:2] + [box(0, 0, max(w // 2, 1), max(h // 2, 1)), box(w // 4, h // 4, max(w // 2, 1), max(h // 2, 1))]
        objects.append(parts)
        hws.append((h, w))
    return objects, hws


@pytest.fixture(scope="module")
def sweep():
    objects, hws = sweep_objects(77, 300)
    return objects, hws, [R.poly_mask(p, h, w) for p, (h, w) in zip(objects, hws)]


HAND = [([[1, 1, 4, 1, 4, 3, 1, 3]], (5, 6)), ([[0.5, 0.5, 4.5, 0.5, 2.5, 4.5]], (5, 6)), ([[-1, -1, -1, 9, 9, 9, 9, -1]], (5, 6)),
        ([[2, 2]], (5, 6)), ([[1, 1, 4, 3]], (5, 6)), ([], (5, 6)), ([box(0, 0, 2, 3)], (5, 6)), ([box(2, 1, 3, 2)], (5, 6)),
        ([box(3, 3, 1, 1)], (5, 6)), ([box(4, 3, 2, 2)], (5, 6)), ([box(0, 0, 2, 2), box(1, 1, 3, 2)], (5, 6)),
        ([[0, 0, 1, 0, 1, 1, 0, 1]], (1, 1))]
# Integer polygons on 33 x 33 on which ys + s*t computed as ONE fused multiply-add changes a pixel (slopes like 5/6 whose product
# with t is a tie in float64; found by searching 60000 seeded polygons with exact rational arithmetic -- one in 10^4 is such a
# case, so the sweep alone would hardly notice a contracted kernel).
HALF_CASES = [[11, 6, 16, 17, 21, 10, 27, 5, 25, 1], [5, 12, 9, 15, 0, 26], [8, 5, 12, 10, 22, 0], [34, 2, 25, 4, 15, -3, 10, 7],
              [36, 1, 29, 12, 18, 16]]


def test_hand_answers_raw_abi_and_ops(lib):
    objects, hws = [p for p, _ in HAND], [hw for _, hw in HAND]
    want = [R.poly_mask(p, h, w) for p, (h, w) in HAND]
    assert want[0][1:3, 1:4].all() and int(want[0].sum()) == 6 and int(want[2].sum()) == 30 and int(want[3].sum()) == 0
    check(abi_poly(lib, objects, hws, shift=3), want, "hand answers, raw ABI")
    got = ops_poly([objects[:-1], objects[-1:]], [(5, 6), (1, 1)])
    check(list(got[0]) + list(got[1]), want, "hand answers, ops")


def test_unfused_multiply_add_decides_pixels(lib):
    objects, hws = [[xy] for xy in HALF_CASES], [(33, 33)] * len(HALF_CASES)
    want = [R.poly_mask(p, 33, 33) for p in objects]
    check(abi_poly(lib, objects, hws, shift=0), want, "half cases, raw ABI")
    check(list(ops_poly([objects], [(33, 33)])[0]), want, "half cases, ops")


def test_sweep_first_half_raw_abi(lib, sweep):
    objects, hws, want = sweep
    check(abi_poly(lib, objects[:150], hws[:150], shift=5), want[:150], "sweep, raw ABI")


def test_sweep_second_half_ops_and_mask_utils(sweep):
    from seam_match_rcnn_amd import mask_utils as M
    objects, hws, want = sweep
    objects, hws, want = objects[150:], hws[150:], want[150:]
    by_size = {}
    for i, hw in enumerate(hws):
        by_size.setdefault(hw, []).append(i)
    sizes = list(by_size)
    assert len(sizes) >= 6                                            # one batch mixing image sizes in a single launch
    got = ops_poly([[objects[i] for i in by_size[hw]] for hw in sizes], sizes)
    for hw, stack in zip(sizes, got):
        assert stack.shape == (len(by_size[hw]), *hw)
        check(list(stack), [want[i] for i in by_size[hw]], f"sweep, ops, images of {hw}")
    six = sizes[:6]
    stacks = M.masks_from_annotations([[{"segmentation": objects[i]} for i in by_size[hw]] for hw in six], six, DEV)
    for hw, stack in zip(six, stacks):
        assert stack.dtype == torch.uint8 and stack.is_contiguous() and stack.device.type == "cuda"
        check(list(stack.cpu().numpy()), [want[i] for i in by_size[hw]], f"sweep, masks_from_annotations, images of {hw}")


def wavy_polygon(rng, cx, cy, radius, k):
    th = np.sort(rng.uniform(0, 2 * np.pi, k))
    r = radius * (0.75 + 0.2 * np.sin(rng.integers(2, 7) * th + rng.uniform(0, 6.28))) + rng.uniform(-3, 3, k)
    xy = np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], 1)
    return [float(v) for v in np.round(xy.reshape(-1), 2)]                # DeepFashion2 stores two decimals at most


def test_workload_shape_800x1216_eight_objects():
    from seam_match_rcnn_amd import ops
    rng = np.random.default_rng(8)
    h, w = 800, 1216
    objs = []
    for i in range(8):
        k = [40, 300, 77, 150, 41, 299, 120, 64][i]
        parts = [wavy_polygon(rng, rng.uniform(0, w), rng.uniform(0, h), rng.uniform(60, 420), k)]
        if i % 3 == 0:
            parts.append(wavy_polygon(rng, rng.uniform(0, w), rng.uniform(0, h), 90.0, 40))
        objs.append(parts)
    got = ops.poly_masks([objs], [(h, w)], DEV)[0]
    again = ops.poly_masks([objs], [(h, w)], DEV)[0]
    assert got.shape == (8, h, w) and torch.equal(got, again)
    got = got.cpu().numpy()
    want = [R.poly_mask(p, h, w) for p in objs]
    assert all(1000 < int(m.sum()) for m in want)
    check(list(got), want, "800 x 1216")


# ------------------------------------------------------------------------------------------------ RLE
@pytest.fixture(scope="module")
def rle_sweep():
    rng = np.random.default_rng(901)
    objects, hws = [], []
    for i in range(100):
        h, w = int(rng.choice(SIZES)), int(rng.choice(SIZES))
        objects.append(R.random_counts(rng, h, w, max_runs=int(rng.choice([1, 2, 3, 12, 200])), zero_runs=(i % 2 == 0)))
        hws.append((h, w))
    objects += [[33 * 65], [0, 33 * 65], [0, 0, 0, 33 * 65], [1, 0, 0, 1, 33 * 65 - 2], [7, 0, 33 * 65 - 7], [0, 1, 33 * 65 - 2, 1]]
    hws += [(33, 65)] * 6                          # all zeros, all ones, zero-length runs at the start, inside and of both values
    return objects, hws, [R.rle_decode(c, h, w) for c, (h, w) in zip(objects, hws)]


def test_rle_raw_abi(lib, rle_sweep):
    objects, hws, want = rle_sweep
    assert int(want[100].sum()) == 0 and int(want[101].sum()) == 33 * 65
    half = len(objects) // 2
    check(abi_rle(lib, objects[:half], hws[:half], shift=1), want[:half], "RLE, raw ABI")
    check(abi_rle(lib, objects[-6:], hws[-6:], shift=7), want[-6:], "RLE edge cases, raw ABI")


def test_rle_ops_and_ann_to_mask(rle_sweep):
    from seam_match_rcnn_amd import mask_utils as M
    from seam_match_rcnn_amd import ops
    objects, hws, want = rle_sweep
    half = len(objects) // 2
    objects, hws, want = objects[half:], hws[half:], want[half:]
    by_size = {}
    for i, hw in enumerate(hws):
        by_size.setdefault(hw, []).append(i)
    sizes = list(by_size)
    got = ops.rle_masks([[objects[i] for i in by_size[hw]] for hw in sizes], sizes, DEV)
    again = ops.rle_masks([[objects[i] for i in by_size[hw]] for hw in sizes], sizes, DEV)
    for hw, stack, rep in zip(sizes, got, again):
        assert torch.equal(stack, rep)
        check(list(stack.cpu().numpy()), [want[i] for i in by_size[hw]], f"RLE, ops, images of {hw}")
    for i in list(range(0, len(objects), 6)) + list(range(len(objects) - 6, len(objects))):     # compressed strings, bytes, plain lists
        h, w = hws[i]
        s = R.rle_to_string(objects[i])
        for counts in (s, s.encode(), objects[i]):
            m = M.annToMask({"segmentation": {"counts": counts, "size": [h, w]}}, [h, w])
            assert isinstance(m, np.ndarray) and m.dtype == np.uint8 and np.array_equal(m, want[i]), (i, type(counts))
    m = M.annToMask({"segmentation": HAND[1][0]}, [5, 6])
    assert np.array_equal(m, R.poly_mask(HAND[1][0], 5, 6))


# ------------------------------------------------------------------------------------------------ end to end
def test_targets_to_device_feeds_the_evaluator_and_the_resize():
    """Annotations -> ``targets_to_device`` -> ``DetectionEvaluator``: the AP equals, exactly, the AP over masks made by the
    restatement; polygon, multi-part, uncompressed and compressed RLE objects share the images."""
    from seam_match_rcnn_amd import evaluator_det as E
    from seam_match_rcnn_amd import mask_utils as M
    from seam_match_rcnn_amd.models.matchrcnn import resize_masks_nearest
    rng = np.random.default_rng(4)
    sizes = [(90, 120), (75, 64)]
    def counts_of(mask):                                                  # plain run lengths of the column-major bytes
        flat = np.concatenate([[0], mask.T.reshape(-1)])
        return np.diff(np.concatenate([[0], np.flatnonzero(np.diff(flat)), [mask.size]])).tolist()

    blob, slab = R.poly_mask([wavy_polygon(rng, 30, 40, 25, 30)], 75, 64), R.poly_mask([box(5, 15, 50, 50)], 75, 64)
    assert np.array_equal(R.rle_decode(counts_of(blob), 75, 64), blob) and np.array_equal(R.rle_decode(counts_of(slab), 75, 64), slab)
    segs = [[[box(10, 8, 40, 52)], [wavy_polygon(rng, 85, 50, 28, 60)], [box(20, 60, 25, 25), box(70, 5, 30, 13)]],
            [{"counts": counts_of(blob), "size": [75, 64]}, {"counts": R.rle_to_string(counts_of(slab)), "size": [75, 64]},
             [box(30, 10, 30, 30)]]]
    gt_boxes = [torch.tensor([[10., 8, 50, 60], [57, 22, 113, 78], [20, 5, 100, 85]]), torch.tensor([[5., 15, 55, 65], [5, 15, 55, 65], [30, 10, 60, 40]])]
    labels = [torch.tensor([1, 2, 1]), torch.tensor([2, 2, 3])]
    targets = [dict(boxes=b, labels=l, segmentation=s, size=hw, image_id=i) for i, (b, l, s, hw) in enumerate(zip(gt_boxes, labels, segs, sizes))]
    moved = M.targets_to_device(targets, DEV)
    ref_targets = []
    for t, m, (h, w) in zip(targets, moved, sizes):
        assert set(m) == {"boxes", "labels", "masks", "image_id"} and m["boxes"].is_cuda and m["image_id"] == t["image_id"]
        want = np.stack([R.ann_mask(s, h, w) for s in t["segmentation"]])
        assert m["masks"].dtype == torch.uint8 and m["masks"].is_cuda and m["masks"].is_contiguous() and tuple(m["masks"].shape) == want.shape
        assert np.array_equal(m["masks"].cpu().numpy(), want) and want.reshape(len(want), -1).any(1).all()
        ref_targets.append(dict(boxes=t["boxes"], labels=t["labels"], masks=torch.from_numpy(want)))
        same = resize_masks_nearest(m["masks"], (h, w))
        assert same.data_ptr() == m["masks"].data_ptr() and same.dtype == torch.uint8
        small = resize_masks_nearest(m["masks"], (h // 2, w // 3))
        ref_small = resize_masks_nearest(torch.from_numpy(want), (h // 2, w // 3))
        assert small.dtype == torch.uint8 and small.is_contiguous() and torch.equal(small.cpu(), ref_small)
    g = torch.Generator().manual_seed(1)
    outputs = []
    for b, l in zip(gt_boxes, labels):                                   # fixed fake detections: shifted ground-truth boxes, soft disks
        k = 6
        boxes = (b.repeat(2, 1) + torch.randint(-6, 7, (k, 4), generator=g).float()).clamp(min=0)
        yy, xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing="ij")
        probs = torch.stack([(((yy - 13.5) ** 2 + (xx - 13.5) ** 2) <= r * r).float() * 0.9 for r in (14., 12., 13., 10., 15., 11.)])[:, None]
        outputs.append(dict(boxes=boxes.to(DEV), labels=l.repeat(2).to(DEV), scores=torch.linspace(0.9, 0.3, k).to(DEV), mask_probs=probs.to(DEV)))
    ev, ref = E.DetectionEvaluator(), E.DetectionEvaluator()
    ev.update(outputs, moved)
    ref.update(outputs, ref_targets)
    got, want = ev.summarize(verbose=False), ref.summarize(verbose=False)
    assert got["segm"] == want["segm"] and got["bbox"] == want["bbox"]
    assert any(v not in (-1.0, 0.0) for v in got["segm"])
