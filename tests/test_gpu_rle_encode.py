"""GPU: csrc/seam_rle.hip against the host restatement of rleEncode (tests/rle_refs.py), bit for bit, no case left out.  Raw
C-ABI launches read an input that starts at an odd address and write workspace, counts and positions poisoned with 0xA5 behind
1 MiB guards; every launch runs twice and must repeat itself; the tables are packed by this file's own loops.  The paste route is
held against the existing ``seam_paste_masks_f32`` output ``> 0.5`` and against ``seam_mask_inter_f32``'s ``det_area``.  Then the
same through ``ops``, ``mask_utils`` and ``evaluator_det.coco_results``.  The references are computed once per module."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mask_refs as MR                                                  # noqa: E402
import rle_refs as R                                                    # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
GUARD = 1 << 20
SHAPES = [(1, 1), (1, 65), (65, 1), (31, 33), (32, 32), (33, 31), (64, 257), (257, 65)]
HALF_UP = float(np.nextafter(np.float32(0.5), np.float32(1.0)))


@pytest.fixture(scope="module")
def lib():
    from seam_match_rcnn_amd import _native
    return _native.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def contents(h, w, rng):
    """name -> uint8 [h,w]"""
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"zeros": np.zeros((h, w), np.uint8), "ones": np.ones((h, w), np.uint8),
           "checker": ((yy + xx) % 2).astype(np.uint8), "checker_set_first": ((yy + xx + 1) % 2).astype(np.uint8),
           "alt_columns": (xx % 2).astype(np.uint8).copy(),
           "alternating": ((xx * h + yy) % 2).astype(np.uint8), "alternating_set_first": ((xx * h + yy + 1) % 2).astype(np.uint8)}
    for name, (y, x) in {"tl": (0, 0), "tr": (0, w - 1), "bl": (h - 1, 0), "br": (h - 1, w - 1)}.items():
        m = np.zeros((h, w), np.uint8)
        m[y, x] = 1
        out["corner_" + name] = m
    carry = np.zeros((h, w), np.uint8)                                   # bottom row + top row of the next column
    carry[h - 1, 0:w:2] = 1
    carry[0, 1:w:2] = 1
    out["carry"] = carry
    last = (rng.random((h, w)) < 0.3).astype(np.uint8)
    last[h - 1, w - 1] = 1
    out["set_last_pixel"] = last
    for p in (0.02, 0.5, 0.98):
        out[f"random_{p}"] = (rng.random((h, w)) < p).astype(np.uint8)
    out["bytes_2_255_1"] = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=(h, w))
    return out


@pytest.fixture(scope="module")
def dense():
    """(names, masks, counts by the restatement), every shape x every content"""
    rng = np.random.default_rng(31)
    names, masks = [], []
    for h, w in SHAPES:
        for name, m in contents(h, w, rng).items():
            names.append(f"{h}x{w} {name}")
            masks.append(m)
    want = [R.rle_encode(m) for m in masks]
    for h, w in SHAPES:                                                  # the capacity case: a boundary at every position
        assert want[names.index(f"{h}x{w} alternating")] == [1] * (h * w)
        assert want[names.index(f"{h}x{w} alternating_set_first")] == [0] + [1] * (h * w)
    return names, masks, want


# ------------------------------------------------------------------------------------------------ raw ABI
def poisoned(nbytes):
    """nbytes at a 1 MiB offset into a buffer of 0xA5, guards on both sides -> (whole buffer, the middle)"""
    raw = torch.full((GUARD + nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    return raw, raw[GUARD:GUARD + nbytes]


def untouched(raw, nbytes):
    return bool((raw[:GUARD] == 0xA5).all()) and bool((raw[GUARD + nbytes:] == 0xA5).all())


def up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def counts_from(positions, ends, hws):
    out, lo = [], 0
    for hi, (h, w) in zip(ends, hws):
        p = [int(v) for v in positions[lo:hi]]
        assert all(a < b for a, b in zip(p, p[1:])) and (not p or (0 <= p[0] and p[-1] < h * w)), "positions must ascend inside the mask"
        edges = [0] + p + [h * w]
        out.append([b - a for a, b in zip(edges, edges[1:])])
        lo = hi
    return out


def finish(positions_call, counts, last_cell, hws):
    """The caller's half: inclusive scan, then the positions kernel into a poisoned buffer of exactly the total."""
    scan = torch.cumsum(counts.view(torch.int32), 0)
    assert scan.dtype == torch.int64
    ends = [int(v) for v in scan[torch.as_tensor(last_cell, device=DEV)].cpu()]
    total = ends[-1]
    pos_raw, pos = poisoned(4 * total)
    rc = positions_call(scan, pos.data_ptr() if total else None, total)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert untouched(pos_raw, 4 * total), "wrote outside the positions"
    got = pos.cpu().numpy().view(np.int32)
    return counts_from(got, ends, hws), got.tobytes()


def abi_dense(lib, masks, shift=1):
    hws = [m.shape for m in masks]
    obj_off, cell_off, nbytes, cells = [], [0], 0, 0
    for h, w in hws:                                                     # this file's own packing
        obj_off.append(nbytes)
        nbytes += h * w
        cells += ((h + 31) // 32) * w
        cell_off.append(cells)
    hw_host = np.ascontiguousarray(np.asarray(hws, np.int32).reshape(-1, 2))
    src_raw = torch.empty((shift + nbytes,), dtype=torch.uint8, device=DEV)
    src = src_raw[shift:]
    assert src.data_ptr() % 2 == 1                                       # the input starts at an odd address
    src.copy_(up(np.concatenate([m.reshape(-1) for m in masks])))
    d_hw, d_off, d_cell = up(hw_host), up(np.asarray(obj_off, np.int64)), up(np.asarray(cell_off, np.int64))
    n, runs = len(masks), []
    for _ in range(2):
        ws_raw, ws = poisoned(4 * cells)
        ct_raw, ct = poisoned(4 * cells)
        rc = lib.seam_rle_encode_masks_u8(src.data_ptr(), nbytes, hw_host.ctypes.data, d_hw.data_ptr(), d_off.data_ptr(),
                                          d_cell.data_ptr(), ws.data_ptr(), 4 * cells, ct.data_ptr(), n, stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(ws_raw, 4 * cells) and untouched(ct_raw, 4 * cells), "wrote outside the workspace or the counts"

        def positions(scan, pos_ptr, total):
            return lib.seam_rle_positions_masks(hw_host.ctypes.data, d_hw.data_ptr(), d_cell.data_ptr(), ws.data_ptr(), 4 * cells,
                                                scan.data_ptr(), pos_ptr, total, n, stream())

        got, raw_pos = finish(positions, ct, [c - 1 for c in cell_off[1:]], hws)
        runs.append((got, raw_pos, ws.cpu().numpy().tobytes(), ct.cpu().numpy().tobytes()))
    assert runs[0][1:] == runs[1][1:], "two launches differ"
    return runs[0][0]


def abi_paste(lib, probs, boxes, h, w):
    d = probs.shape[0]
    per = ((h + 31) // 32) * w
    assert int(lib.seam_rle_encode_ws_bytes(h, w)) == 4 * per
    cells, runs = per * d, []
    for _ in range(2):
        ws_raw, ws = poisoned(4 * cells)
        ct_raw, ct = poisoned(4 * cells)
        rc = lib.seam_rle_encode_paste_f32(probs.data_ptr(), boxes.data_ptr(), d, h, w, ws.data_ptr(), 4 * cells, ct.data_ptr(), stream())
        assert rc == 0, rc
        torch.cuda.synchronize()
        assert untouched(ws_raw, 4 * cells) and untouched(ct_raw, 4 * cells), "wrote outside the workspace or the counts"

        def positions(scan, pos_ptr, total):
            return lib.seam_rle_positions_paste(d, h, w, ws.data_ptr(), 4 * cells, scan.data_ptr(), pos_ptr, total, stream())

        got, raw_pos = finish(positions, ct, [per * (i + 1) - 1 for i in range(d)], [(h, w)] * d)
        runs.append((got, raw_pos, ws.cpu().numpy().tobytes(), ct.cpu().numpy().tobytes()))
    assert runs[0][1:] == runs[1][1:], "two launches differ"
    return runs[0][0]


def differing(got, want):
    return [i for i, (g, c) in enumerate(zip(got, want)) if [int(v) for v in g] != [int(v) for v in c]]


def test_dense_one_batch_of_every_shape_and_content(lib, dense):
    names, masks, want = dense
    got = abi_dense(lib, masks, shift=1)
    bad = differing(got, want)
    assert len(got) == len(want) and not bad, [names[i] for i in bad[:10]]


def test_dense_every_object_singly(lib, dense):
    names, masks, want = dense
    bad = [names[i] for i, m in enumerate(masks) if differing(abi_dense(lib, [m], shift=1 + 2 * (i % 3)), [want[i]])]
    assert not bad, bad[:10]


def test_refusals_leave_the_poison(lib):
    m = np.ones((33, 31), np.uint8)
    h, w = m.shape
    cells = 2 * w
    hw_ok = np.asarray([[h, w]], np.int32)
    src, d_hw, d_off, d_cell = up(m.reshape(-1)), up(hw_ok), up(np.zeros(1, np.int64)), up(np.asarray([0, cells], np.int64))
    ws_raw, ws = poisoned(4 * cells)
    ct_raw, ct = poisoned(4 * cells)
    ps_raw, ps = poisoned(4 * cells * 32)
    scan = torch.full((cells,), 2, dtype=torch.int64, device=DEV)
    probs, boxes = torch.ones((2, 28, 28), device=DEV), torch.tensor([[1.0, 1.0, 20.0, 20.0]] * 2, device=DEV)
    S, P, H, O, Cc, W, Ct, Sc, Ps = src.data_ptr(), hw_ok.ctypes.data, d_hw.data_ptr(), d_off.data_ptr(), d_cell.data_ptr(), \
        ws.data_ptr(), ct.data_ptr(), scan.data_ptr(), ps.data_ptr()
    enc, pos, encp, posp = lib.seam_rle_encode_masks_u8, lib.seam_rle_positions_masks, lib.seam_rle_encode_paste_f32, lib.seam_rle_positions_paste
    B, s, cap = 4 * cells, stream(), cells * 32
    bad_hw = [np.asarray([[0, w]], np.int32), np.asarray([[h, 0]], np.int32), np.asarray([[16385, 1]], np.int32), np.asarray([[1, 16385]], np.int32)]
    refused = [
        enc(None, h * w, P, H, O, Cc, W, B, Ct, 1, s), enc(S, h * w, None, H, O, Cc, W, B, Ct, 1, s), enc(S, h * w, P, None, O, Cc, W, B, Ct, 1, s),
        enc(S, h * w, P, H, None, Cc, W, B, Ct, 1, s), enc(S, h * w, P, H, O, None, W, B, Ct, 1, s), enc(S, h * w, P, H, O, Cc, None, B, Ct, 1, s),
        enc(S, h * w, P, H, O, Cc, W, B, None, 1, s), enc(S, h * w, P, H, O, Cc, W, B, Ct, -1, s), enc(S, h * w, P, H, O, Cc, W, B - 4, Ct, 1, s),
        enc(S, h * w, P, H, O, Cc, W, B + 2, Ct, 1, s),
        pos(None, H, Cc, W, B, Sc, Ps, cap, 1, s), pos(P, None, Cc, W, B, Sc, Ps, cap, 1, s), pos(P, H, None, W, B, Sc, Ps, cap, 1, s),
        pos(P, H, Cc, None, B, Sc, Ps, cap, 1, s), pos(P, H, Cc, W, B, None, Ps, cap, 1, s), pos(P, H, Cc, W, B, Sc, None, cap, 1, s),
        pos(P, H, Cc, W, B, Sc, Ps, cap, -1, s), pos(P, H, Cc, W, B, Sc, Ps, -1, 1, s),
        encp(None, boxes.data_ptr(), 2, 20, 30, W, B, Ct, s), encp(probs.data_ptr(), None, 2, 20, 30, W, B, Ct, s),
        encp(probs.data_ptr(), boxes.data_ptr(), 2, 20, 30, None, B, Ct, s), encp(probs.data_ptr(), boxes.data_ptr(), 2, 20, 30, W, B, None, s),
        encp(probs.data_ptr(), boxes.data_ptr(), -1, 20, 30, W, B, Ct, s), encp(probs.data_ptr(), boxes.data_ptr(), 2, 0, 30, W, B, Ct, s),
        encp(probs.data_ptr(), boxes.data_ptr(), 2, 20, 0, W, B, Ct, s), encp(probs.data_ptr(), boxes.data_ptr(), 2, 16385, 1, W, B, Ct, s),
        encp(probs.data_ptr(), boxes.data_ptr(), 2, 1, 16385, W, B, Ct, s), encp(probs.data_ptr(), boxes.data_ptr(), 2, 64, 64, W, B, Ct, s),
        posp(2, 20, 30, None, B, Sc, Ps, cap, s), posp(2, 20, 30, W, B, None, Ps, cap, s), posp(2, 20, 30, W, B, Sc, None, cap, s),
        posp(-1, 20, 30, W, B, Sc, Ps, cap, s), posp(2, 0, 30, W, B, Sc, Ps, cap, s), posp(2, 20, 16385, W, B, Sc, Ps, cap, s),
    ]
    for t in bad_hw:
        refused += [enc(S, h * w, t.ctypes.data, H, O, Cc, W, B, Ct, 1, s), pos(t.ctypes.data, H, Cc, W, B, Sc, Ps, cap, 1, s)]
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused), refused
    assert lib.seam_rle_encode_ws_bytes(0, 5) == 0 and lib.seam_rle_encode_ws_bytes(5, 16385) == 0 and lib.seam_rle_encode_ws_bytes(-1, 5) == 0
    assert lib.seam_rle_encode_ws_bytes(16384, 16384) == 4 * 512 * 16384 and lib.seam_rle_encode_ws_bytes(33, 31) == 4 * 2 * 31
    # n == 0 / D == 0 are no-ops that return 0, whatever else is passed
    assert enc(None, 0, None, None, None, None, None, 0, None, 0, s) == 0 and pos(None, None, None, None, 0, None, None, 0, 0, s) == 0
    assert encp(None, None, 0, 0, 0, None, 0, None, s) == 0 and posp(0, 0, 0, None, 0, None, None, 0, s) == 0
    torch.cuda.synchronize()
    for raw in (ws_raw, ct_raw, ps_raw):
        assert bool((raw == 0xA5).all()), "a refused or empty call wrote something"
    # the wrappers' own checks
    from seam_match_rcnn_amd import ops
    with pytest.raises(ValueError):
        ops.rle_encode_paste(probs, boxes[:1], (20, 30))
    with pytest.raises(ValueError):
        ops.rle_encode_paste(probs, boxes, (0, 30))
    with pytest.raises(ValueError):
        ops.rle_encode(src[:5], ops.mask_layout([1], [(h, w)]))
    assert ops.rle_encode_paste(probs[:0], boxes[:0], (20, 30)) == [] and ops.rle_encode(src[:0], ops.mask_layout([0], [(h, w)])) == []


# ------------------------------------------------------------------------------------------------ the paste route
def detections(h, w, seed):
    """12 detections: boxes of every awkward kind, maps random / holding exact 0.5 values / all below / all above 0.5"""
    rng = np.random.default_rng(seed)
    fw, fh = float(w), float(h)
    boxes = [[0.2 * fw, 0.3 * fh, 0.7 * fw, 0.8 * fh],                   # inside
             [-0.3 * fw, 0.2 * fh, 0.4 * fw, 0.6 * fh],                  # over the left edge
             [0.3 * fw, -0.4 * fh, 0.8 * fw, 0.5 * fh],                  # over the top edge
             [0.6 * fw, 0.1 * fh, 1.3 * fw, 0.7 * fh],                   # over the right edge
             [0.1 * fw, 0.5 * fh, 0.6 * fw, 1.4 * fh],                   # over the bottom edge
             [-5.0, -7.0, fw + 6.0, fh + 9.0],                           # the whole image and more: reaches the last row
             [fw + 5.0, fh + 3.0, 2.0 * fw + 9.0, 2.0 * fh + 7.0],       # fully outside
             [0.4 * fw, 0.2 * fh, 0.4 * fw, 0.9 * fh],                   # degenerate, x0 == x1
             [0.8 * fw, 0.7 * fh, 0.2 * fw, 0.1 * fh],                   # inverted
             [0.5 * fw + 0.1, 0.5 * fh + 0.2, 0.5 * fw + 0.4, 0.5 * fh + 0.4],     # sub-pixel
             [0.0, 0.0, fw, fh],                                         # exactly the image
             [0.05 * fw, 0.0, 0.95 * fw, fh + 3.0]]                      # full height, inside in x: a run ends at the last row
    maps = rng.uniform(0, 1, size=(12, 28, 28)).astype(np.float32)
    maps[1][rng.random((28, 28)) < 0.5] = 0.5                            # exact 0.5 values among random ones
    maps[2][:] = 0.5
    maps[3][:] = rng.uniform(0.0, 0.4999, size=(28, 28))                # all < 0.5
    maps[4][:] = rng.uniform(0.5001, 1.0, size=(28, 28))                # all > 0.5
    maps[5][:] = 1.0
    maps[6][:] = 1.0
    maps[7][:] = 1.0
    maps[10][:] = HALF_UP
    maps[11][:] = rng.uniform(0.5001, 1.0, size=(28, 28))
    return torch.from_numpy(maps).to(DEV), torch.tensor(boxes, dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("hw", [(65, 97), (257, 33)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_paste_route_equals_the_thresholded_paste(lib, hw):
    from seam_match_rcnn_amd import mask_utils as M
    from seam_match_rcnn_amd import ops
    h, w = hw
    probs, boxes = detections(h, w, seed=h)
    pasted = (ops.paste_masks(probs[:, None], boxes, (h, w))[:, 0] > 0.5).to(torch.uint8)
    dense_masks = pasted.cpu().numpy()
    want = [R.rle_encode(m) for m in dense_masks]
    area = ops.mask_inter(probs, boxes, torch.empty((0, h, w), dtype=torch.uint8, device=DEV))[1].tolist()
    assert area[5] > 0.9 * h * w and dense_masks[5][h - 1].all() and area[6] == 0 and area[8] == 0 and area[2] == 0 and area[3] == 0
    assert area[0] > 0 and area[1] > 0 and area[4] > 0 and area[10] > 0 and dense_masks[11][h - 1].any() and dense_masks[4][h - 1].any()
    got = abi_paste(lib, probs, boxes, h, w)
    bad = differing(got, want)
    assert not bad, bad
    assert [R.rle_area(c) for c in got] == area                          # the set seam_mask_inter_f32 counts
    for route in (ops.rle_encode_paste(probs, boxes, (h, w)), ops.rle_encode_paste(probs[:, None], boxes, (h, w))):
        assert all(isinstance(c, np.ndarray) and c.dtype == np.int64 for c in route) and not differing(route, want)
    shifted = torch.cat([boxes.new_zeros(1), boxes.reshape(-1)])[1:].reshape(-1, 4)      # boxes off the 16-byte grid
    assert shifted.data_ptr() % 16 and not differing(ops.rle_encode_paste(probs, shifted, (h, w)), want)
    rles = M.encode_detections(probs[:, None], boxes, (h, w))
    assert rles == M.encode(pasted) and [r["size"] for r in rles] == [[h, w]] * 12
    assert [M.rle_from_string(r["counts"]) for r in rles] == want and M.area(rles).tolist() == area


# ------------------------------------------------------------------------------------------------ through the module
def test_mask_utils_round_trip(dense):
    from seam_match_rcnn_amd import mask_utils as M
    names, masks, want = dense
    for hw in ((31, 33), (64, 257)):
        idx = [i for i, m in enumerate(masks) if m.shape == hw]
        stack = np.stack([masks[i] for i in idx])                        # [n,h,w]
        c_order = np.ascontiguousarray(stack.transpose(1, 2, 0))         # [h,w,n], C order
        f_order = np.asfortranarray(c_order)
        assert c_order.flags.c_contiguous and f_order.flags.f_contiguous and not f_order.flags.c_contiguous
        from_dev, from_c, from_f = M.encode(torch.from_numpy(stack).to(DEV)), M.encode(c_order), M.encode(f_order)
        assert from_dev == from_c == from_f and len(from_dev) == len(idx)
        for r, i in zip(from_dev, idx):
            assert r["size"] == list(hw) and isinstance(r["counts"], bytes) and M.rle_from_string(r["counts"]) == want[i], names[i]
        back = M.decode(from_dev)
        assert back.dtype == np.uint8 and back.shape == (*hw, len(idx)) and back.flags.f_contiguous
        assert np.array_equal(back, (c_order != 0).astype(np.uint8))
        on_dev = M.decode(from_dev, keep_on_device=True)
        assert on_dev.is_cuda and on_dev.dtype == torch.uint8 and np.array_equal(on_dev.cpu().numpy(), (stack != 0).astype(np.uint8))
        one = M.encode(masks[idx[3]])
        assert one == from_dev[3] and np.array_equal(M.decode(one), (masks[idx[3]] != 0).astype(np.uint8))
        assert M.area(from_dev).tolist() == [R.rle_area(want[i]) for i in idx] == [int((masks[i] != 0).sum()) for i in idx]
        assert M.toBbox(from_dev).tolist() == [R.rle_to_bbox(want[i], *hw) for i in idx]


def test_ann_to_rle_and_mask_iou():
    from seam_match_rcnn_amd import mask_utils as M
    h, w = 75, 64
    polys = [[[5.0, 15.0, 5.0, 65.0, 55.0, 65.0, 55.0, 15.0]], [[10.5, 3.2, 60.1, 20.7, 33.3, 70.9]],
             [[1.0, 1.0, 20.0, 1.0, 20.0, 12.0, 1.0, 12.0], [30.0, 40.0, 62.0, 44.0, 40.0, 73.0]]]
    rles = [M.annToRLE({"segmentation": p}, [h, w]) for p in polys]
    for p, r in zip(polys, rles):
        m = M.annToMask({"segmentation": p}, [h, w])
        assert np.array_equal(m, MR.poly_mask(p, h, w)) and m.any()
        assert r == M.encode(m) and M.rle_from_string(r["counts"]) == R.rle_encode(m)
        assert M.annToRLE({"segmentation": r}, [h, w]) is r
        unc = {"size": [h, w], "counts": R.rle_encode(m)}
        assert M.annToRLE({"segmentation": unc}, [h, w]) == r
    rng = np.random.default_rng(3)
    extra = [(rng.random((h, w)) < p).astype(np.uint8) for p in (0.1, 0.6)] + [np.zeros((h, w), np.uint8)]
    dt = rles + [M.encode(m) for m in extra]
    gt = [rles[0], M.encode(extra[1]), rles[2], M.encode(extra[2])]
    crowd = [0, 1, 1, 0]
    dm = [MR.poly_mask(p, h, w) for p in polys] + extra
    gm = [dm[0], extra[1], dm[2], extra[2]]
    want = np.zeros((len(dt), len(gt)))
    for i, a in enumerate(dm):
        for j, b in enumerate(gm):
            inter = int(((a != 0) & (b != 0)).sum())
            den = int(a.sum()) if crowd[j] else int(a.sum()) + int(b.sum()) - inter
            want[i, j] = inter / den if den else 0.0
    got = M.iou(dt, gt, crowd)
    assert got.dtype == np.float64 and np.array_equal(got, want) and got[0, 0] == 1.0 and 0 < got[3, 1] < 1


def test_coco_results_close_the_evaluator_loop():
    """mask_probs -> coco_results -> decode -> the evaluator's pasted-mask route: the same AP, to the last bit, as the
    evaluator's own paste-free route; and the export is a JSON document."""
    from seam_match_rcnn_amd import evaluator_det as E
    from seam_match_rcnn_amd import mask_utils as M
    h, w = 97, 65
    yy, xx = torch.meshgrid(torch.arange(28.), torch.arange(28.), indexing="ij")
    disks = torch.stack([(((yy - 13.5) ** 2 + (xx - 13.5) ** 2) <= r * r).float() * 0.9 for r in (14., 12., 13., 10., 15., 11., 9.)])
    gt_boxes = torch.tensor([[5., 8., 40., 60.], [20., 30., 64., 96.], [0., 60., 30., 97.]])
    gt_labels = torch.tensor([1, 2, 1])
    gt_masks = torch.stack([torch.from_numpy(MR.poly_mask([[x0, y0, x0, y1, x1, y1, x1, y0]], h, w)) for x0, y0, x1, y1 in gt_boxes.tolist()])
    g = torch.Generator().manual_seed(9)
    boxes = (torch.cat([gt_boxes, gt_boxes, gt_boxes[:1]]) + torch.randint(-5, 6, (7, 4), generator=g).float())
    out = dict(boxes=boxes.to(DEV), labels=torch.tensor([1, 2, 1, 1, 2, 2, 1]).to(DEV), scores=torch.linspace(0.95, 0.2, 7).to(DEV),
               mask_probs=disks[:, None].to(DEV))
    tgt = dict(boxes=gt_boxes, labels=gt_labels, masks=gt_masks.to(DEV))
    res = E.coco_results([out], [42], [(h, w)], label_to_category=[0, 101, 102])
    assert json.loads(json.dumps(res)) == res and len(res) == 7
    assert [r["category_id"] for r in res] == [101, 102, 101, 101, 102, 102, 101] and all(r["image_id"] == 42 for r in res)
    assert all(isinstance(r["segmentation"]["counts"], str) and r["segmentation"]["size"] == [h, w] for r in res)
    assert [r["bbox"] for r in res] == [[float(v[k]) for v in E._xywh(boxes.numpy())] for k in range(7)]
    decoded = M.decode([r["segmentation"] for r in res], keep_on_device=True)
    assert tuple(decoded.shape) == (7, h, w) and all(int(d.sum()) > 0 for d in decoded)
    pasted = dict(boxes=out["boxes"], labels=out["labels"], scores=out["scores"], masks=decoded[:, None].to(torch.float32))
    a, b = E.DetectionEvaluator(), E.DetectionEvaluator()
    a.update([out], [tgt])
    b.update([pasted], [tgt])
    sa, sb = a.summarize(verbose=False), b.summarize(verbose=False)
    assert sa == sb and any(v not in (-1.0, 0.0) for v in sa["segm"])
    via_masks = E.coco_results([pasted], [42], [(h, w)], label_to_category=[0, 101, 102])     # pasted masks go through encode
    assert via_masks == res
