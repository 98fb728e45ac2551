"""CPU: the host logic of the device-side input path -- the tables ``ops.stage_u8_batch`` and ``ops.resized_mask_layout`` build
(worked out by hand below), the refusals that must come before any launch, and ``PreparedImages`` at the transform."""
import numpy as np
import pytest
import torch

from seam_match_rcnn_amd import _native, ops
from seam_match_rcnn_amd.input_pipeline import prepare_batch                      # the feature: absent, this file fails at import
from seam_match_rcnn_amd.models import detection as det
from seam_match_rcnn_amd.models.detection import GeneralizedRCNNTransform


def test_batch_tables_by_hand():
    imgs = [torch.zeros((5, 7, 3), dtype=torch.uint8), torch.zeros((4, 3, 3), dtype=torch.uint8)]
    tables, n = ops.stage_u8_batch(imgs, [(10, 14), (8, 6)], 32, 32, [True, False], None)
    assert n == 2 and tables.dtype == torch.uint8 and tables.numel() == 64          # 28 bytes per image, rounded up to 32s
    raw = tables.numpy()
    assert raw[:16].view(np.int64).tolist() == [64, 64 + 5 * 7 * 3]                 # the images follow the tables: 64, 169 (odd)
    assert raw[16:56].view(np.int32).reshape(2, 5).tolist() == [[5, 7, 10, 14, 1], [4, 3, 8, 6, 0]]
    assert not raw[56:].any()
    with pytest.raises(ValueError):
        ops.stage_u8_batch(imgs, [(33, 14), (8, 6)], 32, 32, [False, False], None)  # taller than the padded frame
    with pytest.raises(ValueError):
        ops.stage_u8_batch(imgs, [(10, 0), (8, 6)], 32, 32, [False, False], None)


def test_resized_mask_layout_by_hand():
    lay = ops.mask_layout([2, 0, 1], [(3, 5), (4, 4), (2, 7)])
    out_lay, obj_out = ops.resized_mask_layout(lay, [(6, 9), (8, 8), (1, 3)], [True, False, True])
    assert obj_out.dtype == np.int32 and obj_out.tolist() == [[6, 9, 1], [6, 9, 1], [1, 3, 1]]
    assert out_lay.obj_off.tolist() == [0, 54, 108] and out_lay.img_off == [0, 108, 108, 111] and out_lay.total == 111
    assert lay.obj_off.tolist() == [0, 15, 30]                                     # the source layout is left as it was
    _, none = ops.resized_mask_layout(lay, [(6, 9), (8, 8), (1, 3)])
    assert none[:, 2].tolist() == [0, 0, 0]
    with pytest.raises(ValueError):
        ops.resized_mask_layout(lay, [(6, 9), (8, 8)], [True, False, True])
    with pytest.raises(ValueError):
        ops.resized_mask_layout(lay, [(6, 9), (8, 8), (1, 3)], [True])
    _, t = ops.pack_rle_masks([[[15], None], [], [[0, 14]]], [(3, 5), (4, 4), (2, 7)])
    assert t["sel"].tolist() == [0, 2]                                             # the objects the RLE tables carry
    r = ops._resized_tables(t, out_lay, obj_out)
    assert r["obj_out"].tolist() == [[6, 9, 1], [1, 3, 1]] and r["obj_out_off"].tolist() == [0, 108]
    assert t["obj_out_off"].tolist() == [0, 30]


def test_no_device_no_launch(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    img = torch.zeros((8, 9, 3), dtype=torch.uint8)
    with pytest.raises(_native.SeamNativeError):
        ops.preprocess_u8_batch([img], [(8, 9)], 32, 32)
    with pytest.raises(_native.SeamNativeError):
        ops.preprocess_u8_batch([img.numpy()], [(8, 9)], 32, 32)
    off, dims = torch.zeros(1, dtype=torch.int64), torch.tensor([[8, 9, 8, 9, 0]], dtype=torch.int32)
    with pytest.raises(_native.SeamNativeError):
        ops.preprocess_u8_flat(img.reshape(-1), off, dims, 32, 32, False)

    class Model:
        transform = GeneralizedRCNNTransform(64, 96)
    with pytest.raises(_native.SeamNativeError):
        prepare_batch([img], [{"boxes": torch.zeros((0, 4))}], "cpu", Model())
    with pytest.raises(ValueError, match="uint8"):
        prepare_batch([img.float()], [{}], "cpu", Model())
    with pytest.raises(ValueError, match="one target"):
        prepare_batch([img], [], "cpu", Model())


def test_prepared_images_at_the_transform():
    tr = det.GeneralizedRCNNTransform(64, 96)
    s2d = tr.prepared_s2d()
    assert s2d == det.STEM_S2D
    x = torch.zeros((2, 32, 48, 12) if s2d else (2, 64, 96, 4))
    p = det.PreparedImages(x, [(64, 91), (64, 65)], [(37, 53), (50, 51)], (64, 96), 64, 96, 32, s2d)
    assert len(p) == 2 and det.image_list(p) is p
    got = tr(p)
    assert got[0] is x and got[1] == [(64, 91), (64, 65)] and got[2] == [(37, 53), (50, 51)] and got[3] == (64, 96)
    for other in (det.GeneralizedRCNNTransform(72, 96), det.GeneralizedRCNNTransform(64, 128), det.GeneralizedRCNNTransform(64, 96, 64)):
        with pytest.raises(ValueError, match="min_size"):
            other(p)
    with pytest.raises(ValueError, match="layout"):
        tr(det.PreparedImages(x, p.sizes, p.orig, p.padded, 64, 96, 32, not s2d))
    tr.compute_dtype = torch.float16
    with pytest.raises(ValueError, match="layout"):
        tr(p)
    a = torch.zeros(3, 4, 5, requires_grad=True)
    listed = det.image_list((a,))
    assert isinstance(listed, list) and not listed[0].requires_grad and listed[0].data_ptr() == a.data_ptr()
