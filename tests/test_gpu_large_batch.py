"""The bench's step batches at full size: tensors past 2^31 and 2^32 bytes.

A timed config-2 step sends 8 clips x 10 frames of 800^2 through ONE ``forward_fixed_rois`` call (fp32), and a config-5 step
8 clips x 30 frames of 1080p (fp16).  The stem, layer1 and P2 activations of those batches are 3.3 GB and 7.9 GB: the kernels
reach frames past byte 2^31 (and 2^32, 3 * 2^31) only by rebasing their buffer descriptors per image group.  The frames whose
activation straddles a multiple of 2^31 bytes are computed from the shapes, and each of them -- with the first and the last
frame -- must give the same bits as the frame run alone: every FPN level, the RPN head's outputs and ``roi_features``.  The
last frame of the fp32 batch is also checked against the CPU oracle at test_gpu_config1's tolerance.
"""
import pytest
import torch

import seam_match_rcnn_amd.synth as synth
from conftest import to_torch
from oracle import detection as OD
from test_gpu_ops import assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TWO31 = 1 << 31


@pytest.fixture(scope="module")
def model_and_state():
    # as bench.build_model
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    sd = to_torch(synth.video_matchrcnn_state(5))
    m = videomatchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    m.load_state_dict(sd)
    return m.to(DEV).eval(), sd


def frames_to_check(n_frames, per_frame):
    """The first and last frame, and every frame whose [f * per_frame, (f + 1) * per_frame) byte range holds a multiple of 2^31."""
    out = {0, n_frames - 1}
    j = 1
    while j * TWO31 < n_frames * per_frame:
        f = (j * TWO31) // per_frame
        if f * per_frame < j * TWO31:       # straddles (a frame starting exactly on the boundary is that boundary's frame too)
            out.add(f)
        else:
            out.update({f - 1, f})
        j += 1
    return sorted(out)


def per_frame_bytes(feats, hp, wp, es):
    """The largest per-frame activation of the body: the stem output [hp/2, wp/2, 64], layer1 / P2 [hp/4, wp/4, 256]."""
    p2 = feats["0"][0].numel() * es
    stem = (hp // 2) * (wp // 2) * 64 * es
    return max(p2, stem)


def flat_rpn(rpn, f):
    """the RPN head's outputs of frame f: (objectness, deltas) of every level, in order"""
    return [t[f] for pair in rpn for t in pair]


def check_batch(m, frames, rois, dtype, label):
    """Run the whole batch once, then each chosen frame alone; returns (chosen frames with byte offsets, batch results)."""
    n = len(frames)
    with torch.no_grad():
        res, feats, rpn = m.forward_fixed_rois(frames, [rois] * n, run_rpn_head=True)
    torch.cuda.synchronize()
    es = feats["0"].element_size()
    hp, wp = feats["0"].shape[1] * 4, feats["0"].shape[2] * 4
    per = per_frame_bytes(feats, hp, wp, es)
    assert n * per > TWO31, f"{label}: the batch does not reach 2^31 bytes ({n} x {per})"
    chosen = frames_to_check(n, per)
    kept = {f: ({k: v[f].clone() for k, v in feats.items()}, [t.clone() for t in flat_rpn(rpn, f)], res[f]["roi_features"].clone())
            for f in chosen}
    last_rf = res[-1]["roi_features"].clone()
    del res, feats, rpn
    torch.cuda.empty_cache()
    offsets = [(f, f * per) for f in chosen]
    print(f"{label}: {n} frames x {per} B per frame = {n * per} B; frames checked (frame, first byte): {offsets}")
    for f in chosen:
        with torch.no_grad():
            r1, f1, rpn1 = m.forward_fixed_rois(frames[f:f + 1], [rois], run_rpn_head=True)
        torch.cuda.synchronize()
        fb, rb, rfb = kept[f]
        for k in fb:
            assert torch.equal(fb[k], f1[k][0]), f"{label}: frame {f} (byte {f * per}) FPN level {k} differs from the frame alone"
        for i, (a, b) in enumerate(zip(rb, flat_rpn(rpn1, 0))):
            assert torch.equal(a, b), f"{label}: frame {f} (byte {f * per}) RPN output {i} differs from the frame alone"
        assert torch.equal(rfb, r1[0]["roi_features"]), f"{label}: frame {f} (byte {f * per}) roi_features differ from the frame alone"
    return offsets, last_rf


def test_config2_fp32_batch_past_2gib(model_and_state):
    m, sd = model_and_state
    torch.cuda.reset_peak_memory_stats()
    # 8 clips x 10 frames of 800^2, the bench's fixed ROIs (32 per frame in the resized frame)
    from seam_match_rcnn_amd.models.detection import resized_size
    frames = torch.cat([torch.from_numpy(synth.frames(c, 10, 800, 800)) for c in range(8)]).to(DEV)
    rh, rw, _ = resized_size(800, 800)
    rois = torch.from_numpy(synth.fixed_rois(32, rh, rw)).to(DEV)
    flist = list(frames.unbind(0))
    offsets, last_rf = check_batch(m, flist, rois, torch.float32, "config-2 fp32")
    assert [f for f, _ in offsets] == [0, 52, 79]
    # the last frame against the CPU oracle (test_gpu_config1's tolerance)
    img = frames[-1].cpu()
    batch, sizes = OD.transform([img], 800, 1333)
    ofe = OD.fpn(OD.resnet50_body(batch, sd), sd)
    orf = OD.multiscale_roi_align([ofe[k] for k in "0123"], [rois.cpu()], sizes, 14)
    assert_close(last_rf, orf)
    print(f"config-2 fp32: peak allocated {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
    del frames, flist, last_rf
    torch.cuda.empty_cache()


def test_config5_fp16_batch_past_4gib(model_and_state):
    m, _ = model_and_state
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    from seam_match_rcnn_amd.models.detection import resized_size
    rh, rw, _ = resized_size(1080, 1920)
    rois = torch.from_numpy(synth.fixed_rois(64, rh, rw)).to(DEV)
    # 8 clips x 30 frames of 1080p, made clip by clip on the host and kept on the device
    frames = torch.cat([torch.from_numpy(synth.frames(500 + c, 30, 1080, 1920)).to(DEV) for c in range(8)])
    flist = list(frames.unbind(0))
    try:
        m.set_compute_dtype(torch.float16)            # as test_gpu_config5
        offsets, _ = check_batch(m, flist, rois, torch.float16, "config-5 fp16")
    finally:
        m.set_compute_dtype(torch.float32)
    assert [f for f, _ in offsets] == [0, 65, 130, 195, 239]
    print(f"config-5 fp16: peak allocated {torch.cuda.max_memory_allocated() / 1e9:.1f} GB")
    del frames, flist
    torch.cuda.empty_cache()
