"""GPU: the one-launch frame path of a MovingFashion batch -- ``ops.frames_prepare_batch`` / ``ops.frames_prepare_flat``
(``seam_frames_prepare_batch_u8``, csrc/seam_frames.hip), ``input_pipeline.prepare_batch`` on a lazy
``datasets.MFDataset.MovingFashionDataset`` batch, ``frames.prepare_frames`` and ``evaluator.collect_descriptors`` over its loader.

The kernel makes a 64 x 64 tile of the half-size image per block, so the frame sizes are: 2 x 2 (the smallest), 3 x 2, 9 x 7 and
101 x 75 (odd: the scale is not 2 and every column has its own weights), 64 x 96 and 270 x 480 (smaller than a tile, several
tiles with a partial last one), 128 x 128 (exactly one tile), 130 x 128 and 128 x 131 (one tile + 1 in either axis), one 1080 x 1920
frame, the 100 x 100 zero placeholder, and two images of modes 0 and 1.  Everything is compared byte for byte: with the per-frame
route (``ops.frame_noise`` + ``ops.resize_bicubic_u8``, one reference per module) for the generator's draws, with
``oracle.frames`` for given draws."""
import random

import numpy as np
import pytest
import torch

import mf_fixture as MF
from oracle import frames as OF
from seam_match_rcnn_amd import _native, frames, ops
from seam_match_rcnn_amd.datasets.MFDataset import MovingFashionDataset, get_dataloader      # the feature: absent, no import
from seam_match_rcnn_amd.input_pipeline import prepare_batch, prepare_images
from seam_match_rcnn_amd.models import detection as det

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
# (h, w, mode)
CASES = [(2, 2, 2), (3, 2, 2), (33, 47, 0), (9, 7, 2), (101, 75, 2), (45, 31, 1), (64, 96, 2), (270, 480, 2), (128, 128, 2),
         (130, 128, 2), (128, 131, 2), (1080, 1920, 2), (100, 100, 0)]
MODES = [c[2] for c in CASES]
SIGMAS = [0.05 if k % 2 else 0.25 for k in range(len(CASES))]
SEEDS = [2 ** 63 + 17 if k == 4 else 1000 + 7919 * k for k in range(len(CASES))]


def images_of(cases=CASES, seed=0):
    rng = np.random.RandomState(seed)
    return [torch.zeros(h, w, 3, dtype=torch.uint8) if (h, w, m) == (100, 100, 0)
            else torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)) for h, w, m in cases]


def per_frame(img, mode, sigma, seed):
    """The route of the per-frame entry points: two launches for the noise and the flip, four for the resize."""
    img = img.to(DEV)
    if mode == 0:
        return img.clone()
    if mode == 1:
        return ops.frame_noise(img, 0.0)
    return ops.resize_bicubic_u8(ops.frame_noise(img, sigma, None, seed), img.shape[0] // 2, img.shape[1] // 2)


@pytest.fixture(scope="module")
def batch():
    imgs = images_of()
    want = [per_frame(i, m, s, sd).cpu() for i, m, s, sd in zip(imgs, MODES, SIGMAS, SEEDS)]
    return imgs, want


# ---- 1. bit identity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("host", [True, False])
def test_equals_the_per_frame_route(batch, host):
    imgs, want = batch
    src = imgs if host else [i.to(DEV) for i in imgs]
    keep = [i.clone() for i in src]
    got = ops.frames_prepare_batch(src, MODES, SIGMAS, SEEDS, device=DEV)
    assert len(got) == len(CASES) and len({g.untyped_storage().data_ptr() for g in got}) == 1            # views of one buffer
    for k, ((h, w, m), g, ref) in enumerate(zip(CASES, got, want)):
        assert g.dtype == torch.uint8 and g.is_cuda and tuple(g.shape) == ops.frame_out_size(h, w, m) + (3,), k
        assert torch.equal(g.cpu(), ref), (k, h, w, m)
    assert torch.equal(got[2].cpu(), imgs[2]) and torch.equal(got[5].cpu(), imgs[5].flip(-1)) and not got[12].any()
    assert all(torch.equal(a, b) for a, b in zip(src, keep))                                             # the caller's tensors are not written
    again = ops.frames_prepare_batch(src, MODES, SIGMAS, SEEDS, device=DEV)
    assert all(torch.equal(a, b) for a, b in zip(got, again))                                            # two calls, equal bytes
    other = ops.frames_prepare_batch(src[:2] + src[3:5], [2] * 4, SIGMAS[:4], [5, 6, 7, 8], device=DEV)
    assert not torch.equal(other[3], got[4])                                                             # the seed matters
    quiet = ops.frames_prepare_batch([src[4]], [2], [0.0], [3], device=DEV)[0]                           # sigma 0: flip + resize alone
    assert torch.equal(quiet, ops.resize_bicubic_u8(ops.frame_noise(imgs[4].to(DEV), 0.0), 50, 37))


def test_prepare_clip_keeps_its_results(batch):
    imgs, _ = batch
    clip = [imgs[k].to(DEV) for k in (4, 6, 9)]
    sig = [0.25, 0.05, 0.25]
    got = frames.prepare_clip(clip, True, sig, seed=3)
    want = [frames.prepare_frame(f, True, s, 3 + 7919 * i) for i, (f, s) in enumerate(zip(clip, sig))]
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    plain = frames.prepare_clip(clip, noise=False)
    assert all(torch.equal(a, ops.frame_noise(f, 0.0)) for a, f in zip(plain, clip))
    assert frames.prepare_clip([]) == []


# ---- 2. given draws ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("host", [True, False])
def test_given_draws_equal_the_oracle(host):
    cases = [(3, 2, 2), (45, 31, 1), (9, 7, 2), (101, 75, 2)]
    imgs = images_of(cases, 1)
    rng = np.random.RandomState(2)
    draws = [rng.randn(h, w, 3) if m == 2 else None for h, w, m in cases]
    sig = [0.25, 0.05, 0.05, 0.25]
    src = imgs if host else [i.to(DEV) for i in imgs]
    got = ops.frames_prepare_batch(src, [c[2] for c in cases], sig, [0] * 4, device=DEV,
                                   noise_values=[None if d is None else torch.from_numpy(d) for d in draws])
    for img, d, s, g in zip(imgs, draws, sig, got):
        np.testing.assert_array_equal(g.cpu().numpy(), OF.prepare_frame(img.numpy(), d, s))
    with pytest.raises(ValueError):
        ops.frames_prepare_batch(src, [c[2] for c in cases], sig, [0] * 4, device=DEV, noise_values=[None] * 4)


# ---- 3. the flat launch: guards, entries that do not fit -------------------------------------------------------------------------------

FLAT = [(9, 7, 2), (33, 47, 0), (130, 128, 2), (45, 31, 1), (3, 2, 2)]
FLAT_SIGMAS = [0.25, 0.0, 0.05, 0.0, 0.25]
FLAT_SEEDS = [21, 22, 23, 24, 25]
GUARD = 64


def flat_batch():
    """Input and output buffers laid out by hand: an odd gap between the images, 0xA5 guards in front of, between and behind
    the outputs -> (input bytes, in_off, dims, output bytes, out_off, output sizes)."""
    imgs = images_of(FLAT, 3)
    in_off, out_off, pos_i, pos_o = [], [], 5, GUARD
    for img, (h, w, m) in zip(imgs, FLAT):
        oh, ow = ops.frame_out_size(h, w, m)
        in_off.append(pos_i)
        out_off.append(pos_o)
        pos_i += img.numel() + 3
        pos_o += oh * ow * 3 + 7
    src = np.full(pos_i, 0x3C, np.uint8)
    for img, o in zip(imgs, in_off):
        src[o:o + img.numel()] = img.numpy().reshape(-1)
    dst = np.full(pos_o + GUARD, 0xA5, np.uint8)
    return imgs, src, np.asarray(in_off, np.int64), np.asarray(FLAT, np.int32), dst, np.asarray(out_off, np.int64)


def run_flat(src, in_off, dims, dst, out_off, max_hw=(130, 128)):
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    flat, out = d(src), d(dst)
    ops.frames_prepare_flat(flat, d(in_off), d(dims), d(np.asarray(FLAT_SIGMAS)), d(np.asarray(FLAT_SEEDS, np.int64)), out, d(out_off),
                            *max_hw)
    torch.cuda.synchronize()
    return flat.cpu().numpy(), out.cpu().numpy()


def test_nothing_outside_the_outputs_is_written():
    imgs, src, in_off, dims, dst, out_off = flat_batch()
    src_after, out = run_flat(src, in_off, dims, dst, out_off)
    np.testing.assert_array_equal(src_after, src)                                          # the input buffer is read only
    inside = np.zeros(dst.size, bool)
    for img, (h, w, m), s, sd, o in zip(imgs, FLAT, FLAT_SIGMAS, FLAT_SEEDS, out_off):
        want = per_frame(img, m, s, sd).cpu().numpy().reshape(-1)
        inside[o:o + want.size] = True
        np.testing.assert_array_equal(out[o:o + want.size], want)
    assert (out[~inside] == 0xA5).all() and (~inside[:GUARD]).all() and (~inside[-GUARD:]).all()


def test_an_entry_that_does_not_fit_is_left_alone():
    """The kernel's own bounds (no fault is provoked: an entry is refused before any access).  One launch per kind of bad entry,
    always image 2 (several tiles) or 0; the other images must still be right and the refused one's output bytes untouched."""
    imgs, src, in_off, dims, dst, out_off = flat_batch()
    want = [per_frame(img, m, s, sd).cpu().numpy().reshape(-1) for img, (h, w, m), s, sd in zip(imgs, FLAT, FLAT_SIGMAS, FLAT_SEEDS)]

    def check(bad, **tables):
        t = dict(in_off=in_off.copy(), dims=dims.copy(), out_off=out_off.copy())
        for k, (row, value) in tables.items():
            t[k][row] = value
        src_after, out = run_flat(src, t["in_off"], t["dims"], dst, t["out_off"])
        np.testing.assert_array_equal(src_after, src)
        for k, (w, o) in enumerate(zip(want, out_off)):
            if k == bad:
                assert (out[o:o + w.size] == 0xA5).all(), k
            else:
                np.testing.assert_array_equal(out[o:o + w.size], w)
        assert (out[:GUARD] == 0xA5).all() and (out[-GUARD:] == 0xA5).all()

    check(2, in_off=(2, src.size - 10))                       # the input ends behind the buffer
    check(2, in_off=(2, -8))
    check(2, out_off=(2, dst.size - 100))                     # the output ends behind the buffer
    check(0, out_off=(0, -1))
    check(2, dims=(2, (2 ** 31 - 1, 2 ** 31 - 1, 2)))         # a size far beyond both buffers
    check(2, dims=(2, (130, 128, 3)))                         # no such mode
    check(2, dims=(2, (131, 128, 2)))                         # higher than the launch was sized for
    check(4, dims=(4, (1, 6, 2)))                             # a frame that cannot be halved
    lib = _native.lib()
    p = torch.zeros(64, dtype=torch.uint8, device=DEV).data_ptr()
    call = lambda n, a=p, mh=8: lib.seam_frames_prepare_batch_u8(a, 64, p, p, p, p, None, None, 0, p, 64, p, n, mh, 8, None)
    bad = call(0)
    assert bad != 0 and call(65536) == bad and call(1, None) == bad and call(1, p, 0) == bad
    assert lib.seam_frames_prepare_batch_u8(p, 64, p, p, p, p, p, None, 8, p, 64, p, 1, 8, 8, None) == bad      # draws without offsets


# ---- 4. prepare_batch on a lazy batch of the dataset ---------------------------------------------------------------------------------

class StubModel:
    def __init__(self):
        self.transform = det.GeneralizedRCNNTransform(64, 96)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("mf"))
    return MF.write(root), root


def lazy_batch(tree, noise=True):
    from seam_match_rcnn_amd import transform as T
    ds = MovingFashionDataset(tree[0], root=tree[1], lazy=True, noise=noise, transform=T.RandomHorizontalFlip(0.5))
    random.seed(4)
    np.random.seed(4)
    entries = [(0, "in", None), (0, "video", 0.3, 0), (0, "video", 0.8, 1), (1, "in", None), (1, "video", 0.5, 1), (1, "video", 1.0, 1),
               (2, "video", 0.2, 1)]
    images, targets = zip(*[ds[x] for x in entries])
    return list(images), list(targets)


@pytest.mark.parametrize("s2d", [False, True])
@pytest.mark.parametrize("noise", [True, False])
def test_prepare_batch_on_a_lazy_batch(tree, s2d, noise, monkeypatch):
    monkeypatch.setattr(det, "STEM_S2D", s2d)
    m = StubModel()
    images, targets = lazy_batch(tree, noise)
    flips = [bool(t.get("hflip", False)) for t in targets]
    assert any(flips) and not all(flips) and [t["frame_prep"] for t in targets] == [0, 2 if noise else 1, 2 if noise else 1, 0, 2 if noise else 1, 0, 2 if noise else 1]
    assert targets[5]["valid"] is False                                                    # the zero placeholder is in the batch
    ready = [per_frame(i, t["frame_prep"], t["frame_sigma"], t.get("frame_seed", 0)) for i, t in zip(images, targets)]
    halved = [tuple(r.shape[:2]) for r in ready]
    want = prepare_images(ready, DEV, m, flips)
    prepared, pt = prepare_batch(images, targets, DEV, m, masks="none")
    assert prepared.orig == halved == [tuple(int(v) for v in t["boxes"][0, 2:].tolist()[::-1]) for t in targets]
    assert prepared.sizes == want.sizes and prepared.padded == want.padded and prepared.s2d == s2d
    assert torch.equal(prepared.tensor, want.tensor)
    for t, src in zip(pt, targets):
        assert not {"frame_prep", "frame_sigma", "frame_seed", "hflip"} & set(t) and t["boxes"].is_cuda and t["tag"] == src["tag"]
    assert all("frame_prep" in t for t in targets)                                         # the caller's targets are left as they were
    again, _ = prepare_batch([i.to(DEV) for i in images], targets, DEV, m, masks="none")  # device inputs, and determinism
    assert torch.equal(again.tensor, want.tensor)
    out_i, out_t = frames.prepare_frames(images, targets, DEV)
    assert all(torch.equal(a, b) for a, b in zip(out_i, ready)) and not any("frame_prep" in t or "frame_seed" in t for t in out_t)
    assert [t.get("hflip", False) for t in out_t] == flips
    with pytest.raises(ValueError):
        prepare_batch(images, [dict(t, noise_sigma=0.1) if k == 0 else t for k, t in enumerate(targets)], DEV, m, masks="none")


# ---- 5. the evaluator through the loader ----------------------------------------------------------------------------------------------

BIG = {"p0": ((128, 160), [(256, 320), (257, 321)], 1, True), "p1": ((128, 160), [(256, 320), (256, 320)], 0, True)}


def test_collect_descriptors_over_a_lazy_loader(tmp_path):
    import seam_match_rcnn_amd.synth as synth
    from conftest import to_torch
    from seam_match_rcnn_amd import evaluator as EV
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    ann = MF.write(str(tmp_path), BIG)
    model = videomatchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    model.load_state_dict(to_torch(synth.video_matchrcnn_state(5)))
    model = model.to(DEV).eval()
    model.transform.min_size, model.transform.max_size = 128, 160
    ds = MovingFashionDataset(ann, root=str(tmp_path), lazy=True)
    loader = get_dataloader(ds, 4, False, is_seq=True, num_workers=0, fixed_frame=[0.1, 0.5, 0.9], fixed_video_i=1)
    random.seed(8)
    np.random.seed(8)
    batches = [(list(i), list(t)) for i, t in loader]
    assert len(batches) == 2 and all([t["frame_prep"] for t in ts] == [0, 2, 2, 2] for _, ts in batches)
    by_hand = [([per_frame(i, t["frame_prep"], t["frame_sigma"], t.get("frame_seed", 0)) for i, t in zip(im, ts)],
                [{k: v for k, v in t.items() if k not in frames.FRAME_KEYS} for t in ts]) for im, ts in batches]
    got = EV.collect_descriptors(model, batches, DEV, score_threshold=0.0)
    want = EV.collect_descriptors(model, by_hand, DEV, score_threshold=0.0)
    assert got.count_street == 2 and got.shop_mat.shape == (2, 256) and list(got.product_keys) == [0, 1]
    assert got.tracklets_gt.shape == (6, 4) and got.tracklets_gt[0].tolist() == [1.0, 0.0, 11.0, 12.0]
    for name, a in vars(got).items():
        b = getattr(want, name)
        if isinstance(a, torch.Tensor):
            assert torch.equal(a, b), name
        elif isinstance(a, np.ndarray):
            np.testing.assert_array_equal(a, b, err_msg=name)
        else:
            assert a == b or list(a) == list(b), name
    assert all("frame_prep" in t for _, ts in batches for t in ts)
