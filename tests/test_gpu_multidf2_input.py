"""GPU: the device-side noise of a Multi-DeepFashion2 batch -- ``ops.noise_u8_batch`` (``seam_noise_u8_batch``, csrc/seam_frames.hip),
``ops.preprocess_u8_batch(noise=...)``, ``input_pipeline.prepare_batch`` / ``apply_noise`` and ``evaluator_df2.evaluate`` over
``datasets.MultiDF2Dataset.get_dataloader``.

Images are RandomState bytes of sizes (37, 53), (48, 40), (1, 1) and (2, 129): odd byte offsets, rows that are no dword multiple, the
smallest image.  With given draws the kernel must equal the NumPy arithmetic (``oracle.frames.noise_flip``) bit for bit; with its own
draws it must equal ``ops.frame_noise`` bit for bit (one generator) and a NumPy restatement of the generator up to the last-place
freedom of ``log`` and ``cos``: no byte off by more than one level, at most 1 byte in 10^4 different (perturbing the draws by
+-8 ulp flips 0 of 213,030 bytes at these sizes and sigmas on the CPU)."""
import random

import numpy as np
import pytest
import torch

import df2_fixture as FX
from conftest import to_torch
from oracle import frames as OF
from seam_match_rcnn_amd import _native, ops
from seam_match_rcnn_amd.datasets.MultiDF2Dataset import MultiDeepFashion2Dataset, get_dataloader     # the feature: absent, no import
from seam_match_rcnn_amd.input_pipeline import apply_noise, prepare_batch
from seam_match_rcnn_amd.models import detection as det
from seam_match_rcnn_amd.transform import ToTensor

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SHAPES = [(37, 53), (48, 40), (1, 1), (2, 129)]
SIGMAS = [0.1, 0.0, 0.25, 0.1]
SEEDS = [11, 12, 2 ** 63 + 13, 14]
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def images_of(seed=0):
    rng = np.random.RandomState(seed)
    return [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in SHAPES]


def draws_of(seed=1):
    rng = np.random.RandomState(seed)
    return [rng.randn(h, w, 3) for h, w in SHAPES]


def to_tensor(img):
    """torchvision's ``to_tensor`` on the host (bytes / 255, correctly rounded), as the eager route runs it."""
    return img.cpu().permute(2, 0, 1).float().div(255).contiguous()


# ---- 1. given draws ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("host", [True, False])
def test_given_draws_equal_numpy(host):
    imgs, draws = images_of(), draws_of()
    src = imgs if host else [i.to(DEV) for i in imgs]
    keep = [i.clone() for i in src]
    got = ops.noise_u8_batch(src, SIGMAS, SEEDS, noise_values=[torch.from_numpy(d) for d in draws], device=DEV)
    assert len(got) == 4 and len({g.untyped_storage().data_ptr() for g in got}) == 1          # views of one buffer
    for img, d, s, g in zip(imgs, draws, SIGMAS, got):
        assert g.dtype == torch.uint8 and g.is_cuda and g.shape == img.shape
        want = OF.noise_flip(img.numpy()[..., ::-1], d, s)
        np.testing.assert_array_equal(g.cpu().numpy(), want)
    assert torch.equal(got[1].cpu(), imgs[1])                                                  # sigma 0: the input
    assert not torch.equal(got[0].cpu(), imgs[0]) and not torch.equal(got[3].cpu(), imgs[3])
    assert all(torch.equal(a, b) for a, b in zip(src, keep))                                   # the caller's tensors are not written
    with pytest.raises(ValueError):
        ops.noise_u8_batch(imgs, SIGMAS, SEEDS, noise_values=[torch.from_numpy(d) for d in draws[:3]], device=DEV)
    with pytest.raises(ValueError):
        ops.noise_u8_batch(imgs, SIGMAS, SEEDS, noise_values=[torch.from_numpy(d).float() for d in draws], device=DEV)
    with pytest.raises(ValueError):
        ops.noise_u8_batch(imgs, SIGMAS[:3], SEEDS, device=DEV)


def staged(imgs, draws, guard=16):
    """A flat buffer as the launch takes it, built by hand with 0xA5 guard bytes in front of the first image and behind the last:
    (host uint8 array, offsets, dims, where the sigma / seed tables start, the draws' element offsets)."""
    n = len(imgs)
    head = 32 * ((28 * n + 31) // 32)
    nbytes = [i.numel() for i in imgs]
    off = np.cumsum([head + guard] + nbytes)[:-1]
    end = int(off[-1] + nbytes[-1])
    at = (end + guard + 7) // 8 * 8
    buf = np.full(at + 16 * n, 0xA5, np.uint8)
    dims = np.asarray([(i.shape[0], i.shape[1], i.shape[0], i.shape[1], 0) for i in imgs], np.int32)
    buf[:8 * n] = off.astype(np.int64).view(np.uint8)
    buf[8 * n:28 * n] = dims.reshape(-1).view(np.uint8)
    for i, o, b in zip(imgs, off, nbytes):
        buf[o:o + b] = i.numpy().reshape(-1)
    buf[at:at + 8 * n] = np.asarray(SIGMAS, np.float64).view(np.uint8)
    buf[at + 8 * n:] = np.asarray(SEEDS, np.uint64).view(np.uint8)
    d_off = np.cumsum([0] + [d.size for d in draws])[:-1].astype(np.int64)
    return buf, off, nbytes, at, d_off


def launch(flat, n, at, draws, d_off, off_table=None, dims_table=None, nbytes=None):
    lib = _native.lib()
    off_ptr = flat.data_ptr() if off_table is None else off_table.data_ptr()
    dims_ptr = flat.data_ptr() + 8 * n if dims_table is None else dims_table.data_ptr()
    rc = lib.seam_noise_u8_batch(flat.data_ptr(), flat.numel() if nbytes is None else nbytes, off_ptr, dims_ptr, flat.data_ptr() + at,
                                 flat.data_ptr() + at + 8 * n, None if draws is None else draws.data_ptr(),
                                 None if d_off is None else d_off.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return int(rc)


def test_nothing_outside_the_images_is_written():
    imgs, draws = images_of(2), draws_of(3)
    buf, off, nbytes, at, d_off = staged(imgs, draws)
    flat = torch.from_numpy(buf).to(DEV)
    dd = torch.from_numpy(np.concatenate([d.reshape(-1) for d in draws])).to(DEV)
    assert launch(flat, 4, at, dd, torch.from_numpy(d_off).to(DEV)) == 0
    out = flat.cpu().numpy()
    inside = np.zeros(buf.size, bool)
    for img, d, s, o, b in zip(imgs, draws, SIGMAS, off, nbytes):
        inside[o:o + b] = True
        np.testing.assert_array_equal(out[o:o + b], OF.noise_flip(img.numpy()[..., ::-1], d, s).reshape(-1))
    np.testing.assert_array_equal(out[~inside], buf[~inside])               # tables, both guards, padding, sigma and seed tables
    assert (out[off[0] - 16:off[0]] == 0xA5).all() and (out[off[-1] + nbytes[-1]:off[-1] + nbytes[-1] + 16] == 0xA5).all()
    assert (out[inside] != buf[inside]).any()


def test_an_entry_that_does_not_fit_is_left_alone():
    """The kernel's own bound (no fault is provoked: the entry is refused before any access): offsets past the buffer, a negative
    offset, sizes whose byte count overflows 63 bits, and a byte count smaller than the image leave every byte as it was."""
    imgs, draws = images_of(4), draws_of(5)
    sigmas_all = SIGMAS[:1] + [0.2] + SIGMAS[2:]
    buf, off, nbytes, at, _ = staged(imgs, draws)
    buf[at:at + 32] = np.asarray(sigmas_all, np.float64).view(np.uint8)     # every image noisy: each must be refused by its entry
    dims = buf[32:112].view(np.int32).reshape(4, 5).copy()
    bad_off = np.asarray([buf.size - nbytes[0] + 1, -8, buf.size, off[3]], np.int64)
    dims[3, :2] = (2 ** 31 - 1, 2 ** 31 - 1)
    flat = torch.from_numpy(buf).to(DEV)
    assert launch(flat, 4, at, None, None, torch.from_numpy(bad_off).to(DEV), torch.from_numpy(dims).to(DEV)) == 0
    np.testing.assert_array_equal(flat.cpu().numpy(), buf)
    assert launch(flat, 4, at, None, None, nbytes=int(off[0]) + 1) == 0     # a buffer that ends inside the first image
    np.testing.assert_array_equal(flat.cpu().numpy(), buf)
    bad = launch(flat, 0, at, None, None)
    assert bad != 0 and launch(flat, 65536, at, None, None) == bad
    np.testing.assert_array_equal(flat.cpu().numpy(), buf)


# ---- 2. device draws -----------------------------------------------------------------------------------------------------------

def splitmix64(x):
    x = (x + np.uint64(0x9E3779B97F4A7C15)) & M64
    x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M64
    x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M64
    return x ^ (x >> np.uint64(31))


def numpy_noise(img, sigma, seed):
    """The generator (counter-based Box-Muller on two splitmix64 hashes of (seed, element)) and the byte arithmetic, in NumPy."""
    with np.errstate(over="ignore"):
        i = np.arange(img.size, dtype=np.uint64)
        s = np.uint64(seed)
        r0 = splitmix64(s ^ (i * np.uint64(2) + np.uint64(1)))
        r1 = splitmix64(s ^ (i * np.uint64(2) + np.uint64(2)) ^ np.uint64(0xD1B54A32D192ED03))
    u0 = ((r0 >> np.uint64(11)).astype(np.float64) + 1.0) * (1.0 / 9007199254740993.0)
    u1 = (r1 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
    n = np.sqrt(-2.0 * np.log(u0)) * np.cos(6.283185307179586 * u1)
    x = img.reshape(-1) / 255.0
    x = x + n * sigma
    x = x * 255.0
    return np.asarray(np.clip(x, 0, 255.0), dtype=np.uint8).reshape(img.shape)


def test_device_draws_are_the_frame_noise_generator():
    imgs = images_of(6)
    got = ops.noise_u8_batch(imgs, SIGMAS, SEEDS, device=DEV)
    again = ops.noise_u8_batch([i.to(DEV) for i in imgs], SIGMAS, SEEDS)
    other = ops.noise_u8_batch(imgs, SIGMAS, [s + 1 for s in SEEDS], device=DEV)
    differ = total = 0
    for k, (img, s, seed, g) in enumerate(zip(imgs, SIGMAS, SEEDS, got)):
        one = ops.frame_noise(img.to(DEV).flip(-1).contiguous(), s, None, seed)
        assert torch.equal(g, one), k                                        # one generator in the project
        assert torch.equal(g, again[k])
        if s == 0.0:
            assert torch.equal(g.cpu(), img) and torch.equal(other[k], g)
            continue
        if img.numel() > 3:
            assert not torch.equal(g, other[k])
        want = numpy_noise(img.numpy(), s, seed).astype(np.int32)
        d = np.abs(g.cpu().numpy().astype(np.int32) - want)
        print(f"image {k} {tuple(img.shape)} sigma {s}: {int((d != 0).sum())} of {d.size} bytes differ from NumPy, max {int(d.max())}")
        assert d.max() <= 1
        differ += int((d != 0).sum())
        total += d.size
    assert differ * 10 ** 4 <= total


def test_device_draw_statistics():
    img = torch.full((256, 256, 3), 128, dtype=torch.uint8)
    (out,) = ops.noise_u8_batch([img], [0.1], [5], device=DEV)
    d = out.cpu().numpy().astype(np.float64) / 255.0 - 128 / 255.0
    print("mean", d.mean(), "std", d.std())
    assert abs(d.mean() + 0.5 / 255) < 1e-3          # truncation to uint8 biases by half a level; standard error 2.3e-4
    assert abs(d.std() - 0.1) < 1e-3                 # standard error 1.6e-4


# ---- 3. prepare_batch ------------------------------------------------------------------------------------------------------------

class StubModel:
    def __init__(self):
        self.transform = det.GeneralizedRCNNTransform(64, 96)


def lazy_targets(flips):
    out = []
    for (h, w), s, seed, f in zip(SHAPES, SIGMAS, SEEDS, flips):
        t = dict(boxes=torch.tensor([[0.0, 0.0, float(w), float(h)]]), labels=torch.tensor([1]), size=(h, w), noise_sigma=s,
                 i="1_101", tag=0)
        if h > 2:                                     # the two full-size images carry an object's polygon
            t["segmentation"] = [[[2.0, 2.0, w - 2.0, 2.0, w - 2.0, h - 2.0, 2.0, h - 2.0]]]
        if s > 0:
            t["noise_seed"] = seed
        if f:
            t["hflip"] = True
        out.append(t)
    return out


@pytest.mark.parametrize("s2d", [False, True])
def test_prepare_batch_with_noisy_targets(s2d, monkeypatch):
    monkeypatch.setattr(det, "STEM_S2D", s2d)
    m = StubModel()
    assert m.transform.prepared_s2d() == s2d
    imgs = images_of(7)
    flips = [True, False, False, True]
    targets = lazy_targets(flips)
    noisy = ops.noise_u8_batch(imgs, SIGMAS, [t.get("noise_seed", 0) for t in targets], device=DEV)
    floats = [(to_tensor(n).flip(-1).contiguous() if f else to_tensor(n)).to(DEV) for n, f in zip(noisy, flips)]
    with torch.no_grad():
        want, sizes, orig, padded = m.transform(floats)
    for masks in ("resized", "none"):
        prepared, pt = prepare_batch(imgs, targets, DEV, m, masks=masks)
        assert prepared.s2d == s2d and prepared.sizes == list(sizes) and prepared.padded == tuple(padded)
        assert torch.equal(prepared.tensor, want)
        for t, src, z in zip(pt, targets, sizes):
            assert not {"noise_sigma", "noise_seed", "segmentation", "size", "hflip"} & set(t)
            assert ("masks" in t) == (masks == "resized" and "segmentation" in src) and t["i"] == "1_101" and t["boxes"].is_cuda
            if "masks" in t:
                assert tuple(t["masks"].shape) == (1,) + tuple(z) and bool(t["masks"].any())
    assert all("noise_sigma" in t for t in targets)                           # the caller's targets are left as they were
    # without the keys: the bits of today's route (the launch is not made), which differ from the noisy batch
    bare = [{k: v for k, v in t.items() if k not in ("noise_sigma", "noise_seed")} for t in targets]
    plain, _ = prepare_batch(imgs, bare, DEV, m, masks="none")
    with torch.no_grad():
        want_plain = m.transform([(to_tensor(i).flip(-1).contiguous() if f else to_tensor(i)).to(DEV) for i, f in zip(imgs, flips)])[0]
    assert torch.equal(plain.tensor, want_plain) and not torch.equal(plain.tensor, want)
    quiet = [dict(t, noise_sigma=0.0) for t in bare]
    assert torch.equal(prepare_batch(imgs, quiet, DEV, m, masks="none")[0].tensor, want_plain)      # sigma 0: the identity
    out_i, out_t = apply_noise(imgs, targets, DEV)
    assert all(torch.equal(a, b) for a, b in zip(out_i, noisy)) and not any("noise_sigma" in t or "noise_seed" in t for t in out_t)
    assert [("segmentation" in t) for t in out_t] == [("segmentation" in t) for t in targets]


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------

def test_eval_forward_on_a_noisy_prepared_batch():
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd.models.matchrcnn import matchrcnn_resnet50_fpn, params
    m = matchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14, min_size=128, max_size=160, **params)
    sd = synth.detector_state(5, 14)
    sd.update(synth.match_predictor_state(6, "roi_heads.match_predictor."))
    m.load_state_dict(to_torch(sd), strict=False)
    m = m.to(DEV).eval()
    rng = np.random.RandomState(8)
    imgs = [torch.from_numpy(rng.randint(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in ((100, 125), (96, 120))]
    targets = [dict(boxes=torch.tensor([[10.0, 12.0, 90.0, 80.0]]), labels=torch.tensor([2]), noise_sigma=0.1, noise_seed=21, hflip=True),
               dict(boxes=torch.tensor([[20.0, 8.0, 100.0, 90.0]]), labels=torch.tensor([3]), noise_sigma=0.1, noise_seed=22)]
    noisy = ops.noise_u8_batch(imgs, [0.1, 0.1], [21, 22], device=DEV)
    floats = [to_tensor(noisy[0]).flip(-1).contiguous().to(DEV), to_tensor(noisy[1]).to(DEV)]
    with torch.no_grad():
        prepared, pt = prepare_batch(imgs, targets, DEV, m, masks="none")
        got = m(prepared, targets=pt)
        want = m(floats, targets=pt)
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))


# ---- 5. the evaluator through the loader ----------------------------------------------------------------------------------------

def test_evaluate_over_the_dataloader(tmp_path):
    import seam_match_rcnn_amd.synth as synth
    from seam_match_rcnn_amd import evaluator_df2 as EV
    from seam_match_rcnn_amd.models.video_matchrcnn import videomatchrcnn_resnet50_fpn
    ann_file, root = FX.write(tmp_path)
    model = videomatchrcnn_resnet50_fpn(pretrained_backbone=False, num_classes=14)
    model.load_state_dict(to_torch(synth.video_matchrcnn_state(5)))
    model = model.to(DEV).eval()
    model.transform.min_size, model.transform.max_size = 128, 160

    def run(ds):
        random.seed(3)
        np.random.seed(3)
        torch.manual_seed(3)
        return EV.evaluate(model, get_dataloader(ds, batch_size=3, is_parallel=False, n_products=1), DEV, verbose=False)

    eager = run(MultiDeepFashion2Dataset(ann_file, root, ToTensor(), noise=False))
    lazy = run(MultiDeepFashion2Dataset(ann_file, root, noise=False, lazy=True))
    print("eager", eager, "lazy", lazy)
    assert len(eager) == 3 and all(np.isfinite(eager)) and eager == lazy
    random.seed(3)
    np.random.seed(3)
    torch.manual_seed(3)
    noisy_ds = MultiDeepFashion2Dataset(ann_file, root, noise=True, lazy=True)
    ret, rep = EV.evaluate(model, get_dataloader(noisy_ds, batch_size=3, is_parallel=False, n_products=1), DEV, verbose=False,
                           return_report=True)
    assert len(ret) == 3 and all(np.isfinite(ret))
    t = rep.tables
    assert t.count_products == 2 and bool(torch.isfinite(t.shop_mat).all()) and bool(torch.isfinite(t.street_mat).all())
    assert all(np.isfinite(rep.accuracy(k)).all() for k in rep.counts)
