"""CPU: ``datasets.MFDataset`` -- the sampler against a restatement of the reference's and against the reference's own recorded
batches, the eager sample against ``oracle.frames`` with the same draws, the lazy contract, the frame readers, and the argument
errors of ``ops.frames_prepare_batch`` (which has no CPU path)."""
import builtins
import json
import os
import pickle
import random
import sys

import numpy as np
import pytest
import torch

import mf_fixture as MF
from conftest import ROOT
from oracle import frames as OF
from seam_match_rcnn_amd import _native, ops, transform as T
from seam_match_rcnn_amd.datasets import MFDataset as M                # the feature: absent, no import
from seam_match_rcnn_amd.datasets.MFDataset import MFBatchSampler, MovingFashionDataset, collate_fn, get_dataloader


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp("mf"))
    return MF.write(root), root


def dataset(tree, **kw):
    return MovingFashionDataset(tree[0], root=tree[1], **kw)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(MF.SAMPLER_CASES))
def test_sampler_equals_the_reference(name):
    n, batch_size, drop_last, kw, seed = MF.SAMPLER_CASES[name]
    with open(os.path.join(ROOT, "tests", "golden", "mf_sampler_golden.json")) as fp:
        golden = json.load(fp)[name]
    sampler = MFBatchSampler(None, torch.utils.data.SequentialSampler(range(n)), batch_size, drop_last, **kw)
    random.seed(seed)
    got = list(sampler)
    random.seed(seed)
    want = MF.reference_batches(range(n), batch_size, drop_last, **kw)
    assert got == want and all(isinstance(e, tuple) for b in got for e in b)
    assert MF.as_json(got) == golden["batches"]                        # the reference's own output, to the last bit of every t
    assert len(sampler) == golden["len"] == n // kw.get("n_products", 1) + (0 if drop_last else 1)
    assert len(got) > 0 and (name == "keep_last" or all(len(b) > 0 for b in got))


def test_sampler_shapes():
    """What the cases above are meant to reach, spelled out."""
    def run(name):
        n, batch_size, drop_last, kw, seed = MF.SAMPLER_CASES[name]
        random.seed(seed)
        return list(MFBatchSampler(None, torch.utils.data.SequentialSampler(range(n)), batch_size, drop_last, **kw))
    b = run("default")
    assert len(b) == 5 and all([e[1] for e in x] == ["in", "video", "video", "video"] for x in b)
    assert all(x[1][2] <= x[2][2] <= x[3][2] for x in b)
    assert [len(x) for x in run("n_products_2")] == [8, 8] and run("n_products_2")[0][4][0] == 1       # the fifth position is dropped
    assert [e[2] for e in run("uniform_sampling")[0][1:]] == [0.0, 0.5, 1.0]
    assert [e[2] for e in run("fixed_frame_float")[0][1:]] == [0.5, 0.5]
    assert [e[2] for e in run("fixed_frame_list")[1][1:]] == [0.1, 0.6, 0.9]
    assert [len(x) for x in run("first_n_withvideo")] == [4, 4, 1, 1, 1]
    assert all(len(e) == 4 and e[3] == 1 for x in run("fixed_video_i") for e in x[1:])
    assert {e[0] for x in run("fixed_ind") for e in x} == {1}
    one = run("batch_size_1")
    assert len(one) == 3 and [e[2] for e in one[0][1:]] == list(np.linspace(0.0, 1.0, 7))[:-1]
    assert [len(x) for x in run("keep_last")] == [8, 8, 4]


def test_get_dataloader(tree):
    ds = dataset(tree, lazy=True)
    loader = get_dataloader(ds, 3, False, n_products=1, is_seq=True, num_workers=0, fixed_video_i=1)
    assert isinstance(loader.batch_sampler, MFBatchSampler) and loader.collate_fn is collate_fn and len(loader) == 3
    assert isinstance(loader.batch_sampler.sampler, torch.utils.data.SequentialSampler)
    assert isinstance(get_dataloader(ds, 3, False, num_workers=0).batch_sampler.sampler, torch.utils.data.RandomSampler)
    random.seed(0)
    seen = []
    for images, targets in loader:
        assert len(images) == len(targets) == 3 and [t["tag"] for t in targets] == [1, 0, 0]
        assert [t["video_i"] for t in targets] == [-1, 1, 1] and len({t["i"] for t in targets}) == 1
        seen.append(targets[0]["i"])
    assert seen == [0, 1, 2]


# ---- the dataset -----------------------------------------------------------------------------------------------------------------

def test_product_ids_and_lists(tree):
    assert dataset(tree).product_ids == ["p0", "p1", "p2"] and len(dataset(tree)) == 3
    assert dataset(tree, blacklist=["p1"]).product_ids == ["p0", "p2"]
    assert dataset(tree, whitelist=["p2", "p1"]).product_ids == ["p1", "p2"]
    assert dataset(tree, blacklist=["p0"], whitelist=["p0"]).product_ids == ["p1", "p2"]       # the blacklist decides


def test_shop_sample(tree):
    ds = dataset(tree)
    for x in (1, (1, "in", None)):
        img, t = ds[x]
        assert np.array_equal(np.asarray(img), MF.shop_of("p1")) and img.size == (28, 40)
        assert t["tag"] == 1 and t["i"] == 1 and t["video_i"] == -1 and t["tracklet"] is None and t["index"] is None
        assert t["source"] == 0 and t["paths"] == {"video_paths": ["vid/p1_0.npy", "vid/p1_1.npy"], "img_path": "shop/p1.png"}
        assert t["boxes"].tolist() == [[0.0, 0.0, 28.0, 40.0]] and t["boxes"].dtype == torch.float32 and t["labels"].tolist() == [0]
        assert t["masks"].shape == (1, 40, 28) and t["masks"].dtype == torch.uint8 and bool(t["masks"].all())
        assert "valid" not in t and "index2" not in t and "frame_prep" not in t


@pytest.mark.parametrize("noise", [True, False])
def test_eager_frame_equals_the_oracle(tree, noise):
    ds = dataset(tree, noise=noise)
    for x, vid, frame in (((0, "video", 0.45, 0), 0, 2), ((0, "video", 0.7, 1), 1, 3), ((1, "video", 0.0, 0), 0, 0)):
        random.seed(5)
        np.random.seed(6)
        img, t = ds[x]
        random.seed(5)
        np.random.seed(6)
        sigma = 0.25 if random.random() > 0.75 else 0.05
        bgr = MF.stack_of(ds.product_ids[x[0]], vid)[frame]
        want = OF.prepare_frame(bgr, np.random.randn(*bgr.shape) if noise else None, sigma)
        assert np.array_equal(np.asarray(img), want)
        h, w = want.shape[:2]
        assert (h, w) == ((bgr.shape[0] // 2, bgr.shape[1] // 2) if noise else bgr.shape[:2])
        assert t["boxes"].tolist() == [[0.0, 0.0, float(w), float(h)]] and t["masks"].shape == (1, h, w) and bool(t["masks"].all())
        assert t["tag"] == 0 and t["valid"] is True and t["index2"] == frame and t["video_i"] == vid and t["index"] == x[2]
        want_box = MF.tracklets_of(ds.product_ids[x[0]])[vid].get(str(frame), [-1, -1, -1, -1])
        assert isinstance(t["tracklet"], np.ndarray) and t["tracklet"].tolist() == want_box
    assert ds[(0, "video", 0.7, 1)][1]["tracklet"].tolist() == [-1, -1, -1, -1]                # frame 3: no box
    assert ds[(2, "video", 0.5, 0)][1]["tracklet"] is None                                    # p2 has no tracklets


def test_tracklet_without_video_i_reads_video_0(tree):
    """The reference's rule, kept: a drawn video is looked up in the table of video 0."""
    ds = dataset(tree, noise=False)
    seen = set()
    for seed in range(8):
        random.seed(seed)
        img, t = ds[(0, "video", 0.45)]
        seen.add(t["video_i"])
        assert t["tracklet"].tolist() == MF.tracklets_of("p0")[0]["2"]
        assert np.array_equal(np.asarray(img), MF.stack_of("p0", t["video_i"])[2][:, :, ::-1])
    assert seen == {0, 1}


def test_integer_index_is_refused(tree):
    with pytest.raises(ValueError):
        dataset(tree)[(0, "video", 1, 0)]


class Unreadable:
    n_frames = 4

    def __init__(self, path):
        pass

    def read(self, k):
        return False, None


@pytest.mark.parametrize("lazy", [False, True])
def test_unreadable_frame(tree, lazy):
    ds = dataset(tree, lazy=lazy, frame_reader=Unreadable)
    random.seed(1)
    state = random.getstate()
    img, t = ds[(0, "video", 0.5, 1)]
    assert random.getstate() == state                                      # no sigma draw for a frame that was not read
    a = img.numpy() if lazy else np.asarray(img)
    assert a.shape == (100, 100, 3) and a.dtype == np.uint8 and not a.any()
    assert t["valid"] is False and t["index2"] == 2 and t["boxes"].tolist() == [[0.0, 0.0, 100.0, 100.0]]
    assert t["tracklet"].tolist() == MF.tracklets_of("p0")[1]["2"]
    if lazy:
        assert t["frame_prep"] == 0 and t["frame_sigma"] == 0.0 and "frame_seed" not in t and "masks" not in t
    else:
        assert t["masks"].shape == (1, 100, 100)
    assert ds[(0, "video", 0.99, 1)][1]["index2"] == 3
    out_of_range = dataset(tree, lazy=lazy)[(0, "video", 1.0, 1)]         # frame 5 of 5: the stack reader cannot read it
    assert out_of_range[1]["valid"] is False and tuple(out_of_range[0].shape if lazy else np.asarray(out_of_range[0]).shape) == (100, 100, 3)


def test_lazy_and_eager_share_the_random_stream(tree):
    flip = T.Compose([T.RandomHorizontalFlip(0.5)])
    entries = [(0, "in", None), (0, "video", 0.3), (0, "video", 0.8), (1, "in", None), (1, "video", 0.5), (2, "video", 0.2, 1)] * 3
    runs = []
    for lazy in (False, True):
        ds = dataset(tree, lazy=lazy, transform=T.Compose([T.ToTensor(lazy=lazy), flip]))
        random.seed(11)
        np.random.seed(12)
        rows = []
        for x in entries:
            calls = []
            real = random.random
            random.random = lambda: calls.append(real()) or calls[-1]
            try:
                img, t = ds[x]
            finally:
                random.random = real
            rows.append((t["video_i"], tuple(calls), t["boxes"].tolist(), img, t))
        runs.append((rows, random.getstate()))
    (eager, s0), (lazy, s1) = runs
    assert s0 == s1
    flips = 0
    for x, e, l in zip(entries, eager, lazy):
        assert e[:3] == l[:3]                                          # videos, the sigma and flip draws, the (flipped) boxes
        t = l[4]
        if x[1] == "video":
            sigma = 0.25 if e[1][0] > 0.75 else 0.05
            assert t["frame_prep"] == 2 and t["frame_sigma"] == sigma and 0 <= t["frame_seed"] < 2 ** 63
            assert l[3].dtype == torch.uint8 and tuple(l[3].shape[:2]) == (2 * (e[3].shape[1]) + l[3].shape[0] % 2, 2 * e[3].shape[2] + l[3].shape[1] % 2)
            flipped = e[1][1] < 0.5
        else:
            assert t["frame_prep"] == 0 and t["frame_sigma"] == 0.0 and "frame_seed" not in t
            assert torch.equal(l[3], (e[3].flip(-1) if e[1][0] < 0.5 else e[3]).mul(255).round().to(torch.uint8).permute(1, 2, 0))
            flipped = e[1][0] < 0.5
        assert bool(t.get("hflip", False)) == flipped and "masks" not in t and "masks" in e[4]
        flips += flipped
    assert 0 < flips < len(entries)
    assert len({(r[4]["i"], r[0]) for r in lazy if r[4]["tag"] == 0}) > 3          # more than one video per product was drawn


def test_lazy_targets(tree):
    ds = dataset(tree, lazy=True)
    np.random.seed(3)
    random.seed(3)
    img, t = ds[(0, "video", 0.45, 0)]
    bgr = MF.stack_of("p0", 0)[2]
    assert isinstance(img, torch.Tensor) and img.dtype == torch.uint8 and np.array_equal(img.numpy(), bgr)     # BGR, full resolution
    np.random.seed(3)
    assert t["frame_prep"] == 2 and t["frame_sigma"] in (0.05, 0.25) and t["frame_seed"] == int(np.random.randint(0, 2 ** 63))
    assert t["boxes"].tolist() == [[0.0, 0.0, 26.0, 18.0]] and "masks" not in t and t["valid"] is True and t["index2"] == 2
    img, t = ds[0]
    assert np.array_equal(img.numpy(), MF.shop_of("p0")) and t["frame_prep"] == 0 and t["frame_sigma"] == 0.0 and "frame_seed" not in t
    state = np.random.get_state()[1].copy()
    img, t = dataset(tree, lazy=True, noise=False)[(0, "video", 0.45, 0)]
    assert np.array_equal(img.numpy(), bgr) and t["frame_prep"] == 1 and "frame_seed" not in t
    assert t["boxes"].tolist() == [[0.0, 0.0, 53.0, 37.0]] and np.array_equal(np.random.get_state()[1], state)
    # the flip of a frame that is still at full resolution moves the boxes inside the half-size image
    random.seed(0)
    img, t = dataset(tree, lazy=True, transform=T.RandomHorizontalFlip(1.0))[(0, "video", 0.45, 0)]
    t["boxes"][0, 2] = 20.0
    img, t = T.RandomHorizontalFlip(1.0)(img, t)
    assert t["boxes"].tolist() == [[6.0, 0.0, 26.0, 18.0]] and t["hflip"] is False


# ---- the frame readers -------------------------------------------------------------------------------------------------------------

def test_without_cv2_the_error_names_the_hook(tree, monkeypatch):
    real = builtins.__import__

    def no_cv2(name, *a, **k):
        if name == "cv2":
            raise ImportError("No module named 'cv2'")
        return real(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_cv2)
    monkeypatch.delitem(sys.modules, "cv2", raising=False)
    with pytest.raises(ImportError, match="frame_reader"):
        M.open_frames(os.path.join(tree[1], "vid", "clip.mp4"))
    data = {"p": {"img_path": "shop/p0.png", "video_paths": ["vid/clip.mp4"], "source": 1}}
    path = os.path.join(tree[1], "mp4.json")
    with open(path, "w") as fp:
        json.dump(data, fp)
    ds = MovingFashionDataset(path, root=tree[1])
    assert ds[0][0].size == (45, 31)                                       # shop images need no reader
    with pytest.raises(ImportError, match="frame_reader"):
        ds[(0, "video", 0.5)]
    assert "cv2" not in sys.modules


def test_module_imports_no_decoder_or_vision_package():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); import seam_match_rcnn_amd.datasets.MFDataset; "
            "print([m for m in ('cv2', 'torchvision', 'pycocotools') if m in sys.modules])" % ROOT)
    assert subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True).stdout.strip() == "[]"


def test_npy_reader_pickles(tree):
    path = os.path.join(tree[1], "vid", "p0_0.npy")
    r = M.NpyFrameReader(path)
    assert r.n_frames == MF.FRAMES and isinstance(r.stack, np.memmap)
    ok, frame = r.read(4)
    assert ok and np.array_equal(frame, MF.stack_of("p0", 0)[4]) and frame.flags.writeable
    assert r.read(5) == (False, None) and r.read(-1) == (False, None)
    r2 = pickle.loads(pickle.dumps(r))                                     # with the map open
    assert r2.path == path and r2.n_frames == MF.FRAMES and np.array_equal(r2.read(1)[1], MF.stack_of("p0", 0)[1])
    assert pickle.loads(pickle.dumps(M.open_frames)) is M.open_frames and isinstance(M.open_frames(path), M.NpyFrameReader)
    ds = pickle.loads(pickle.dumps(dataset(tree, lazy=True)))             # what a dataloader worker receives
    assert np.array_equal(ds[(0, "video", 0.0, 0)][0].numpy(), MF.stack_of("p0", 0)[0])
    bad = os.path.join(tree[1], "bad.npy")
    np.save(bad, np.zeros((2, 3, 3), np.uint8))
    with pytest.raises(ValueError):
        M.NpyFrameReader(bad)


# ---- ops.frames_prepare_batch without a device ---------------------------------------------------------------------------------------

def test_frames_prepare_batch_argument_errors(monkeypatch):
    img = torch.zeros(4, 6, 3, dtype=torch.uint8)
    if not torch.cuda.is_available():
        with pytest.raises(_native.SeamNativeError):
            ops.frames_prepare_batch([img], [2], [0.05], [1])
        with pytest.raises(_native.SeamNativeError):
            ops.frames_prepare_flat(img.reshape(-1), None, None, None, None, None, None, 4, 6)
        from seam_match_rcnn_amd import frames
        with pytest.raises(_native.SeamNativeError):
            frames.prepare_frames([img], [{"frame_prep": 2, "frame_sigma": 0.05, "frame_seed": 1}], "cuda:0")
    with pytest.raises(_native.SeamNativeError):
        ops.frames_prepare_batch([img.numpy()], [2], [0.05], [1])         # not a tensor: refused before anything else
    with pytest.raises(ValueError):                                        # draws of the wrong type are refused before the device is asked for
        ops.frames_prepare_batch([img], [2], [0.05], [1], noise_values=[torch.zeros(4, 6, 3)])
    with pytest.raises(ValueError):
        ops.frames_prepare_batch([img], [2], [0.05], [1], noise_values=[])
    # the checks behind the device check, with a device pretended (nothing is launched: every call is refused before the staging)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    for bad in (dict(modes=[3]), dict(modes=[2, 2]), dict(sigmas=[float("inf")]), dict(seeds=[]), dict(images=[]),
                dict(images=[torch.zeros(1, 6, 3, dtype=torch.uint8)]), dict(images=[torch.zeros(4, 6, 4, dtype=torch.uint8)])):
        kw = dict(images=[img], modes=[2], sigmas=[0.05], seeds=[1])
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.frames_prepare_batch(**kw)
    with pytest.raises(TypeError):
        ops.frames_prepare_batch([img.float()], [2], [0.05], [1])
    assert ops.frame_out_size(37, 53, 2) == (18, 26) and ops.frame_out_size(37, 53, 1) == (37, 53) and ops.frame_out_size(3, 2, 0) == (3, 2)
