"""CPU: ``datasets.MultiDF2Dataset`` -- the data side of phase 2 -- on the hand-made fixture of tests/df2_fixture.py, and the noise
tables ``ops.stage_u8_batch`` appends.  Every expected value is worked out by hand from that file's tables; the eager noise is
compared with the reference's arithmetic (``MultiDF2Dataset.py:157-167``), written out below."""
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

import df2_fixture as FX
from conftest import ROOT
from seam_match_rcnn_amd import ops, ops_input
from seam_match_rcnn_amd.datasets.DF2Dataset import DeepFashion2Dataset, RandomSampler
from seam_match_rcnn_amd.datasets.MultiDF2Dataset import (MultiDeepFashion2Dataset, MultiDF2BatchSampler,       # the feature: absent,
                                                         get_dataloader)                                       # no import
from seam_match_rcnn_amd.transform import Compose, RandomHorizontalFlip, ToTensor
from seam_match_rcnn_amd.utils import collate_fn


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return FX.write(tmp_path_factory.mktemp("mdf2"))


@pytest.fixture()
def no_device_masks(monkeypatch):
    """The eager form rasterises ``"masks"`` on the HIP device; these tests are about the image, so the masks are left zero."""
    monkeypatch.setattr(DeepFashion2Dataset, "_masks", lambda self, kept, h, w: torch.zeros((len(kept), h, w), dtype=torch.uint8))


def test_match_maps_and_the_onestreet_filter(files):
    ds = MultiDeepFashion2Dataset(files[0], files[1], lazy=True)
    assert ds.match_map_street == {"1_101": [1, 2], "2_202": [4], "1_303": [6]}
    assert ds.match_map_shop == {"1_101": [3], "1_303": [5], "3_404": [7]}
    assert len(ds) == 3
    assert MultiDF2BatchSampler(ds, RandomSampler(ds, entries=[0, 1]), 2, True, n_products=1).pair_keys == ["1_101", "1_303"]
    one = MultiDeepFashion2Dataset(files[0], files[1], filter_onestreet=True, lazy=True)
    assert one.match_map_street == {"1_101": [1, 2]} and one.match_map_shop == {"1_101": [3]} and len(one) == 1
    assert MultiDF2BatchSampler(one, RandomSampler(one, entries=[0]), 2, True, n_products=1).pair_keys == ["1_101"]


def test_addressing_and_target(files):
    ds = MultiDeepFashion2Dataset(files[0], files[1], lazy=True)
    plain = DeepFashion2Dataset(files[0], files[1], lazy=True)
    for t, want in ((0.0, 1), (0.49, 1), (0.5, 2), (0.99, 2)):
        img, target, image_id = ds[("1_101", "street", t)]
        assert image_id == want and np.array_equal(img.numpy(), FX.pixels(want))
        assert target["i"] == "1_101" and target["tag"] == 0
        _, base, base_id = plain[want - 1]
        assert base_id == image_id
        assert set(target) == set(base) | {"i", "tag", "noise_sigma"} and target["noise_sigma"] == 0.0
        for k, v in base.items():
            assert torch.equal(target[k], v) if torch.is_tensor(v) else target[k] == v, k
    img, target, image_id = ds[("1_101", "shop", None)]
    assert image_id == 3 and target["tag"] == 1 and target["i"] == "1_101" and np.array_equal(img.numpy(), FX.pixels(3))
    assert target["sources"].tolist() == [1] and target["size"] == (48, 40) and "masks" not in target


def reference_noise(img_id, seed, noise):
    """ref MultiDF2Dataset.py:157-167 after ``random.seed(seed); np.random.seed(seed)`` for a street image (no earlier draw)."""
    random.seed(seed)
    np.random.seed(seed)
    tmp_noise = (0.1 if random.random() > 0.75 else 0.0) if noise else 0.0
    image = FX.pixels(img_id)
    image = image / 255.0
    image += np.random.randn(*image.shape) * tmp_noise
    image = image * 255.0
    image = np.clip(image, 0, 255.0)
    return np.asarray(image, dtype=np.uint8), tmp_noise, random.getstate(), np.random.randn()


def test_eager_noise_is_the_reference_arithmetic(files, no_device_masks):
    ds = MultiDeepFashion2Dataset(files[0], files[1], noise=True)
    seen = set()
    for seed in range(8):
        want, sigma, state, next_draw = reference_noise(2, seed, True)
        random.seed(seed)
        np.random.seed(seed)
        img, target, image_id = ds[("1_101", "street", 0.7)]
        assert image_id == 2 and np.array_equal(np.array(img), want), seed
        assert random.getstate() == state and np.random.randn() == next_draw          # the same draws were made, sigma 0 or not
        assert np.array_equal(want, FX.pixels(2)) == (sigma == 0.0)
        assert "noise_sigma" not in target and "noise_seed" not in target and "masks" in target
        seen.add(sigma)
    assert seen == {0.0, 0.1}
    off = MultiDeepFashion2Dataset(files[0], files[1], noise=False)
    random.seed(1)
    np.random.seed(1)
    state = random.getstate()
    img, _, _ = off[("1_101", "street", 0.7)]
    assert np.array_equal(np.array(img), FX.pixels(2)) and random.getstate() == state          # noise=False draws nothing from random
    assert np.random.randn() == reference_noise(2, 1, False)[3]                               # ... and randn all the same
    x, _, _ = MultiDeepFashion2Dataset(files[0], files[1], ToTensor())[("1_101", "shop", None)]
    assert x.dtype == torch.float32 and tuple(x.shape) == (3, 48, 40)


def test_byte_round_trip_is_the_identity():
    v = np.arange(256, dtype=np.uint8)
    assert np.array_equal(np.asarray(np.clip(v / 255.0 * 255.0, 0, 255.0), dtype=np.uint8), v)


def test_lazy_form_keeps_the_random_stream_and_the_bytes(files, no_device_masks):
    tf_e, tf_l = Compose([ToTensor(), RandomHorizontalFlip(0.5)]), Compose([ToTensor(lazy=True), RandomHorizontalFlip(0.5)])
    eager = MultiDeepFashion2Dataset(files[0], files[1], tf_e, noise=True)
    lazy = MultiDeepFashion2Dataset(files[0], files[1], tf_l, noise=True, lazy=True)
    seen = set()
    for seed in range(8):
        for entry in (("1_101", "shop", None), ("1_101", "street", 0.2)):
            random.seed(seed)
            np.random.seed(seed)
            _, te, ide = eager[entry]
            after_eager = random.getstate()
            random.seed(seed)
            np.random.seed(seed)
            if entry[1] == "shop":
                random.choice([3])
            sigma = 0.1 if random.random() > 0.75 else 0.0
            want_seed = int(np.random.randint(0, 2 ** 63)) if sigma > 0 else None
            random.seed(seed)
            np.random.seed(seed)
            img, tl, idl = lazy[entry]
            assert random.getstate() == after_eager and ide == idl
            assert tl["noise_sigma"] == sigma and isinstance(tl["noise_sigma"], float)
            assert ("noise_seed" in tl) == (sigma > 0) and tl.get("noise_seed") == want_seed
            assert img.dtype == torch.uint8 and np.array_equal(img.numpy(), FX.pixels(idl))       # bytes: no noise, no flip yet
            assert bool(tl.get("hflip", False)) == ("hflip" in tl) and torch.equal(tl["boxes"], te["boxes"])
            assert "segmentation" in tl and tl["size"] == FX.SIZES[idl] and "masks" not in tl
            seen.add(sigma)
    assert seen == {0.0, 0.1}
    quiet = MultiDeepFashion2Dataset(files[0], files[1], noise=False, lazy=True)
    random.seed(0)
    state = random.getstate()
    _, t, _ = quiet[("1_303", "street", 0.0)]
    assert t["noise_sigma"] == 0.0 and "noise_seed" not in t and random.getstate() == state


def test_batch_sampler(files):
    ds = MultiDeepFashion2Dataset(files[0], files[1], lazy=True)
    base = RandomSampler(ds, entries=[0, 1])
    sampler = MultiDF2BatchSampler(ds, base, 6, True, n_products=2)
    assert len(sampler) == 2 // 2 == 1 and len(MultiDF2BatchSampler(ds, base, 6, False, n_products=2)) == 2
    random.seed(4)
    torch.manual_seed(4)
    first = [list(sampler) for _ in range(3)]
    for batches in first:
        assert len(batches) == 1
        (b,) = batches
        assert [e[1] for e in b] == ["shop", "street", "street"] * 2
        assert {b[0][0], b[3][0]} == {"1_101", "1_303"}
        for p in (0, 3):
            assert b[p][2] is None and b[p + 1][0] == b[p + 2][0] == b[p][0]
            assert 0.0 <= b[p + 1][2] <= b[p + 2][2] < 1.0
    random.seed(4)
    torch.manual_seed(4)
    assert [list(sampler) for _ in range(3)] == first
    rest = list(MultiDF2BatchSampler(ds, base, 9, False, n_products=3))            # 2 products of 3 entries: never a full batch
    assert [len(b) for b in rest] == [6]
    for bad in (dict(batch_size=6, n_products=0), dict(batch_size=5, n_products=2), dict(batch_size=True, n_products=1)):
        with pytest.raises(ValueError):
            MultiDF2BatchSampler(ds, base, drop_last=True, **bad)
    with pytest.raises(ValueError):
        MultiDF2BatchSampler(ds, [0, 1], 6, True, n_products=2)


_ORDER = """
import json, random, sys, torch
sys.path.insert(0, {root!r})
from seam_match_rcnn_amd.datasets.MultiDF2Dataset import MultiDeepFashion2Dataset, get_dataloader
ds = MultiDeepFashion2Dataset({ann!r}, {img!r}, lazy=True)
random.seed(9)
torch.manual_seed(9)
print(json.dumps([list(b) for _ in range(3) for b in get_dataloader(ds, 3, False, n_products=1).batch_sampler]))
"""


def test_order_does_not_depend_on_the_hash_seed(files):
    ds = MultiDeepFashion2Dataset(files[0], files[1], lazy=True)
    random.seed(9)
    torch.manual_seed(9)
    here = [[list(e) for e in b] for _ in range(3) for b in get_dataloader(ds, 3, False, n_products=1).batch_sampler]
    assert len(here) == 6 and {b[0][0] for b in here} == {"1_101", "1_303"}
    code = _ORDER.format(root=ROOT, ann=files[0], img=files[1])
    for hash_seed in ("1", "2"):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True,
                             env=dict(os.environ, PYTHONHASHSEED=hash_seed)).stdout
        assert json.loads(out) == here


def test_dataloader_collates_products(files):
    ds = MultiDeepFashion2Dataset(files[0], files[1], ToTensor(lazy=True), noise=True, lazy=True)
    random.seed(6)
    torch.manual_seed(6)
    loader = get_dataloader(ds, 3, False, n_products=1)
    assert loader.collate_fn is collate_fn and len(loader) == 2
    keys = []
    for images, targets, ids in loader:
        assert len(images) == len(targets) == len(ids) == 3
        assert [t["tag"] for t in targets] == [1, 0, 0] and len({t["i"] for t in targets}) == 1
        assert ids[0] in ds.match_map_shop[targets[0]["i"]] and all(i in ds.match_map_street[targets[0]["i"]] for i in ids[1:])
        keys.append(targets[0]["i"])
    assert sorted(keys) == ["1_101", "1_303"]


def test_noise_tables_follow_the_last_image(monkeypatch):
    monkeypatch.setattr(ops_input, "_staging", lambda nbytes, device: torch.full((nbytes + 64,), 0xEE, dtype=torch.uint8))   # unpinned
    rng = np.random.RandomState(0)
    imgs = [torch.from_numpy(rng.randint(0, 256, (5, 7, 3)).astype(np.uint8)), torch.from_numpy(rng.randint(0, 256, (4, 3, 3)).astype(np.uint8))]
    args = (imgs, [(10, 14), (8, 6)], 32, 32, [True, False], "cuda:0")
    plain, n = ops.stage_u8_batch(*args)
    assert n == 2 and plain.numel() == 64 + 105 + 36 == 205
    noisy, n2 = ops.stage_u8_batch(*args, noise=([0.1, 0.0], [2 ** 63 + 5, 7]))
    assert n2 == 2 and noisy.numel() == 208 + 32 and torch.equal(noisy[:205], plain)
    raw = noisy.numpy()
    assert not raw[205:208].any()
    assert raw[208:224].view(np.float64).tolist() == [0.1, 0.0] and raw[224:240].view(np.uint64).tolist() == [2 ** 63 + 5, 7]
    assert np.array_equal(raw[64:169], imgs[0].numpy().reshape(-1)) and np.array_equal(raw[169:205], imgs[1].numpy().reshape(-1))
    with pytest.raises(ValueError):
        ops.stage_u8_batch(*args, noise=([0.1], [1, 2]))
    with pytest.raises(ValueError):
        ops.stage_u8_batch(*args, noise=([0.1, float("nan")], [1, 2]))
    with pytest.raises(ValueError):
        ops.stage_u8_batch(*args[:5], None, noise=([0.1, 0.0], [1, 2]))
