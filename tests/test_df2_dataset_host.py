"""CPU: ``datasets.DF2Dataset``, ``transform`` and ``utils`` -- the data side of the phase-1 loop -- on the hand-made fixture of
tests/df2_fixture.py.  Every expected value below is worked out by hand from that file's tables."""
import random

import numpy as np
import pytest
import torch

import df2_fixture as FX
from seam_match_rcnn_amd.datasets.DF2Dataset import (DF2MatchingSampler, DeepFashion2Dataset, DistributedSampler, RandomSampler,
                                                    get_dataloader)
from seam_match_rcnn_amd.transform import Compose, RandomHorizontalFlip, ToTensor
from seam_match_rcnn_amd.utils import collate_fn, warmup_lr_scheduler


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    return FX.write(tmp_path_factory.mktemp("df2"))


@pytest.fixture(scope="module")
def lazy_ds(files):
    return DeepFashion2Dataset(files[0], files[1], lazy=True)


def test_index_maps_and_accepted_entries(lazy_ds):
    ds = lazy_ds
    assert ds.ids == [1, 2, 3, 4, 5, 6, 7, 8] and len(ds) == 8
    assert ds.categories == {3: "short sleeve top", 1: "trousers", 13: "sling dress"}
    assert ds.json_category_id_to_contiguous_id == {3: 1, 1: 2, 13: 3}                # file order, not id order
    assert ds.contiguous_category_id_to_json_id == {1: 3, 2: 1, 3: 13}
    assert ds.id_to_img_map == {k: k + 1 for k in range(8)} and ds.idx_to_id_map == {k + 1: k for k in range(8)}
    assert ds.street_inds == [1, 2, 4, 6, 8] and ds.shop_inds == [3, 5, 7]
    assert ds.match_map_street == {"1_101": [1, 2], "2_202": [4], "1_303": [6]}      # style '0' skipped, image 8 has no key
    assert ds.match_map_shop == {"1_101": [3], "1_303": [5], "3_404": [7]}
    assert sorted(ds.accepted_entries) == [1, 2, 3, 5, 6] and len(set(ds.accepted_entries)) == 5
    assert ds.get_img_info(4) == ds.coco.imgs[5] and ds.coco.imgs[5]["source"] == "shop"
    assert ds.coco.cats[13]["name"] == "sling dress"


def test_lazy_sample_filters_and_keeps_the_annotations(lazy_ds):
    img, t, image_id = lazy_ds[0]                                                     # image 1: kept, crowd, area 0, kept
    assert image_id == 1
    assert img.dtype == torch.uint8 and tuple(img.shape) == (40, 56, 3) and np.array_equal(img.numpy(), FX.pixels(1))
    assert torch.equal(t["boxes"], torch.tensor([[4., 5., 24., 29.], [28., 10., 50.5, 35.]])) and t["boxes"].dtype == torch.float32
    assert t["labels"].tolist() == [3, 2] and t["labels"].dtype == torch.int64 and t["classes"] is t["labels"]
    assert torch.equal(t["area"], torch.tensor([480.0, 310.5]))
    assert t["pair_ids"].tolist() == [101, 101] and t["styles"].tolist() == [1, 0] and t["sources"].tolist() == [0, 0]
    assert t["size"] == (40, 56) and "masks" not in t
    assert t["segmentation"] == [FX.ANNOTATIONS[0]["segmentation"], FX.ANNOTATIONS[3]["segmentation"]]
    img3, t3, id3 = lazy_ds[2]                                                        # a shop image
    assert id3 == 3 and t3["sources"].tolist() == [1] and t3["labels"].tolist() == [3] and t3["size"] == (48, 40)
    assert torch.equal(t3["boxes"], torch.tensor([[5., 6., 33., 42.]]))


def test_eager_dataset_is_refused_inside_a_worker(files, monkeypatch):
    ds = DeepFashion2Dataset(files[0], files[1])
    monkeypatch.setattr(torch.utils.data, "get_worker_info", lambda: object())
    with pytest.raises(RuntimeError, match="num_workers=0"):
        ds[0]


def _keys(ds, img_id):
    return {s + "_" + str(p) for s, p in ds.coco.imgs[img_id]["match_desc"].items() if s != "0"}


def test_matching_sampler_yields_street_shop_pairs(lazy_ds):
    ds = lazy_ds
    base = RandomSampler(ds)
    assert len(base) == 5 and sorted(base) == [0, 1, 2, 3, 4]
    sampler = DF2MatchingSampler(ds, base, 4, drop_last=True)
    assert len(sampler) == 5 // (4 // 2) == 2
    random.seed(3)
    torch.manual_seed(3)
    seen = set()
    for _ in range(4):
        batches = list(sampler)
        assert len(batches) == 2                             # 5 accepted images, each with a partner: 10 indices, 2 left over
        for b in batches:
            assert len(b) == 4
            for k in range(0, 4, 2):
                street, shop = ds.id_to_img_map[b[k]], ds.id_to_img_map[b[k + 1]]
                assert street in ds.street_inds and shop in ds.shop_inds
                assert _keys(ds, street) & _keys(ds, shop)
                seen.add((street, shop))
    assert seen == {(1, 3), (2, 3), (6, 5)}                  # product 101's shop image meets both of its street images
    rest = DF2MatchingSampler(ds, base, 4, drop_last=False)
    assert [len(b) for b in rest] == [4, 4, 2] and len(rest) == (5 + 3) // 4
    with pytest.raises(ValueError):
        DF2MatchingSampler(ds, [0, 1], 4, True)
    with pytest.raises(ValueError):
        DF2MatchingSampler(ds, base, True, True)


def test_distributed_sampler_shards(lazy_ds):
    shards = [DistributedSampler(lazy_ds, num_replicas=2, rank=r) for r in range(2)]
    assert [len(s) for s in shards] == [3, 3] and [(s.world, s.rank, s.per_rank) for s in shards] == [(2, 0, 3), (2, 1, 3)]
    for epoch in (0, 1, 7):
        for s in shards:
            s.set_epoch(epoch)
        a, b = list(shards[0]), list(shards[1])
        assert len(a) == len(b) == 3
        assert sorted(a + b[:2]) == [0, 1, 2, 3, 4]          # disjoint before the padding ...
        assert b[2] == a[0]                                  # ... which repeats the permutation's head
        g = torch.Generator().manual_seed(epoch)
        assert a + b[:2] == torch.randperm(5, generator=g).tolist()
        assert list(shards[0]) == a and list(shards[1]) == b                          # the same epoch gives the same shards
    plain = DistributedSampler(lazy_ds, num_replicas=2, rank=1, shuffle=False)
    assert list(plain) == [3, 4, 0]


def test_to_tensor_is_bytes_over_255(files):
    from PIL import Image
    pil = Image.open(f"{files[1]}/2.png")
    bytes_ = torch.from_numpy(FX.pixels(2))
    x, t = ToTensor()(pil, {"k": 1})
    assert t == {"k": 1} and x.dtype == torch.float32 and tuple(x.shape) == (3, 37, 53) and x.is_contiguous()
    assert torch.equal(x, bytes_.permute(2, 0, 1).float().div(255))
    assert torch.equal(ToTensor()(bytes_, {})[0], x)
    lazy = ToTensor(lazy=True)(pil, {})[0]
    assert lazy.dtype == torch.uint8 and torch.equal(lazy, bytes_)


def test_lazy_and_eager_flip_decide_alike(files):
    from PIL import Image
    pil = Image.open(f"{files[1]}/1.png")
    boxes = torch.tensor([[4., 5., 24., 29.], [28., 10., 50.5, 35.]])
    masks = torch.zeros((2, 40, 56), dtype=torch.uint8)
    masks[0, 5:29, 4:24] = 1
    masks[1, 10:35, 28:50] = 1
    eager = Compose([ToTensor(), RandomHorizontalFlip(0.5)])
    lazy = Compose([ToTensor(lazy=True), RandomHorizontalFlip(0.5)])
    plain = ToTensor()(pil, {})[0]
    flipped = []
    for k in range(12):
        random.seed(k)
        want = random.random() < 0.5
        random.seed(k)
        xe, te = eager(pil, {"boxes": boxes.clone(), "masks": masks.clone()})
        drawn_e = random.random()
        random.seed(k)
        xl, tl = lazy(pil, {"boxes": boxes.clone(), "segmentation": [[], []], "size": (40, 56)})
        drawn_l = random.random()
        assert drawn_e == drawn_l                            # one draw per call in both forms
        assert bool(tl.get("hflip", False)) == want
        assert torch.equal(te["boxes"], tl["boxes"])
        assert torch.equal(xl, torch.from_numpy(FX.pixels(1)))                       # the bytes are left alone
        if want:
            assert torch.equal(te["boxes"], torch.tensor([[32., 5., 52., 29.], [5.5, 10., 28., 35.]]))   # 56 - x2, 56 - x1
            assert torch.equal(xe, plain.flip(-1)) and torch.equal(te["masks"], masks.flip(-1))
        else:
            assert torch.equal(te["boxes"], boxes) and torch.equal(xe, plain) and torch.equal(te["masks"], masks)
        flipped.append(want)
    assert any(flipped) and not all(flipped)
    random.seed(0)
    with pytest.raises(ValueError, match="segmentation"):
        RandomHorizontalFlip(1.0)(torch.from_numpy(FX.pixels(1)), {"boxes": boxes.clone(), "masks": masks})


def test_dataloader_over_the_lazy_dataset(files):
    ds = DeepFashion2Dataset(files[0], files[1], Compose([ToTensor(lazy=True), RandomHorizontalFlip(0.5)]), lazy=True)
    random.seed(5)
    torch.manual_seed(5)
    loader = get_dataloader(ds, 2, False)
    assert len(loader) == 5
    n = 0
    for images, targets, ids in loader:
        assert len(images) == len(targets) == len(ids) == 2
        assert ids[0] in ds.street_inds and ids[1] in ds.shop_inds
        for img, t, i in zip(images, targets, ids):
            assert img.dtype == torch.uint8 and tuple(img.shape) == FX.SIZES[i] + (3,) and t["size"] == FX.SIZES[i]
            assert len(t["segmentation"]) == len(t["boxes"]) == len(t["labels"])
        n += 1
    assert n == 5


def test_collate_and_warmup():
    assert collate_fn([(1, "a", 10), (2, "b", 20)]) == ((1, 2), ("a", "b"), (10, 20))
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=0.5)
    sched = warmup_lr_scheduler(opt, 4, 0.2)
    lrs = []
    for _ in range(6):
        lrs.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step()
    assert lrs == pytest.approx([0.5 * v for v in (0.2, 0.4, 0.6, 0.8, 1.0, 1.0)])
