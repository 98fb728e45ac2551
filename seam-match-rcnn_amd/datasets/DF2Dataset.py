"""DeepFashion2 for the phase-1 loop: ``DeepFashion2Dataset``, ``RandomSampler``, ``DistributedSampler``, ``DF2MatchingSampler``
and ``get_dataloader`` -- the names a loop written against the reference's ``datasets/DF2Dataset.py`` imports -- without
torchvision, pycocotools or ``torch._six``.

The annotation file is the COCO-format json that ``DeepFtoCoco.py`` writes (``images`` with ``source`` and ``match_desc``,
``annotations`` with ``pair_id`` / ``style`` / ``source``, ``categories``) and is indexed here.  Images are opened with Pillow.

Two forms of a sample:

* ``lazy=False`` -- dense masks: ``target["masks"]`` is built per object with ``mask_utils.annToMask``.  That rasterises on the HIP
  device, so this form is for ``num_workers=0``; inside a dataloader worker it raises.
* ``lazy=True`` -- the image is the uint8 ``[H,W,3]`` tensor of the decoded RGB bytes and the target carries
  ``"segmentation"`` (one entry per kept object) and ``"size"`` ``(h, w)`` instead of ``"masks"``: the contract of
  ``mask_utils.targets_to_device`` and ``input_pipeline.prepare_batch``.  Nothing touches the device, so workers are fine.
"""
from __future__ import annotations

import json
import os
import random

import torch
from torch.utils.data import DataLoader, Dataset, Sampler

from ..transform import image_bytes
from ..utils import collate_fn

STREET, SHOP = "user", "shop"      # the two values of an image's and an annotation's ``source``

# per-object annotation fields that become target tensors: (annotation key, target key, value of one object)
_OBJECT_FIELDS = (("pair_id", "pair_ids", lambda o: o["pair_id"]),
                  ("style", "styles", lambda o: o["style"]),
                  ("source", "sources", lambda o: int(o["source"] != STREET)))


class _CocoIndex:
    """What callers reach for through ``dataset.coco``: ``imgs`` and ``cats`` by id; plus each image's annotations in file order
    and the category ids in file order."""

    def __init__(self, doc: dict):
        self.imgs = {entry["id"]: entry for entry in doc.get("images", ())}
        self.cats = {entry["id"]: entry for entry in doc.get("categories", ())}
        self.cat_order = [entry["id"] for entry in doc.get("categories", ())]
        self.anns_of = {img_id: [] for img_id in self.imgs}
        for ann in doc.get("annotations", ()):
            self.anns_of.setdefault(ann["image_id"], []).append(ann)


def _match_keys(image_entry: dict, skip_zero: bool) -> list:
    """``"<style>_<pair_id>"`` for every entry of an image's ``match_desc``; style ``'0'`` (no style annotated) left out on request."""
    return [f"{style}_{pair}" for style, pair in image_entry["match_desc"].items() if not (skip_zero and style == "0")]


class DeepFashion2Dataset(Dataset):
    """``dataset[idx] -> (img, target, image_id)`` over the images of ``ann_file`` in the order of their sorted ids.

    Attributes a loop or a sampler reads: ``ids`` (sorted image ids), ``categories`` (id -> name),
    ``json_category_id_to_contiguous_id`` and ``contiguous_category_id_to_json_id``, ``id_to_img_map`` (position -> image id) and
    ``idx_to_id_map`` (image id -> position), ``street_inds`` / ``shop_inds`` (ids of the images whose ``source`` is ``'user'`` /
    ``'shop'``), ``match_map_street`` / ``match_map_shop`` (``"<style>_<pair_id>"`` -> image ids of that side, style ``'0'``
    skipped), ``accepted_entries`` (ids of the images whose key occurs on both sides) and ``coco`` (``imgs``, ``cats``).

    The contiguous label of a category is 1 + its position in the file's ``categories`` list.  The reference takes the order
    of pycocotools' ``getCatIds()``, which returns the categories in file order as far as its published source shows;
    pycocotools is not installed where this project is tested, so that is not verified.

    Objects kept in a target: ``iscrowd == 0`` and ``area != 0``.  ``boxes`` are float32 xyxy in image pixels; ``labels`` and
    ``classes`` are the contiguous labels; ``area``, ``pair_ids``, ``styles`` and ``sources`` (0 street, 1 shop) are present when
    the image's first non-crowd annotation carries the field.  The third element is the ``image_id`` of that annotation, or the
    image's own id when every object is a crowd."""

    def __init__(self, ann_file, root, transforms=None, lazy: bool = False):
        with open(ann_file) as f:
            self.coco = _CocoIndex(json.load(f))
        self.root, self.transforms, self.lazy = root, transforms, bool(lazy)
        self.ids = sorted(self.coco.imgs)
        self.id_to_img_map = dict(enumerate(self.ids))
        self.idx_to_id_map = {img_id: pos for pos, img_id in self.id_to_img_map.items()}
        self.categories = {cat_id: cat["name"] for cat_id, cat in self.coco.cats.items()}
        self.json_category_id_to_contiguous_id = {cat_id: label for label, cat_id in enumerate(self.coco.cat_order, start=1)}
        self.contiguous_category_id_to_json_id = {label: cat_id for cat_id, label in self.json_category_id_to_contiguous_id.items()}
        self.street_inds, self.match_map_street = self._side(STREET)
        self.shop_inds, self.match_map_shop = self._side(SHOP)
        both = self.match_map_street.keys() & self.match_map_shop.keys()
        self.accepted_entries = sorted({img_id for side in (self.match_map_street, self.match_map_shop) for key in both
                                        for img_id in side[key]})

    def _side(self, source: str):
        """(ids of the images of one source, match key -> those of them that carry it)."""
        ids = [img_id for img_id in self.ids if self.coco.imgs[img_id]["source"] == source]
        by_key = {}
        for img_id in ids:
            for key in _match_keys(self.coco.imgs[img_id], skip_zero=True):
                by_key.setdefault(key, []).append(img_id)
        return ids, by_key

    def __len__(self):
        return len(self.ids)

    def get_img_info(self, index):
        return self.coco.imgs[self.ids[index]]

    def _masks(self, kept, h, w):
        if torch.utils.data.get_worker_info() is not None:
            raise RuntimeError("DeepFashion2Dataset(lazy=False) rasterises its masks on the HIP device (mask_utils.annToMask) "
                               "and cannot run inside a dataloader worker: use num_workers=0, or lazy=True with "
                               "input_pipeline.prepare_batch")
        from ..mask_utils import annToMask
        masks = torch.zeros((len(kept), h, w), dtype=torch.uint8)
        for k, obj in enumerate(kept):
            masks[k] = torch.from_numpy(annToMask(obj, [h, w]))
        return masks

    def _decode(self, img_id):
        """(the PIL RGB image of ``img_id``, its target before any transform, the sample's third element)."""
        from PIL import Image
        with Image.open(os.path.join(self.root, self.coco.imgs[img_id]["file_name"])) as f:
            img = f.convert("RGB")
        h, w = img.height, img.width
        visible = [obj for obj in self.coco.anns_of[img_id] if obj["iscrowd"] == 0]
        kept = [obj for obj in visible if obj["area"] != 0]
        first = visible[0] if visible else {}          # the fields of the first non-crowd object decide what a target carries

        xywh = torch.tensor([obj["bbox"] for obj in kept], dtype=torch.float32) if kept else torch.zeros((0, 4))
        labels = torch.tensor([self.json_category_id_to_contiguous_id[obj["category_id"]] for obj in kept], dtype=torch.int64)
        target = {"labels": labels, "boxes": torch.cat([xywh[:, :2], xywh[:, :2] + xywh[:, 2:]], dim=1), "classes": labels}
        if "area" in first:
            target["area"] = torch.tensor([obj["area"] for obj in kept], dtype=torch.float32)
        if "segmentation" in first and self.lazy:
            target["segmentation"], target["size"] = [obj["segmentation"] for obj in kept], (h, w)
        elif "segmentation" in first:
            target["masks"] = self._masks(kept, h, w)
        for field, name, value in _OBJECT_FIELDS:
            if field in first:
                target[name] = torch.tensor([value(obj) for obj in kept], dtype=torch.int64)
        return img, target, first.get("image_id", img_id)

    def __getitem__(self, idx):
        img, target, image_id = self._decode(self.ids[idx])
        sample = (image_bytes(img) if self.lazy else img), target
        if self.transforms is not None:
            sample = self.transforms(*sample)
        return sample[0], sample[1], image_id


def get_dataloader(dataset, batch_size, is_parallel, num_workers=0):
    """The phase-1 loader: street / shop pairs (``DF2MatchingSampler``, incomplete last batch dropped) over a random order of the
    accepted images -- this rank's share of it when ``is_parallel`` -- collated without stacking."""
    order = DistributedSampler(dataset) if is_parallel else RandomSampler(dataset)
    return DataLoader(dataset, batch_sampler=DF2MatchingSampler(dataset, order, batch_size, drop_last=True),
                      collate_fn=collate_fn, num_workers=num_workers)


class RandomSampler(Sampler):
    """The positions ``0 .. len(entries) - 1`` in a fresh random order (torch's global generator) per pass; ``entries`` is
    ``dataset.accepted_entries`` unless given."""

    def __init__(self, dataset, entries=None):
        self.entries = dataset.accepted_entries if entries is None else entries
        if not self.entries:
            raise ValueError("RandomSampler: the dataset has no accepted entries (no match key occurs on both sides)")

    def __len__(self):
        return len(self.entries)

    def __iter__(self):
        return iter(torch.randperm(len(self)).tolist())


def _world(num_replicas, rank):
    """(world size, rank), each taken from the default process group when not given."""
    import torch.distributed as dist
    if (num_replicas is None or rank is None) and not (dist.is_available() and dist.is_initialized()):
        raise RuntimeError("DistributedSampler: no process group is initialised; pass num_replicas and rank")
    return (dist.get_world_size() if num_replicas is None else int(num_replicas)), (dist.get_rank() if rank is None else int(rank))


class DistributedSampler(Sampler):
    """This rank's share of the positions of ``entries`` (``dataset.accepted_entries`` unless given): the permutation seeded with the epoch (``set_epoch``;
    the identity when ``shuffle`` is off) is continued cyclically to a multiple of the world size and cut into one contiguous
    slice of ``len(self)`` positions per rank, so every rank takes the same number of steps."""

    def __init__(self, dataset, num_replicas=None, rank=None, shuffle=True, entries=None):
        self.entries = dataset.accepted_entries if entries is None else entries
        self.world, self.rank = _world(num_replicas, rank)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"DistributedSampler: rank {self.rank} is outside a world of {self.world}")
        self.shuffle, self.epoch = bool(shuffle), 0
        self.per_rank = -(-len(self.entries) // self.world)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __len__(self):
        return self.per_rank

    def __iter__(self):
        n = len(self.entries)
        order = torch.randperm(n, generator=torch.Generator().manual_seed(self.epoch)).tolist() if self.shuffle else list(range(n))
        start = self.rank * self.per_rank
        return iter([order[k % n] for k in range(start, start + self.per_rank)])


class DF2MatchingSampler(Sampler):
    """Batches of dataset positions in street / shop pairs.  For every position the base sampler yields, the accepted image
    there and one partner from the other side -- drawn with ``random.choice`` among all images that share any of its match
    keys -- are appended street first, shop second; a batch is yielded whenever it holds ``batch_size`` positions.  An image
    without a partner is skipped.

    ``drop_last=True`` (the only way ``get_dataloader`` builds it) drops what is left at the end; ``len()`` is then
    ``len(sampler) // (batch_size // 2)``, one pair per base position, as in the reference.  ``drop_last=False``: the remainder
    is yielded once, as a last, shorter batch (the reference's loop would yield every growing partial batch; nothing uses
    that), and ``len()`` is the reference's ``ceil(len(sampler) / batch_size)``."""

    def __init__(self, dataset, sampler, batch_size, drop_last):
        if not isinstance(sampler, Sampler):
            raise ValueError(f"DF2MatchingSampler: sampler must be a torch.utils.data.Sampler, got {type(sampler).__name__}")
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"DF2MatchingSampler: batch_size must be a positive int, got {batch_size!r}")
        if not isinstance(drop_last, bool):
            raise ValueError(f"DF2MatchingSampler: drop_last must be a bool, got {drop_last!r}")
        self.dataset, self.sampler, self.batch_size, self.drop_last = dataset, sampler, batch_size, drop_last

    def _pair(self, img_id):
        """(street id, shop id) for an accepted image and a random partner, or None when the other side has none."""
        ds = self.dataset
        is_street = ds.coco.imgs[img_id]["source"] == STREET
        other = ds.match_map_shop if is_street else ds.match_map_street
        partners = [p for key in _match_keys(ds.coco.imgs[img_id], skip_zero=False) for p in other.get(key, ())]
        if not partners:
            return None
        partner = random.choice(partners)
        return (img_id, partner) if is_street else (partner, img_id)

    def __iter__(self):
        ds, batch = self.dataset, []
        for pos in self.sampler:
            pair = self._pair(ds.accepted_entries[pos])
            if pair is not None:
                batch += [ds.idx_to_id_map[i] for i in pair]
            if len(batch) == self.batch_size:
                yield batch
                batch = []
        if batch and not self.drop_last:
            yield batch

    def __len__(self):
        n = len(self.sampler)
        return n // (self.batch_size // 2) if self.drop_last else -(-n // self.batch_size)
