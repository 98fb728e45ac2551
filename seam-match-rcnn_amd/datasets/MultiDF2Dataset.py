"""Multi-DeepFashion2 for the phase-2 loops and ``evaluator_df2.evaluate``: ``MultiDeepFashion2Dataset``,
``MultiDF2BatchSampler`` and ``get_dataloader`` -- the names a loop written against the reference's
``datasets/MultiDF2Dataset.py`` imports -- on top of ``DF2Dataset.DeepFashion2Dataset`` (the annotation index, the match maps and
the target are its), without torchvision, pycocotools or ``torch._six``.

A sample is addressed by ``(key, tag, index)``: a product (match key ``"<style>_<pair_id>"``), its shop side or its street side,
and for the street side a position in [0, 1) along the product's street images.  A batch is ``n_products`` products of one shop
image followed by ``batch_size // n_products - 1`` street images each.

The reference adds Gaussian noise to one image in four on the host, in float64 (``MultiDF2Dataset.py:157-167``).  Two forms:

* ``lazy=False`` -- that arithmetic and its draw order, here: one ``random.random()`` for sigma (only with ``noise=True``), then
  ``np.random.randn(*shape)`` always, then ``/ 255.0``, ``+ n * sigma``, ``* 255.0``, clip, uint8.  (``v / 255.0 * 255.0`` truncates
  back to ``v`` for all 256 byte values, so the arithmetic is skipped for sigma 0; the draws are not.)
* ``lazy=True`` -- the image stays the decoded uint8 ``[H,W,3]`` bytes; the same ``random.random()`` decides sigma and the target
  carries ``"noise_sigma"`` (a float) and, when sigma > 0, ``"noise_seed"`` (one ``np.random.randint(0, 2**63)``).
  ``input_pipeline.prepare_batch`` / ``apply_noise`` (and ``evaluator_df2.evaluate`` through it) add the noise on the device from
  counter-based draws keyed by that seed (``seam_noise_u8_batch``).  Python's ``random`` stream is the same in both forms, so a
  seeded run picks the same shop images, sigmas and flips either way; NumPy's is not (one integer instead of ``h * w * 3``
  normals), and the noise values are the device generator's, not NumPy's.  As in phase 1 the target carries ``"segmentation"``
  and ``"size"`` in place of ``"masks"``.
"""
from __future__ import annotations

import random

import numpy as np
from torch.utils.data import DataLoader, Sampler

from ..transform import image_bytes
from ..utils import collate_fn
from .DF2Dataset import DeepFashion2Dataset, DistributedSampler, RandomSampler

NOISE_SIGMA, NOISE_ABOVE = 0.1, 0.75        # sigma of a noisy image; the draw above which an image is noisy (one in four)


def pair_keys(dataset) -> list:
    """The match keys present on both sides, sorted."""
    return sorted(dataset.match_map_street.keys() & dataset.match_map_shop.keys())


class MultiDeepFashion2Dataset(DeepFashion2Dataset):
    """``dataset[(key, tag, index)] -> (img, target, image_id)``.  ``tag == "shop"``: one of the key's shop images
    (``random.choice``); otherwise street image number ``int(len(street images of the key) * index)``.  The target is
    ``DeepFashion2Dataset``'s for that image plus ``"i"`` (the key) and ``"tag"`` (1 shop, 0 street), set after the transforms as in
    the reference; ``image_id`` as there (the image's own id when every object is a crowd, where the reference raises).

    ``len()`` is the number of street match keys.  ``filter_onestreet`` keeps the street keys that also occur on the shop side and
    have at least two street images, then the shop keys that survive on the street side.  ``noise`` / ``lazy``: the module's
    docstring.  Without transforms the eager form returns a PIL image (as the reference) and the lazy form the bytes."""

    def __init__(self, ann_file, root, transforms=None, noise: bool = False, filter_onestreet: bool = False, lazy: bool = False):
        super().__init__(ann_file, root, transforms, lazy)
        self.noise = bool(noise)
        if filter_onestreet:
            self.match_map_street = {k: v for k, v in self.match_map_street.items() if k in self.match_map_shop and len(v) >= 2}
            self.match_map_shop = {k: v for k, v in self.match_map_shop.items() if k in self.match_map_street}

    def __len__(self):
        return len(self.match_map_street)

    def __getitem__(self, x):
        key, tag, index = x
        if tag == "shop":
            img_id = random.choice(self.match_map_shop[key])
        else:
            street = self.match_map_street[key]
            img_id = street[int(len(street) * index)]
        img, target, image_id = self._decode(img_id)
        sigma = NOISE_SIGMA if self.noise and random.random() > NOISE_ABOVE else 0.0
        if self.lazy:
            img = image_bytes(img)
            target["noise_sigma"] = sigma
            if sigma > 0:
                target["noise_seed"] = int(np.random.randint(0, 2 ** 63))
        else:
            image = np.array(img)
            draws = np.random.randn(*image.shape)
            if sigma > 0:
                from PIL import Image
                image = image / 255.0
                image += draws * sigma
                image = image * 255.0
                image = np.clip(image, 0, 255.0)
                img = Image.fromarray(np.asarray(image, dtype=np.uint8))
        if self.transforms is not None:
            img, target = self.transforms(img, target)
        target["i"] = key
        target["tag"] = 1 if tag == "shop" else 0
        return img, target, image_id


class MultiDF2BatchSampler(Sampler):
    """Batches of ``(key, tag, index)`` entries.  For every position ``p`` the base sampler yields: ``(pair_keys[p], "shop", None)``
    followed by ``batch_size // n_products - 1`` entries ``(pair_keys[p], "street", t)``, the ``t`` being sorted
    ``random.random()`` draws; a batch is yielded whenever it holds ``batch_size`` entries.  ``drop_last=False`` also yields what
    is left at the end (possibly empty), and ``len()`` is the reference's: ``len(sampler) // n_products``, plus 1 without
    ``drop_last``.

    Two deliberate departures from the reference:

    * ``pair_keys`` is the sorted list of the keys present on both sides.  The reference takes ``list(set(...))``, whose order
      changes with the interpreter's hash seed, so that a seeded run does not repeat from one process to the next.
    * the base sampler is expected to draw positions over ``len(pair_keys)`` (``get_dataloader`` builds it so).  The reference
      draws over ``len(dataset)`` -- the street keys -- and indexes ``pair_keys`` with them, which overruns when a street key
      has no shop image.

    ``n_products`` must be at least 1 and divide ``batch_size`` (the reference's default of 0 divides by zero)."""

    def __init__(self, dataset, sampler, batch_size, drop_last, n_products=0):
        if not isinstance(sampler, Sampler):
            raise ValueError(f"MultiDF2BatchSampler: sampler must be a torch.utils.data.Sampler, got {type(sampler).__name__}")
        if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
            raise ValueError(f"MultiDF2BatchSampler: batch_size must be a positive int, got {batch_size!r}")
        if not isinstance(drop_last, bool):
            raise ValueError(f"MultiDF2BatchSampler: drop_last must be a bool, got {drop_last!r}")
        if isinstance(n_products, bool) or not isinstance(n_products, int) or n_products < 1 or batch_size % n_products:
            raise ValueError(f"MultiDF2BatchSampler: n_products must be a positive int that divides batch_size {batch_size}, "
                             f"got {n_products!r}")
        self.data, self.sampler, self.batch_size, self.drop_last, self.n_products = dataset, sampler, batch_size, drop_last, n_products
        self.pair_keys = pair_keys(dataset)

    def __iter__(self):
        batch = []
        for pos in self.sampler:
            key = self.pair_keys[pos]
            batch.append((key, "shop", None))
            for t in sorted(random.random() for _ in range(self.batch_size // self.n_products - 1)):
                batch.append((key, "street", t))
            if len(batch) == self.batch_size:
                yield batch
                batch = []
        if not self.drop_last:
            yield batch

    def __len__(self):
        n = len(self.sampler) // self.n_products
        return n if self.drop_last else n + 1


def get_dataloader(dataset, batch_size, is_parallel, n_products=0, n_workers=0):
    """The phase-2 loader: ``MultiDF2BatchSampler`` (incomplete last batch dropped) over a random order of the products --
    this rank's share of it when ``is_parallel`` -- collated without stacking."""
    keys = pair_keys(dataset)
    order = DistributedSampler(dataset, entries=keys) if is_parallel else RandomSampler(dataset, entries=keys)
    return DataLoader(dataset, batch_sampler=MultiDF2BatchSampler(dataset, order, batch_size, drop_last=True, n_products=n_products),
                      collate_fn=collate_fn, num_workers=n_workers)
