"""MovingFashion for the phase-3 loops and ``evaluator.evaluate``: ``MovingFashionDataset``, ``MFBatchSampler``,
``get_dataloader`` and ``collate_fn`` -- the names a loop written against the reference's ``datasets/MFDataset.py`` imports --
without cv2 at import time, torchvision or pycocotools.

The annotation file maps a product id to ``{"img_path", "video_paths", "source"[, "tracklets"]}``.  A sample is addressed by
``i`` (the product's shop image) or by ``(i, tag, index[, video_i])``: ``tag == "video"`` is the frame at position ``index`` in
[0, 1) of one of the product's videos (``video_i``, or a ``random.choice``), anything else the shop image.  A batch is
``n_products`` products of one shop image followed by ``batch_size // n_products - 1`` frames each.

Video decode stays on the host, behind ``frame_reader(path)``: an object with ``n_frames`` and ``read(k) -> (success, BGR uint8
[H,W,3] ndarray)``.  The default reader wraps ``cv2.VideoCapture`` (cv2 is imported when the first video is opened) and hands a
path that ends in ``.npy`` to ``NpyFrameReader``: a ``[T,H,W,3]`` BGR stack of pre-extracted frames, memory-mapped.

The reference turns a frame to RGB, adds Gaussian noise in float64 over the full-resolution frame and halves it with PIL, on the
dataloader worker (``MFDataset.py:79-95``).  Two forms:

* ``lazy=False`` -- that arithmetic and its draw order, here: ``random.choice`` of the video (only without ``video_i``), one
  ``random.random()`` for sigma on every frame that was read, ``np.random.randn(*shape)`` only with ``noise=True``, the PIL
  resize, boxes ``[0, 0, w, h]`` and masks of ones.
* ``lazy=True`` -- the same Python ``random`` draws, and the image is the decoded uint8 bytes: the full-resolution BGR frame, the
  RGB shop image, or the 100 x 100 zero placeholder of a frame that could not be read.  The target carries ``"frame_prep"`` (0 as
  it is, 1 BGR -> RGB, 2 BGR -> RGB + noise + half resolution), ``"frame_sigma"`` and, for mode 2, ``"frame_seed"`` (one
  ``np.random.randint(0, 2**63)``); it has no ``"masks"`` and its ``"boxes"`` refer to the final (halved) size.
  ``input_pipeline.prepare_batch`` / ``frames.prepare_frames`` (and ``evaluator.collect_descriptors`` through it) do the frame
  work on the device in one launch (``seam_frames_prepare_batch_u8``).  Python's ``random`` stream is the same in both forms, so a
  seeded run picks the same videos, sigmas and flips either way; NumPy's is not (one integer instead of ``h * w * 3`` normals),
  and the noise values are the device generator's, not NumPy's.
"""
from __future__ import annotations

import json
import os
import random

import numpy as np
import torch
from torch.utils.data import BatchSampler, DataLoader, Dataset, RandomSampler, SequentialSampler
from torch.utils.data.distributed import DistributedSampler

from ..transform import image_bytes

NOISE_STRONG, NOISE_WEAK, NOISE_ABOVE = 0.25, 0.05, 0.75      # sigma of one frame in four, of the others, the draw that decides
FRAME_AS_IS, FRAME_RGB, FRAME_NOISY_HALF = 0, 1, 2            # "frame_prep": the modes of ops.frames_prepare_batch
PLACEHOLDER = (100, 100)                                      # the zero image of an unreadable frame


class Cv2FrameReader:
    """``cv2.VideoCapture`` behind the reader contract; the capture is opened in the process that reads."""

    def __init__(self, path):
        try:
            import cv2
        except ImportError as e:
            raise ImportError("MovingFashionDataset decodes videos with cv2 (opencv-python), which is not installed: install it, "
                              "or pass frame_reader=... (a callable path -> object with n_frames and read(k); NpyFrameReader reads "
                              "pre-extracted [T,H,W,3] BGR stacks)") from e
        self.video = cv2.VideoCapture(path)
        self.n_frames = self.video.get(7)                     # CAP_PROP_FRAME_COUNT, a float as cv2 gives it

    def read(self, k):
        self.video.set(1, k)                                  # CAP_PROP_POS_FRAMES
        return self.video.read()

    def release(self):
        self.video.release()


class NpyFrameReader:
    """Pre-extracted frames: ``path`` is a ``.npy`` file holding a uint8 ``[T,H,W,3]`` BGR stack, opened with ``mmap_mode="r"`` so
    that one frame is read per call.  Pickles as its path."""

    def __init__(self, path):
        self.path = path
        self._stack = None
        self.n_frames = int(self.stack.shape[0])

    @property
    def stack(self):
        if self._stack is None:
            stack = np.load(self.path, mmap_mode="r")
            if stack.dtype != np.uint8 or stack.ndim != 4 or stack.shape[3] != 3:
                raise ValueError(f"{self.path}: expected a uint8 [T,H,W,3] stack, got {stack.dtype} {stack.shape}")
            self._stack = stack
        return self._stack

    def read(self, k):
        if not 0 <= k < self.n_frames:
            return False, None
        return True, np.array(self.stack[k])

    def release(self):
        self._stack = None

    def __getstate__(self):
        return {"path": self.path, "n_frames": self.n_frames}

    def __setstate__(self, state):
        self.path, self.n_frames, self._stack = state["path"], state["n_frames"], None


def open_frames(path):
    """The default ``frame_reader``: ``NpyFrameReader`` for a path ending in ``.npy``, else ``Cv2FrameReader``."""
    return NpyFrameReader(path) if str(path).endswith(".npy") else Cv2FrameReader(path)


class MovingFashionDataset(Dataset):
    """``dataset[i]`` / ``dataset[(i, tag, index[, video_i])] -> (img, target)``; the module's docstring has the forms.  The target:
    ``"paths"``, ``"source"``, ``"tracklet"`` (the annotated box of that frame, ``[-1, -1, -1, -1]`` when the product has
    tracklets but none there, None without tracklets), ``"i"``, ``"video_i"`` (-1 for a shop image), ``"valid"`` and ``"index2"``
    (frames only), ``"index"``, ``"tag"`` (1 shop, 0 frame), ``"labels"``, ``"boxes"`` and, eager, ``"masks"``.

    ``product_ids`` are the sorted keys: all but ``blacklist`` when that is given, else those in ``whitelist``, else all.  The
    tracklet rule is the reference's: without ``video_i`` the table of video 0 is read, whichever video was drawn."""

    def __init__(self, jsonpath, transform=None, noise=True, root="", blacklist=None, whitelist=None, lazy=False, frame_reader=None):
        with open(jsonpath, "r") as fp:
            self.data = json.load(fp)
        if blacklist is not None:
            keep = [k for k in self.data if k not in blacklist]
        elif whitelist is not None:
            keep = [k for k in self.data if k in whitelist]
        else:
            keep = list(self.data)
        self.product_ids = sorted(keep)
        self.product_list = [self.data[k] for k in self.product_ids]
        self.noise, self.transform, self.root = noise, transform, root
        self.lazy = bool(lazy)
        self.frame_reader = open_frames if frame_reader is None else frame_reader

    def __len__(self):
        return len(self.product_list)

    def _frame(self, product, index, video_i, ret):
        """The decoded frame of a video sample (None when it cannot be read); fills the target's video entries."""
        paths = product["video_paths"]
        if video_i is None:
            name = random.choice(paths)
            ret["video_i"] = paths.index(name)
        else:
            ret["video_i"] = video_i
            name = paths[video_i]
        if isinstance(index, int):
            raise ValueError(f"MovingFashionDataset: a frame's index is a position in [0, 1) along the video (a float), got {index!r}")
        reader = self.frame_reader(os.path.join(self.root, name))
        index2 = int(reader.n_frames * index)
        success, frame = reader.read(index2)
        if hasattr(reader, "release"):
            reader.release()
        ret["valid"], ret["index2"] = success, index2
        if "tracklets" in product:
            table = product["tracklets"][0 if video_i is None else video_i]
            box = table.get(str(index2))
            ret["tracklet"] = np.asarray(box if box is not None else [-1, -1, -1, -1])
        return frame if success else None

    def __getitem__(self, x):
        video_i = None
        if isinstance(x, tuple):
            i, tag, index = x[:3]
            if len(x) > 3:
                video_i = x[3]
        else:
            i, tag, index = x, None, None
        product = self.product_list[i]
        ret = {"paths": {"video_paths": product["video_paths"], "img_path": product["img_path"]}, "source": product["source"],
               "tracklet": None, "i": i, "video_i": -1}
        prep = sigma = None
        if tag == "video":
            frame = self._frame(product, index, video_i, ret)
            if frame is None:
                img, prep = np.zeros(PLACEHOLDER + (3,), dtype=np.uint8), FRAME_AS_IS
            else:
                sigma = NOISE_STRONG if random.random() > NOISE_ABOVE else NOISE_WEAK
                prep = FRAME_NOISY_HALF if self.noise else FRAME_RGB
                if self.lazy:
                    img = frame
                else:
                    img = frame[:, :, ::-1]
                    if self.noise:
                        img = img / 255.0
                        img += np.random.randn(*img.shape) * sigma
                        img = img * 255.0
                        img = np.clip(img, 0, 255.0)
                        img = np.asarray(img, dtype=np.uint8)
            if self.lazy:
                img = torch.from_numpy(np.ascontiguousarray(img))
                h, w = (img.shape[0] // 2, img.shape[1] // 2) if prep == FRAME_NOISY_HALF else (img.shape[0], img.shape[1])
            else:
                from PIL import Image
                img = Image.fromarray(np.ascontiguousarray(img))
                if prep == FRAME_NOISY_HALF:
                    img = img.resize((img.size[0] // 2, img.size[1] // 2))
                w, h = img.size
        else:
            from PIL import Image
            img = Image.open(os.path.join(self.root, product["img_path"]))
            w, h = img.size
            if self.lazy:
                img, prep = image_bytes(img), FRAME_AS_IS
        ret["index"] = index
        ret["tag"] = 0 if tag == "video" else 1
        ret["labels"] = torch.tensor([0])
        ret["boxes"] = torch.tensor([[0.0, 0.0, w, h]], dtype=torch.float32)
        if self.lazy:
            ret["frame_prep"], ret["frame_sigma"] = prep, 0.0 if sigma is None else sigma
            if prep == FRAME_NOISY_HALF:
                ret["frame_seed"] = int(np.random.randint(0, 2 ** 63))
        else:
            ret["masks"] = torch.ones(1, h, w, dtype=torch.uint8)
        if self.transform is not None:
            img, ret = self.transform(img, ret)
        return img, ret


def collate_fn(batch):
    """A list of ``(image, target)`` samples -> ``(images, targets)`` tuples: images of different sizes are never stacked."""
    return tuple(zip(*batch))


class MFBatchSampler(BatchSampler):
    """Batches of ``(i, "in", None)`` followed by ``(i, "video", t[, fixed_video_i])`` entries.  For every position ``i`` of the
    base sampler (``fixed_ind`` in its place when given) the frame positions ``t`` are: ``batch_size == 1`` -- the first
    ``n_samples`` of ``linspace(0, 1, n_samples + 1)``; ``uniform_sampling`` -- ``linspace(0, 1, k)``; ``fixed_frame`` a list --
    its values, a number -- ``k`` copies; otherwise ``k`` sorted ``random.random()`` draws, ``k = batch_size // n_products - 1``.
    Only the first ``first_n_withvideo`` products get frames when that is set.  A batch is yielded when it holds ``batch_size``
    entries, or after every product when ``batch_size == 1`` or ``first_n_withvideo`` is set; ``drop_last=False`` also yields what
    is left at the end (possibly empty).  ``len()``: ``len(sampler) // n_products``, plus 1 without ``drop_last``."""

    def __init__(self, dataset, sampler, batch_size, drop_last, n_samples=100, n_products=1, first_n_withvideo=None,
                 uniform_sampling=False, fixed_frame=None, fixed_ind=None, fixed_video_i=None):
        super().__init__(sampler, batch_size, drop_last)
        self.data, self.n_video_samples, self.n_products = dataset, n_samples, n_products
        self.first_n_withvideo, self.uniform_sampling, self.fixed_frame = first_n_withvideo, uniform_sampling, fixed_frame
        self.fixed_ind, self.fixed_video_i = fixed_ind, fixed_video_i

    def _positions(self):
        k = self.batch_size // self.n_products - 1
        if self.batch_size == 1:
            return list(np.linspace(0.0, 1.0, self.n_video_samples + 1))[:-1]
        if self.uniform_sampling:
            return list(np.linspace(0.0, 1.0, k))
        if self.fixed_frame is None:
            return sorted(random.random() for _ in range(k))
        if isinstance(self.fixed_frame, list):
            return list(self.fixed_frame)
        return [self.fixed_frame] * k

    def __iter__(self):
        batch = []
        for count, idx in enumerate(self.sampler):
            if self.fixed_ind is not None:
                idx = self.fixed_ind
            batch.append((idx, "in", None))
            positions = self._positions()
            if self.first_n_withvideo is None or count < self.first_n_withvideo:
                tail = () if self.fixed_video_i is None else (self.fixed_video_i,)
                batch.extend((idx, "video", t) + tail for t in positions)
            if self.batch_size == 1 or len(batch) == self.batch_size or self.first_n_withvideo is not None:
                yield batch
                batch = []
        if not self.drop_last:
            yield batch

    def __len__(self):
        n = len(self.sampler) // self.n_products
        return n if self.drop_last else n + 1


def get_dataloader(dataset, batch_size, is_parallel, n_products=1, first_n_withvideo=None, uniform_sampling=False, fixed_frame=None,
                   is_seq=False, num_workers=8, fixed_ind=None, fixed_video_i=None):
    """The phase-3 loader: ``MFBatchSampler`` (``drop_last=True``) over this rank's share of a shuffled order when
    ``is_parallel``, the dataset's own order when ``is_seq``, else a random order; collated without stacking."""
    if is_parallel:
        order = DistributedSampler(dataset, shuffle=True)
    elif is_seq:
        order = SequentialSampler(dataset)
    else:
        order = RandomSampler(dataset)
    batches = MFBatchSampler(dataset, order, batch_size, drop_last=True, n_products=n_products, first_n_withvideo=first_n_withvideo,
                             uniform_sampling=uniform_sampling, fixed_frame=fixed_frame, fixed_ind=fixed_ind,
                             fixed_video_i=fixed_video_i)
    return DataLoader(dataset, num_workers=num_workers, batch_sampler=batches, collate_fn=collate_fn)
