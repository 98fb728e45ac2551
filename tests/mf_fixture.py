"""A tiny MovingFashion tree for the dataset tests: an annotation JSON, PNG shop images and ``.npy`` frame stacks (uint8
``[T,H,W,3]`` BGR, what ``datasets.MFDataset.NpyFrameReader`` opens) written into a directory, plus the sampler cases shared by
tests/test_mfdataset_host.py and tests/golden/make_mf_sampler_golden.py and a plain restatement of the reference sampler's
``__iter__`` (ref datasets/MFDataset.py:151-186)."""
import json
import os
import random

import numpy as np

FRAMES = 5                                                    # frames per stack
# product id -> (shop image (h, w), the (h, w) of its two videos, source, has tracklets); ids are written unsorted
PRODUCTS = {"p2": ((25, 25), [(24, 30), (9, 7)], 1, False),
            "p0": ((31, 45), [(37, 53), (24, 30)], 1, True),
            "p1": ((40, 28), [(3, 2), (37, 53)], 0, True)}


def stack_of(pid, v, products=None):
    h, w = (products or PRODUCTS)[pid][1][v]
    return np.random.RandomState(100 * int(pid[1:]) + v).randint(0, 256, (FRAMES, h, w, 3)).astype(np.uint8)


def shop_of(pid, products=None):
    h, w = (products or PRODUCTS)[pid][0]
    return np.random.RandomState(7 + int(pid[1:])).randint(0, 256, (h, w, 3)).astype(np.uint8)


def tracklets_of(pid):
    """Per video: boxes for the even frames only, so that an odd frame has none."""
    k = int(pid[1:])
    return [{str(f): [k + v, f, 10 + k + v, 12 + f] for f in range(0, FRAMES, 2)} for v in range(2)]


def write(root, products=None):
    """Writes the tree of ``products`` (default: ``PRODUCTS``) under ``root`` -> the annotation file's path."""
    products = products or PRODUCTS
    from PIL import Image
    os.makedirs(os.path.join(root, "shop"))
    os.makedirs(os.path.join(root, "vid"))
    data = {}
    for pid, (_, videos, source, tracked) in products.items():
        Image.fromarray(shop_of(pid, products)).save(os.path.join(root, "shop", pid + ".png"))
        names = []
        for v in range(len(videos)):
            names.append(f"vid/{pid}_{v}.npy")
            np.save(os.path.join(root, names[-1]), stack_of(pid, v, products))
        data[pid] = {"img_path": f"shop/{pid}.png", "video_paths": names, "source": source}
        if tracked:
            data[pid]["tracklets"] = tracklets_of(pid)
    path = os.path.join(root, "mf.json")
    with open(path, "w") as fp:
        json.dump(data, fp)
    return path


# name -> (positions of the base sampler, batch_size, drop_last, keyword arguments, random seed)
SAMPLER_CASES = {
    "default": (5, 4, True, {}, 1),
    "n_products_2": (5, 8, True, {"n_products": 2}, 2),
    "uniform_sampling": (4, 4, True, {"uniform_sampling": True}, 3),
    "fixed_frame_float": (4, 3, True, {"fixed_frame": 0.5}, 4),
    "fixed_frame_list": (4, 4, True, {"fixed_frame": [0.1, 0.6, 0.9]}, 5),
    "first_n_withvideo": (5, 4, True, {"first_n_withvideo": 2}, 6),
    "fixed_video_i": (3, 4, True, {"fixed_video_i": 1}, 7),
    "fixed_ind": (3, 3, True, {"fixed_ind": 1}, 8),
    "batch_size_1": (3, 1, True, {"n_samples": 6}, 9),
    "keep_last": (5, 8, False, {"n_products": 2}, 10),
}


def reference_batches(positions, batch_size, drop_last, n_samples=100, n_products=1, first_n_withvideo=None, uniform_sampling=False,
                      fixed_frame=None, fixed_ind=None, fixed_video_i=None):
    """What the reference's ``MFBatchSampler.__iter__`` yields over the base positions, statement for statement."""
    out, batch, count = [], [], -1
    for idx in positions:
        if fixed_ind is not None:
            idx = fixed_ind
        batch.append((idx, "in", None))
        count += 1
        if batch_size == 1:
            samples = [x for x in np.linspace(0.0, 1.0, n_samples + 1)][:-1]
        elif not uniform_sampling:
            if fixed_frame is None:
                samples = sorted([random.random() for _ in range((batch_size // n_products) - 1)])
            elif isinstance(fixed_frame, list):
                samples = [x for x in fixed_frame]
            else:
                samples = [fixed_frame for _ in range((batch_size // n_products) - 1)]
        else:
            samples = [x for x in np.linspace(0.00, 1.0, (batch_size // n_products) - 1)]
        if first_n_withvideo is None or count < first_n_withvideo:
            for t in samples:
                batch.append((idx, "video", t) if fixed_video_i is None else (idx, "video", t, fixed_video_i))
        if batch_size == 1 or len(batch) == batch_size or first_n_withvideo is not None:
            out.append(batch)
            batch = []
    if not drop_last:
        out.append(batch)
    return out


def as_json(batches):
    """Batches as JSON holds them: lists, floats as Python floats."""
    return [[[e[0], e[1], None if e[2] is None else float(e[2])] + [int(v) for v in e[3:]] for e in b] for b in batches]
