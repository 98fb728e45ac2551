"""A hand-made DeepFashion2 annotation file with its images, written into a directory: the fixture of
tests/test_df2_dataset_host.py and tests/test_gpu_train_input_model.py.  Every expected value of those tests is worked out
by hand from the tables below.

Images (id: source, match_desc, (h, w)) -- listed out of order in the file:
  1 street {"1": 101}            2 street {"1": 101}     3 shop {"1": 101}     product 101: two street images, one shop image
  4 street {"2": 202}            no shop partner
  5 shop   {"1": 303, "0": 999}  6 street {"0": 999, "1": 303}                 the style-'0' entries are skipped
  7 shop   {"3": 404}            no street partner
  8 street {"0": 555}            style '0' only
Categories in file order: ids 3, 1, 13 -> labels 1, 2, 3.
Image 1 carries four objects: a kept one, an iscrowd one, an area == 0 one and a second kept one (two polygon parts).
"""
import json
import os

import numpy as np

SIZES = {1: (40, 56), 2: (37, 53), 3: (48, 40), 4: (33, 47), 5: (44, 60), 6: (50, 51), 7: (36, 36), 8: (35, 41)}
SOURCE = {1: "user", 2: "user", 3: "shop", 4: "user", 5: "shop", 6: "user", 7: "shop", 8: "user"}
MATCH = {1: {"1": 101}, 2: {"1": 101}, 3: {"1": 101}, 4: {"2": 202}, 5: {"1": 303, "0": 999}, 6: {"0": 999, "1": 303},
         7: {"3": 404}, 8: {"0": 555}}
CATEGORIES = [{"id": 3, "name": "short sleeve top"}, {"id": 1, "name": "trousers"}, {"id": 13, "name": "sling dress"}]
FILE_ORDER = [5, 1, 8, 3, 2, 7, 4, 6]


def _ann(aid, img, cat, bbox, area, segm, pair, style, iscrowd=0):
    return {"id": aid, "image_id": img, "category_id": cat, "bbox": bbox, "area": area, "segmentation": segm, "pair_id": pair,
            "style": style, "source": SOURCE[img], "iscrowd": iscrowd}


def _box_poly(x, y, w, h):
    return [[x, y, x + w, y, x + w, y + h, x, y + h]]


ANNOTATIONS = [
    _ann(10, 1, 13, [4.0, 5.0, 20.0, 24.0], 480.0, _box_poly(4.0, 5.0, 20.0, 24.0), 101, 1),
    _ann(11, 1, 3, [1.0, 1.0, 8.0, 8.0], 64.0, _box_poly(1.0, 1.0, 8.0, 8.0), 101, 0, iscrowd=1),
    _ann(12, 1, 1, [30.0, 2.0, 5.0, 5.0], 0, _box_poly(30.0, 2.0, 5.0, 5.0), 101, 0),
    _ann(13, 1, 1, [28.0, 10.0, 22.5, 25.0], 310.5, [[28.0, 10.0, 40.0, 10.0, 40.0, 22.0, 28.0, 22.0],
                                                      [38.5, 20.0, 50.5, 20.0, 50.5, 35.0, 38.5, 35.0]], 101, 0),
    _ann(20, 2, 13, [3.0, 2.0, 30.0, 31.0], 930.0, _box_poly(3.0, 2.0, 30.0, 31.0), 101, 1),
    _ann(30, 3, 13, [5.0, 6.0, 28.0, 36.0], 700.0, [[5.0, 6.0, 33.0, 6.0, 19.0, 42.0]], 101, 1),
    _ann(40, 4, 3, [6.0, 4.0, 25.0, 20.0], 500.0, _box_poly(6.0, 4.0, 25.0, 20.0), 202, 2),
    _ann(50, 5, 1, [10.0, 8.0, 35.0, 30.0], 1050.0, _box_poly(10.0, 8.0, 35.0, 30.0), 303, 1),
    _ann(60, 6, 1, [7.0, 9.0, 33.0, 32.0], 1056.0, _box_poly(7.0, 9.0, 33.0, 32.0), 303, 1),
    _ann(70, 7, 3, [2.0, 2.0, 30.0, 30.0], 900.0, _box_poly(2.0, 2.0, 30.0, 30.0), 404, 3),
    _ann(80, 8, 3, [3.0, 3.0, 20.0, 20.0], 400.0, _box_poly(3.0, 3.0, 20.0, 20.0), 555, 0),
]


def pixels(img_id):
    h, w = SIZES[img_id]
    return np.random.RandomState(100 + img_id).randint(0, 256, (h, w, 3)).astype(np.uint8)


def write(root):
    """Writes <root>/images/<id>.png and <root>/ann.json; returns (ann_file, image root)."""
    from PIL import Image
    img_root = os.path.join(str(root), "images")
    os.makedirs(img_root, exist_ok=True)
    images = []
    for i in FILE_ORDER:
        Image.fromarray(pixels(i)).save(os.path.join(img_root, f"{i}.png"))
        images.append({"id": i, "file_name": f"{i}.png", "height": SIZES[i][0], "width": SIZES[i][1], "source": SOURCE[i],
                       "match_desc": MATCH[i]})
    ann_file = os.path.join(str(root), "ann.json")
    with open(ann_file, "w") as f:
        json.dump({"images": images, "annotations": ANNOTATIONS, "categories": CATEGORIES}, f)
    return ann_file, img_root
