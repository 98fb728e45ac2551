"""CPU: the COCO-style detection protocol of ``evaluator_det`` (bbox only: box IoU is host float64, no device is touched)
against hand-checked known answers and against the float64 restatement of tests/det_eval_refs.py.

Tolerance 1e-12 (absolute) everywhere: the twelve numbers are means of at most 1010 float64 values in [0, 1]; the evaluator
and the restatement make the same decisions on the same IoUs, so only the order of a summation can differ (1010 * 2^-53 is
about 1e-13).  Every scene keeps its IoUs out of rounding's reach of the thresholds (asserted below)."""
import numpy as np
import pytest
import torch

import det_eval_refs as R
from seam_match_rcnn_amd import evaluator_det as E

TOL = 1e-12

IMG_A = lambda: R.image([[10, 10, 40, 40], [100, 100, 50, 50]], [1, 1],
                        [[200, 200, 40, 40], [10, 10, 40, 40], [100, 100, 50, 42]], [1, 1, 1], [0.9, 0.8, 0.7], gt_area=[1600, 2500])
IMG_B1 = lambda: R.image([[0, 0, 20, 20], [30, 30, 100, 100]], [1, 2], [[0, 0, 20, 20], [30, 30, 100, 100]], [1, 2], [0.9, 0.6],
                         gt_area=[400, 10000])
IMG_B2 = lambda: R.image([[5, 5, 50, 50]], [1], [[5, 5, 50, 50]], [1], [0.5], gt_area=[2500])
IMG_C2 = lambda: R.image([[0, 0, 64, 64]], [2], [[0, 0, 64, 64], [0, 0, 64, 60], [0, 0, 64, 64]], [1, 2, 2], [0.95, 0.85, 0.3],
                         gt_area=[4096])
IMG_E = lambda: R.image([[0, 0, 20, 20], [50, 50, 60, 60], [200, 200, 100, 100]], [3, 3, 3],
                        [[50, 50, 60, 60], [200, 200, 100, 72], [400, 400, 10, 10]], [3, 3, 3], [0.9, 0.8, 0.7],
                        gt_area=[400, 3600, 10000])
IMG_F = lambda: R.image([[0, 0, 50, 50], [100, 100, 200, 200]], [1, 1],
                        [[0, 0, 50, 50], [120, 120, 40, 40], [150, 150, 40, 40], [400, 0, 40, 40]], [1, 1, 1, 1],
                        [0.9, 0.8, 0.7, 0.6], gt_area=[2500, 40000], gt_crowd=[0, 1])


def _no_dets(img):
    return dict(img, det_boxes=np.zeros((0, 4), np.float32), det_labels=np.zeros(0, np.int64), det_scores=np.zeros(0, np.float32))


AP_A = 0.5424092409240924
AP_C = 0.6752475247524753
KNOWN = {
    "A": ([IMG_A()], [AP_A, 2 / 3, 2 / 3, -1, AP_A, -1, 0, 0.85, 0.85, -1, 0.85, -1]),
    "B": ([IMG_B1(), IMG_B2()], [1] * 12),
    "C": ([IMG_A(), IMG_C2()], [AP_C, 0.75, 0.75, -1, AP_C, -1, 0.45, 0.925, 0.925, -1, 0.925, -1]),
    "D": ([_no_dets(IMG_A())], [0, 0, 0, -1, 0, -1, 0, 0, 0, -1, 0, -1]),
    "E": ([IMG_E()], [0.5, 67 / 101, 34 / 101, 0, 1, 0.5, 1 / 3, 0.5, 0.5, 0, 1, 0.5]),
    "F": ([IMG_F()], [1, 1, 1, -1, 1, -1, 1, 1, 1, -1, 1, -1]),
}


def run(scene, max_dets=(1, 10, 100), batches=None, verbose=False):
    ev = E.DetectionEvaluator(iou_types=("bbox",), max_dets=max_dets)
    outs, tgts = R.to_io(scene, torch)
    for lo, hi in (batches or [(0, len(scene))]):
        ev.update(outs[lo:hi], tgts[lo:hi])
    return ev.summarize(verbose=verbose)["bbox"], ev


@pytest.mark.parametrize("case", sorted(KNOWN))
def test_known_answers(case):
    scene, want = KNOWN[case]
    got, _ = run(scene)
    R.assert_same_stats(got, want, TOL, f"case {case}")
    R.assert_same_stats(R.evaluate(scene, "bbox")["stats"], want, TOL, f"restatement, case {case}")


SEEDS = (1, 2, 3, 4, 5, 6)


@pytest.fixture(scope="module")
def scenes():
    out = {s: R.random_scene(s, n_images=5) for s in SEEDS}
    for s, scene in out.items():
        assert R.min_threshold_margin(scene) > 1e-6, f"seed {s}: an IoU sits on a threshold; pick another seed"
        scores = np.concatenate([img["det_scores"] for img in scene])
        assert len(set(scores.tolist())) == len(scores)
    assert sum(len(img["det_labels"]) for sc in out.values() for img in sc) > 60
    assert any(img.get("gt_crowd", np.zeros(1)).any() for sc in out.values() for img in sc)
    return out


@pytest.fixture(scope="module")
def scene_refs(scenes):
    return {s: R.evaluate(scene, "bbox") for s, scene in scenes.items()}


@pytest.mark.parametrize("seed", SEEDS)
def test_random_scenes_agree_with_the_restatement(scenes, scene_refs, seed):
    got, ev = run(scenes[seed])
    ref = scene_refs[seed]
    R.assert_same_stats(got, ref["stats"], TOL, f"seed {seed}")
    assert ev.categories == ref["categories"]
    assert ev.precision["bbox"].shape == ref["precision"].shape == (10, 101, len(ref["categories"]), 4, 3)
    assert ev.recall["bbox"].shape == ref["recall"].shape == (10, len(ref["categories"]), 4, 3)
    assert np.abs(ev.precision["bbox"] - ref["precision"]).max() <= TOL
    assert np.abs(ev.recall["bbox"] - ref["recall"]).max() <= TOL
    assert any(v not in (-1.0, 0.0, 1.0) for v in got)              # the scene decides something


@pytest.mark.parametrize("seed", SEEDS[:3])
def test_order_inside_an_image_and_batch_split_do_not_matter(scenes, scene_refs, seed):
    scene = scenes[seed]
    rng = np.random.RandomState(100 + seed)
    shuffled = []
    for img in scene:
        p = rng.permutation(len(img["det_labels"]))
        shuffled.append(dict(img, det_boxes=img["det_boxes"][p], det_labels=img["det_labels"][p], det_scores=img["det_scores"][p]))
    want = scene_refs[seed]["stats"]
    R.assert_same_stats(run(shuffled)[0], want, TOL, "shuffled detections")
    R.assert_same_stats(run(scene, batches=[(i, i + 1) for i in range(len(scene))])[0], want, TOL, "one image per update")
    R.assert_same_stats(run(scene, batches=[(0, 2), (2, 2), (2, len(scene))])[0], want, TOL, "uneven updates")


def test_detections_of_a_label_without_ground_truth_change_nothing(scenes, scene_refs):
    scene = scenes[2]
    extra = []
    for img in scene:
        boxes = np.concatenate([img["det_boxes"], R.xyxy([[0, 0, 500, 500], [3, 3, 30, 30]])])
        extra.append(dict(img, det_boxes=boxes, det_labels=np.concatenate([img["det_labels"], [0, 99]]),
                          det_scores=np.concatenate([img["det_scores"], np.float32([0.99999, 0.999999])])))
    got, ev = run(extra)
    assert got == run(scene)[0]
    assert 0 not in ev.categories and 99 not in ev.categories
    R.assert_same_stats(got, scene_refs[2]["stats"], TOL)


def test_max_dets_truncation_is_per_image():
    # image 1: a hit at 0.9 and two strays; image 2: a hit at 0.5, below everything in image 1.  One detection PER IMAGE keeps
    # both hits (AR = 1); one detection of the whole run would keep image 1's only (AR = 0.5).
    one = R.image([[10, 10, 40, 40]], [1], [[10, 10, 40, 40], [200, 200, 40, 40], [300, 300, 40, 40]], [1, 1, 1], [0.9, 0.8, 0.7])
    two = R.image([[20, 20, 50, 50]], [1], [[20, 20, 50, 50], [300, 300, 40, 40]], [1, 1], [0.5, 0.4])
    got, _ = run([one, two], max_dets=(1, 2, 3))
    assert got[6] == 1.0
    R.assert_same_stats(got, R.evaluate([one, two], "bbox", max_dets=(1, 2, 3))["stats"], TOL)
    # and the cut at the largest entry: with (1, 1, 2) the third detection of image 1 is never seen
    R.assert_same_stats(run([one, two], max_dets=(1, 1, 2))[0], R.evaluate([one, two], "bbox", max_dets=(1, 1, 2))["stats"], TOL)
    swapped = dict(one, det_scores=np.float32([0.7, 0.8, 0.9]))        # the hit is now third in its image
    got, _ = run([swapped, two], max_dets=(1, 2, 3))
    assert got[6] == 0.5 and got[7] == 0.5 and got[8] == 1.0


def test_the_comparator_rejects_planted_errors(scene_refs):
    scene, want = KNOWN["A"]
    got, _ = run(scene)
    R.assert_same_stats(got, want, TOL)
    # a swapped match: the stray and the exact hit trade scores, so the hit is ranked first
    img = scene[0]
    swapped = [dict(img, det_scores=np.float32([0.8, 0.9, 0.7]))]
    with pytest.raises(AssertionError):
        R.assert_same_stats(got, R.evaluate(swapped, "bbox")["stats"], TOL)
    # an off-by-one recall index: every precision read one recall threshold too late
    ref = scene_refs[1]
    p = ref["precision"]
    shifted = np.concatenate([p[:, 1:], np.where(p[:, -1:] > -1, 0.0, -1.0)], axis=1)
    R.assert_same_stats(R.summarize(ref["precision"], ref["recall"]), ref["stats"], 0.0)
    with pytest.raises(AssertionError):
        R.assert_same_stats(ref["stats"], R.summarize(shifted, ref["recall"]), TOL)
    # one count: a single precision cell moved by one detection in a thousand
    nudged = ref["precision"].copy()
    nudged[nudged > 0] -= 1e-9
    with pytest.raises(AssertionError):
        R.assert_same_stats(ref["stats"], R.summarize(nudged, ref["recall"]), TOL)
    with pytest.raises(AssertionError):
        R.assert_same_stats(got[:11], want, TOL)


def test_crowd_and_area_rules():
    # F without the crowd flag: the two detections inside the big box become false positives of an ordinary ground truth
    scene, _ = KNOWN["F"]
    plain = [dict(scene[0], gt_crowd=np.int64([0, 0]))]
    got, _ = run(plain)
    R.assert_same_stats(got, R.evaluate(plain, "bbox")["stats"], TOL)
    assert got[0] < 1.0
    # area defaults to the box's w*h when the targets carry none
    bare = [{k: v for k, v in IMG_E().items() if k != "gt_area"}]
    R.assert_same_stats(run(bare)[0], KNOWN["E"][1], TOL)


def test_empty_run_and_bad_arguments():
    got, ev = run([])
    assert got == [-1.0] * 12 and ev.categories == []
    with pytest.raises(ValueError):
        E.DetectionEvaluator(iou_types=("keypoints",))
    with pytest.raises(ValueError):
        E.DetectionEvaluator(max_dets=(10, 1, 100))
    ev = E.DetectionEvaluator(iou_types=("bbox",))
    with pytest.raises(ValueError):
        ev.update([], [dict(boxes=torch.zeros(0, 4), labels=torch.zeros(0, dtype=torch.int64))])


class _Stub:
    """Stands in for the model: hands back planted detections, records how it was called."""
    paste_masks = True

    def __init__(self, outputs):
        self.outputs, self.seen, self.modes, self.evals = list(outputs), 0, [], 0

    def eval(self):
        self.evals += 1
        return self

    def __call__(self, images):
        assert not torch.is_grad_enabled()
        self.modes.append(self.paste_masks)
        out = self.outputs[self.seen:self.seen + len(images)]
        self.seen += len(images)
        return out


def test_evaluate_drives_the_loader_and_restores_the_switch(scenes, scene_refs, capsys):
    scene = scenes[3]
    outs, tgts = R.to_io(scene, torch)
    imgs = [torch.zeros(3, 8, 8) for _ in scene]
    loader = [(imgs[:2], tgts[:2]), (imgs[2:], tgts[2:], list(range(2, len(scene))))]          # with and without ids
    model = _Stub(outs)
    stats, ev = E.evaluate(model, loader, torch.device("cpu"), iou_types=("bbox",), verbose=True, return_report=True)
    R.assert_same_stats(stats["bbox"], scene_refs[3]["stats"], TOL)
    assert list(stats) == ["bbox"] and isinstance(ev, E.DetectionEvaluator)
    assert model.modes == [False, False] and model.evals == 1
    assert model.paste_masks is True and "paste_masks" not in vars(model)               # the class default is back
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == "IoU metric: bbox" and len(lines) == 13
    assert lines[1] == f" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=100 ] = {stats['bbox'][0]:0.3f}"
    assert lines[2].startswith(" Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=100 ] = ")
    assert lines[7].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=  1 ] = ")
    assert lines[12].startswith(" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets=100 ] = ")

    def broken():
        yield loader[0]
        raise RuntimeError("loader broke")
    model = _Stub(outs)
    model.paste_masks = True                                                             # an instance setting survives too
    with pytest.raises(RuntimeError, match="loader broke"):
        E.evaluate(model, broken(), torch.device("cpu"), iou_types=("bbox",), verbose=False)
    assert vars(model)["paste_masks"] is True
    assert E.evaluate(_Stub(outs), loader, torch.device("cpu"), iou_types=("bbox",), verbose=False)["bbox"] == stats["bbox"]


def test_model_switch_is_a_class_attribute():
    from seam_match_rcnn_amd.models.matchrcnn import MatchRCNN
    from seam_match_rcnn_amd.models.video_matchrcnn import VideoMatchRCNN
    assert VideoMatchRCNN.paste_masks is True and MatchRCNN.paste_masks is True and "paste_masks" not in vars(MatchRCNN)
