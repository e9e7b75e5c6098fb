"""Anchors tests/oks_oracle.py, the literal host form of COCO keypoint evaluation, to values a reader can check by hand against math.exp."""
import math

import numpy as np

from tests import oks_oracle as ko


def test_identical_keypoints_give_exactly_one():
    gt = [10.0, 20.0, 2, 30.5, 41.25, 1, 0.0, 0.0, 0]
    assert ko.oks_pair(gt, gt, [5, 5, 40, 50], 777.0, ko.variances([0.1, 0.2, 0.3])) == 1.0
    assert ko.oks_pair([10.0, 20.0, 30.5, 41.25, 99.0, 99.0], gt, [5, 5, 40, 50], 777.0, ko.variances([0.1, 0.2, 0.3])) == 1.0   # x, y only


def test_one_visible_keypoint_is_exp_of_minus_e():
    """sigma 0.5: vars = (2 * 0.5)^2 = 1; area 8 (8 + 2^-52 rounds to 8); squared distance 16: e = 16 / 1 / 8 / 2 = 1."""
    assert ko.variances([0.5, 0.5]) == [1.0, 1.0] and 8.0 + ko.EPS == 8.0
    gt = [100.0, 100.0, 2, 0.0, 0.0, 0]
    dt = [104.0, 100.0, 1, 55.0, 66.0, 1]
    assert ko.oks_pair(dt, gt, [90, 90, 20, 20], 8.0, [1.0, 1.0]) == math.exp(-1.0)
    dt = [97.0, 104.0, 1, 0.0, 0.0, 1]                                                 # dx = -3, dy = 4: 25 / 1 / 12.5 / 2 = 1
    assert 12.5 + ko.EPS == 12.5 and ko.oks_pair(dt, gt, [90, 90, 20, 20], 12.5, [1.0, 1.0]) == math.exp(-1.0)


def test_invisible_keypoint_does_not_count():
    gt = [100.0, 100.0, 2, 0.0, 0.0, 0]
    near = ko.oks_pair([104.0, 100.0, 1, 0.0, 0.0, 1], gt, [90, 90, 20, 20], 8.0, [1.0, 1.0])
    far = ko.oks_pair([104.0, 100.0, 1, 1e6, -1e6, 1], gt, [90, 90, 20, 20], 8.0, [1.0, 1.0])
    assert near == far == math.exp(-1.0)


def test_no_visible_keypoint_measures_the_distance_to_the_doubled_box():
    """box [10, 10, 20, 20]: x0 = y0 = -10, x1 = y1 = 50.  Inside: every e is 0.  3 px outside in x with vars 1 and area 4.5 (4.5 + 2^-52
    rounds to 4.5): e = 9 / 1 / 4.5 / 2 = 1, so with K = 2 the similarity is (exp(0) + exp(-1)) / 2."""
    gt = [0.0, 0.0, 0, 0.0, 0.0, 0]
    box = [10.0, 10.0, 20.0, 20.0]
    assert 4.5 + ko.EPS == 4.5
    assert ko.oks_pair([-10.0, 50.0, 1, 20.0, 30.0, 1], gt, box, 4.5, [1.0, 1.0]) == 1.0           # on the border counts as inside
    assert ko.oks_pair([20.0, 30.0, 1, 53.0, 12.0, 1], gt, box, 4.5, [1.0, 1.0]) == (1.0 + math.exp(-1.0)) / 2
    assert ko.oks_pair([20.0, 30.0, 1, -13.0, 12.0, 1], gt, box, 4.5, [1.0, 1.0]) == (1.0 + math.exp(-1.0)) / 2
    assert ko.oks_pair([53.0, 53.0, 1], gt[:3], box, 4.5, [1.0]) == math.exp(-2.0)                # 3 px out in x and in y: e = 18 / 4.5 / 2


def test_result_area_box_and_flags():
    area, box = ko.result_area_box([3.0, 9.0, 1, 13.0, 4.0, 1, 8.0, 6.0, 0], 3)                 # all K keypoints, whatever their third value
    assert area == 50.0 and box == [3.0, 4.0, 10.0, 5.0]
    assert ko.result_area_box([3.0, 9.0, 13.0, 4.0, 8.0, 6.0], 3) == (50.0, [3.0, 4.0, 10.0, 5.0])
    kp = [1.0, 1.0, 2, 0.0, 0.0, 0]
    assert ko.gt_flags({"iscrowd": 0, "num_keypoints": 1, "keypoints": kp}, 2) == (0, 0)
    assert ko.gt_flags({"iscrowd": 1, "num_keypoints": 1, "keypoints": kp}, 2) == (1, 1)
    assert ko.gt_flags({"iscrowd": 0, "num_keypoints": 0, "keypoints": kp}, 2) == (1, 0)          # ignored, and no crowd: no re-match
    assert ko.gt_flags({"iscrowd": 0, "keypoints": kp}, 2) == (0, 0)                              # the field is missing: count v > 0
    assert ko.gt_flags({"iscrowd": 0, "keypoints": [0.0] * 6}, 2) == (1, 0)


def _person(ann_id, image_id, x, y, area, **extra):
    kp = [x + 10.0, y + 10.0, 2, x + 30.0, y + 50.0, 2]
    return dict({"id": ann_id, "image_id": image_id, "category_id": 1, "bbox": [x, y, 40.0, 60.0], "area": area, "iscrowd": 0,
                 "num_keypoints": 2, "keypoints": kp}, **extra)


def test_perfect_and_missing_detections_give_the_expected_ten_numbers():
    dataset = {"images": [{"id": 1}, {"id": 2}], "categories": [{"id": 1}],
               "annotations": [_person(1, 1, 0.0, 0.0, 2000.0), _person(2, 2, 5.0, 5.0, 10000.0)]}
    rows = [{"image_id": a["image_id"], "category_id": 1, "score": 0.9, "keypoints": a["keypoints"]} for a in dataset["annotations"]]
    assert np.allclose(ko.stats(dataset, rows, [0.5, 0.5]), 1.0, rtol=0, atol=1e-15)       # a precision of 1 is 1 / (1 + 2^-52)
    got = ko.stats(dataset, rows[:1], [0.5, 0.5])                                     # the large instance is missed
    ap = 51 / 101                                                                        # precision 1 up to recall 0.5, 0 beyond
    assert np.allclose(got, [ap, ap, ap, 1.0, 0.0, 0.5, 0.5, 0.5, 1.0, 0.0], rtol=0, atol=1e-15)


def test_ignored_without_crowd_is_taken_once_and_crowd_again():
    """Two detections on one ground truth.  num_keypoints == 0: the first takes it (ignored), the second stays unmatched - a false positive.
    iscrowd: both match it, both ignored."""
    blank = _person(1, 1, 0.0, 0.0, 2000.0, num_keypoints=0, keypoints=[0.0] * 6)
    seen = _person(2, 1, 500.0, 500.0, 2000.0)
    rows = [{"image_id": 1, "category_id": 1, "score": s, "keypoints": [10.0, 10.0, 1, 20.0, 20.0, 1]} for s in (0.9, 0.8)]
    rows.append({"image_id": 1, "category_id": 1, "score": 0.7, "keypoints": seen["keypoints"]})
    images, cats = [{"id": 1}], [{"id": 1}]
    g = ko.evaluate({"images": images, "categories": cats, "annotations": [blank, seen]}, rows, [0.5, 0.5])["groups"][(0, 0)]
    assert g["iou"][:2, 0].tolist() == [1.0, 1.0] and g["gt_ignore"][0].tolist() == [1, 0]
    assert g["dt_match"][0, 0].tolist() == [1, 0, 2] and g["dt_ignore"][0, 0].tolist() == [1, 0, 0]
    crowd = dict(blank, iscrowd=1, num_keypoints=2)
    ev = ko.evaluate({"images": images, "categories": cats, "annotations": [crowd, seen]}, rows, [0.5, 0.5])
    g = ev["groups"][(0, 0)]
    assert g["dt_match"][0, 0].tolist() == [1, 1, 2] and g["dt_ignore"][0, 0].tolist() == [1, 1, 0] and ev["counters"]["crowd_rematch"] > 0
