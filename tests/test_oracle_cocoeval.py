"""Hand-checkable cases that pin tests/cocoeval_oracle.py, the numpy restatement of the COCO evaluation rules the device evaluator is compared
against.  No GPU."""
import numpy as np

from tests import cocoeval_oracle as co

ONE = 1.0 / (1.0 + 2.0 ** -52)          # a precision of "1": tp / (fp + tp + 2^-52) = 0.9999999999999998
# The mean of 101 such entries (one threshold's recall axis) is one ulp of rounding away under numpy's pairwise summation: the sum rounds
# to 101 - 2^-46 and the quotient to 1 - 2^-53 = 0.9999999999999999; the mean of all 1010 entries comes back to 0.9999999999999998.
ONE_101 = np.full(101, ONE).mean()


def dataset(anns, cats=(1,), images=(1,)):
    return {"images": [{"id": i} for i in images], "categories": [{"id": c} for c in cats],
            "annotations": [dict({"id": j + 1, "image_id": 1, "category_id": 1, "iscrowd": 0}, **a) for j, a in enumerate(anns)]}


def det(bbox, score, cat=1, img=1):
    return {"image_id": img, "category_id": cat, "bbox": list(bbox), "score": score}


GT = {"bbox": [0, 0, 10, 10], "area": 100}


def run(ds, results):
    ev = co.evaluate(ds, results)
    precision, recall, scores = co.accumulate(ev)
    return ev, precision, recall, scores, co.summarize(precision, recall)


def test_parameters():
    assert co.IOU_THRS.shape == (10,) and co.REC_THRS.shape == (101,) and co.IOU_THRS.dtype == np.float64
    assert co.MAX_DETS == [1, 10, 100] and co.AREA_RNG[1] == [0, 1024] and co.AREA_RNG[2] == [1024, 9216]
    assert ONE == 0.9999999999999998


def test_perfect_detection():
    _ev, precision, _r, scores, s = run(dataset([GT]), [det([0, 0, 10, 10], .9)])
    assert s[0] == ONE and s[1] == ONE_101 and s[2] == ONE_101
    assert abs(ONE_101 - ONE) <= 2.0 ** -53
    assert s[3] == ONE and s[4] == -1 and s[5] == -1                     # area 100: "all" and "small" only
    assert s[6] == 1.0 and s[7] == 1.0 and s[8] == 1.0
    assert s[9] == 1.0 and s[10] == -1 and s[11] == -1
    assert (scores[:, :, 0, 0, 2] == .9).all() and (precision[:, :, 0, 2:, :] == -1).all()


def test_iou_exactly_half_matches_at_the_first_threshold_only():
    ev, precision, recall, _s, s = run(dataset([GT]), [det([0, 0, 10, 5], .9)])
    grp = ev["groups"][(0, 0)]
    assert grp["iou"][0, 0] == 0.5
    assert grp["dt_match"][0, :, 0].tolist() == [1] + [0] * 9            # the strict `<`: an IoU equal to the threshold matches
    assert ev["counters"]["iou_equals_threshold"] >= 1
    assert abs(s[0] - 0.1) <= np.spacing(0.1)
    assert s[1] == ONE_101 and s[2] == 0
    assert s[6] == 0.1 and s[7] == 0.1 and s[8] == 0.1
    assert (precision[0, :, 0, 0, 2] == ONE).all() and (precision[1:, :, 0, 0, 2] == 0).all()
    assert recall[0, 0, 0, 2] == 1.0 and (recall[1:, 0, 0, 2] == 0).all()


def test_false_positive_first():
    _ev, precision, _r, scores, s = run(dataset([GT]), [det([50, 50, 10, 10], .9), det([0, 0, 10, 10], .8)])
    assert s[0] == 0.5 and s[1] == 0.5 and s[2] == 0.5
    assert s[6] == 0.0 and s[7] == 1.0 and s[8] == 1.0
    assert (precision[:, :, 0, 0, 2] == 0.5).all()                       # 1 / (1 + 1 + 2^-52) rounds to 0.5
    assert (scores[:, 0, 0, 0, 2] == .9).all()                           # recall threshold 0 is reached by the first detection already
    assert (scores[:, 1:, 0, 0, 2] == .8).all()                          # every other one at the second
    assert (precision[:, 0, 0, 0, 0] == 0).all() and (precision[:, 1:, 0, 0, 0] == 0).all()      # maxDets 1: only the false positive


def test_category_without_ground_truth_does_not_move_the_means():
    ds = dataset([GT], cats=(1, 2))
    _ev, precision, recall, _s, s = run(ds, [det([0, 0, 10, 10], .9), det([0, 0, 10, 10], .9, cat=2), det([3, 3, 4, 4], .5, cat=2)])
    assert (precision[:, :, 1] == -1).all() and (recall[:, 1] == -1).all()
    assert s[0] == ONE and s[1] == ONE_101 and s[8] == 1.0


def test_detections_outside_the_lists_are_dropped():
    ev, *_ = run(dataset([GT]), [det([0, 0, 10, 10], .9), det([0, 0, 10, 10], .95, cat=7), det([0, 0, 10, 10], .95, img=9)])
    assert list(ev["groups"]) == [(0, 0)] and len(ev["groups"][(0, 0)]["dt"]) == 1


def test_crowd_matches_twice_and_ignores_both():
    crowd = {"bbox": [0, 0, 20, 20], "area": 400, "iscrowd": 1}
    ev, _p, _r, _s, s = run(dataset([crowd, {"bbox": [100, 100, 10, 10], "area": 100}]),
                            [det([0, 0, 10, 10], .9), det([5, 5, 10, 10], .8)])
    grp = ev["groups"][(0, 0)]
    assert grp["iou"][0, 0] == 1.0 and grp["iou"][1, 0] == 1.0           # u = da: both detections lie inside the crowd region
    assert co.bb_iou([[0, 0, 10, 10]], [[0, 0, 20, 20]], [0])[0, 0] == 0.25
    assert (grp["dt_match"][0, :, :] == 1).all()                         # both matched to ground truth 0 at every threshold
    assert (grp["dt_ignore"][0, :, :] == 1).all()
    assert (grp["gt_match"][0, :, 0] == 2).all() and (grp["gt_match"][0, :, 1] == 0).all()
    assert ev["counters"]["crowd_rematch"] >= 10
    assert s[0] == 0.0 and s[8] == 0.0                                   # one non-ignored ground truth, never found; no false positive either


def test_ignore_stop_and_equal_iou_takeover():
    # two ground truths with the same IoU against the detection: the later one takes over
    ev, *_ = run(dataset([{"bbox": [0, 0, 10, 10], "area": 100}, {"bbox": [0, 0, 10, 10], "area": 100}]), [det([0, 0, 10, 8], .9)])
    assert ev["groups"][(0, 0)]["dt_match"][0, 0, 0] == 2 and ev["counters"]["equal_iou_takeover"] >= 1
    # small range: the large ground truth is ignored there; the detection keeps its non-ignored match and the walk stops
    ev, *_ = run(dataset([{"bbox": [0, 0, 100, 100], "area": 10000}, {"bbox": [0, 0, 10, 10], "area": 100}]), [det([0, 0, 10, 10], .9)])
    grp = ev["groups"][(0, 0)]
    assert grp["gt_ignore"][1].tolist() == [1, 0] and grp["dt_match"][1, 0, 0] == 2 and ev["counters"]["ignore_stop"] >= 1


def test_only_the_top_100_of_130_count_and_equal_scores_keep_input_order():
    rng = np.random.RandomState(3)
    score = np.round(rng.rand(130) * 20) / 20                            # many ties
    results = [det([float(j), 0, 10, 10], float(score[j])) for j in range(130)]
    ev, *_ = run(dataset([GT]), results)
    grp = ev["groups"][(0, 0)]
    want = sorted(range(130), key=lambda j: (-score[j], j))[:100]
    assert [r["bbox"][0] for r in grp["dt"]] == [float(j) for j in want]
    assert grp["dt_match"].shape == (4, 10, 100) and grp["iou"].shape == (100, 1)


def test_mask_iou_on_bitmaps():
    a = np.zeros((6, 7), np.uint8)
    a[1:4, 1:5] = 1                                                      # 12 pixels
    b = np.zeros((6, 7), np.uint8)
    b[2:6, 3:7] = 1                                                      # 16 pixels, 4 shared
    iou = co.mask_iou([a, np.zeros_like(a)], [b, b], [0, 1])
    assert iou[0, 0] == 4 / 24 and iou[0, 1] == 4 / 12 and (iou[1] == 0).all()
