"""Hand-checkable cases that pin tests/lviseval_oracle.py, the numpy restatement of the LVIS evaluation rules the device evaluator is compared
against (tests/test_gpu_lviseval.py).  Every expected number is worked out in the comment next to it.  No GPU, no library."""
import numpy as np
import pytest

from tests import lviseval_oracle as lo

ONE = 1.0 / (1.0 + np.spacing(1))            # precision of "all true positives": tp / (fp + tp + spacing(1))
BOX, FAR, ELSE = [0., 0., 10., 10.], [100., 100., 10., 10.], [50., 50., 5., 5.]      # areas 100, 100, 25: all "small"


def _dataset(images, cats, anns):
    """images: (id, neg, not exhaustive); cats: (id, frequency); anns: (image, category, box[, extra fields])."""
    rows = []
    for j, a in enumerate(anns):
        extra = a[3] if len(a) > 3 else {}
        rows.append(dict({"id": j + 1, "image_id": a[0], "category_id": a[1], "bbox": a[2], "area": a[2][2] * a[2][3]}, **extra))
    return {"images": [{"id": i, "neg_category_ids": list(neg), "not_exhaustive_category_ids": list(nel)} for i, neg, nel in images],
            "categories": [{"id": c, "frequency": f} for c, f in cats], "annotations": rows}


def _dt(img, cat, box, score):
    return {"image_id": img, "category_id": cat, "bbox": box, "score": score}


_run = lo.run                                # -> ev, precision, recall, results, printed text


def test_the_cut_comes_before_the_federated_filter():
    """300 high-score detections of a category that is neither positive nor negative in the image fill the image's 300 places and are then
    dropped by the filter; the true positive behind them was cut: no detection is left, recall 0."""
    dataset = _dataset([(1, [], [])], [(1, "f"), (2, "f")], [(1, 1, BOX)])
    crowd = [_dt(1, 2, ELSE, 0.9) for _ in range(300)]
    ev, precision, recall, res, _ = _run(dataset, crowd + [_dt(1, 1, BOX, 0.5)])
    assert ev["counters"]["cut_dropped"] == 1 and ev["counters"]["federated_dropped"] == 300
    assert len(ev["groups"]) == 1 and len(ev["groups"][(0, 0)]["dt"]) == 0
    assert (recall[:, 0, 0] == 0).all() and (precision[:, :, 0, 0] == 0).all() and (precision[:, :, 1] == -1).all()
    assert res["AP"] == 0 and res["AR@300"] == 0
    # one fewer and the true positive is inside the cut
    ev, precision, recall, res, _ = _run(dataset, crowd[:299] + [_dt(1, 1, BOX, 0.5)])
    assert ev["counters"]["cut_dropped"] == 0 and ev["counters"]["federated_dropped"] == 299
    assert (recall[:, 0, 0] == 1).all() and (precision[:, :, 0, 0] == ONE).all()
    assert res["AP"] == pytest.approx(1.0, abs=1e-12) and res["AR@300"] == 1


def test_a_detection_in_an_unlisted_category_is_no_false_positive():
    """Category 2 is positive in image 2 only.  Its detection in image 1 (not positive, not negative there) is dropped: AP as without it."""
    dataset = _dataset([(1, [], []), (2, [], [])], [(1, "f"), (2, "f")], [(1, 1, BOX), (2, 2, BOX)])
    base = [_dt(1, 1, BOX, 0.5), _dt(2, 2, BOX, 0.5)]
    _, p0, r0, res0, _ = _run(dataset, base)
    ev, p1, r1, res1, _ = _run(dataset, base + [_dt(1, 2, ELSE, 0.9)])
    assert ev["counters"]["federated_dropped"] == 1 and ev["counters"]["neg_false_positive"] == 0
    assert np.array_equal(p0, p1) and np.array_equal(r0, r1) and list(res0.items()) == list(res1.items())
    assert (p1[:, :, :, 0] == ONE).all() and res1["AP"] == pytest.approx(1.0, abs=1e-12)
    # detections of an unknown image or an unknown category go the same way
    _, p2, _r, _res, _ = _run(dataset, base + [_dt(77, 1, BOX, 0.9), _dt(1, 77, BOX, 0.9)])
    assert np.array_equal(p0, p2)


def test_negative_and_not_exhaustive_categories():
    """Category 1: a true positive at score 0.5 in image 2, and in image 1 a detection at 0.9 that matches nothing."""
    anns = [(2, 1, BOX)]
    results = [_dt(2, 1, BOX, 0.5), _dt(1, 1, ELSE, 0.9)]
    # image 1 lists the category as negative: a false positive in front of the true positive, tp/(fp+tp) = 1/2 at every recall
    ev, precision, recall, res, _ = _run(_dataset([(1, [1], []), (2, [], [])], [(1, "f")], anns), results)
    assert ev["counters"]["neg_false_positive"] == 20                     # 10 thresholds x the two ranges its area 25 is inside, "all" and "small" ...
    assert (precision[:, :, 0, 0] == 0.5).all() and (precision[:, :, 0, 1] == 0.5).all()
    assert (precision[:, :, 0, 2:] == -1).all()                           # ... and "medium" / "large" have no ground truth: -1
    assert res["AP"] == 0.5 and res["AR@300"] == 1
    # image 1 does not list it: dropped, AP 1
    _, precision, _r, res, _ = _run(_dataset([(1, [], []), (2, [], [])], [(1, "f")], anns), results)
    assert (precision[:, :, 0, 0] == ONE).all()
    # image 1 has the category, annotated not exhaustively: the unmatched detection is ignored, a matched one is still a true positive
    anns = [(2, 1, BOX), (1, 1, FAR)]
    results = results + [_dt(1, 1, FAR, 0.8)]
    ev, precision, recall, res, _ = _run(_dataset([(1, [], [1]), (2, [], [])], [(1, "f")], anns), results)
    g = ev["groups"][(0, 0)]
    assert g["not_exhaustive"] and g["dt_match"][0, 0].tolist() == [0, 1] and g["dt_ignore"][0, 0].tolist() == [1, 0]
    assert ev["counters"]["nel_unmatched_ignored"] > 0 and ev["counters"]["nel_matched_tp"] > 0
    # scores 0.9 ignored, 0.8 tp, 0.5 tp -> precision 0/(0 + 0 + eps) = 0, 1/(1 + eps) = ONE, 2/(2 + eps) = 1.0 (2 + eps rounds to 2); from the right 1.0
    assert (precision[:, :, 0, 0] == 1.0).all() and (recall[:, 0, 0] == 1).all()
    # the same with an exhaustive list: scores 0.9 fp, 0.8 tp, 0.5 tp -> precision 0, 1/2, 2/3, from the right 2/3 everywhere
    ev, precision, recall, res, _ = _run(_dataset([(1, [], []), (2, [], [])], [(1, "f")], anns), results)
    assert (precision[:, :, 0, 0] == 2.0 / (1.0 + 2.0 + np.spacing(1))).all() and (recall[:, 0, 0] == 1).all()
    assert res["AP"] == pytest.approx(2 / 3, abs=1e-12)


def test_an_ignored_annotation():
    """`ignore: 1` takes the annotation out of npig; the detection matched to it is ignored.  `iscrowd` is not read."""
    dataset = _dataset([(1, [], [])], [(1, "f")], [(1, 1, BOX, {"iscrowd": 1}), (1, 1, FAR, {"ignore": 1})])
    ev, precision, recall, res, _ = _run(dataset, [_dt(1, 1, FAR, 0.9), _dt(1, 1, BOX, 0.5)])
    g = ev["groups"][(0, 0)]
    assert g["gt_ignore"][0].tolist() == [0, 1] and ev["counters"]["gt_flag_ignored"] == 2          # inside "all" and "small"
    assert g["dt_match"][0, 0].tolist() == [2, 1] and g["dt_ignore"][0, 0].tolist() == [1, 0]
    assert (recall[:, 0, 0] == 1).all() and (precision[:, :, 0, 0] == ONE).all()                    # npig = 1, one true positive, no false one
    # without the detection on the annotation that counts: recall 0 although the other detection matched
    _, precision, recall, res, _ = _run(dataset, [_dt(1, 1, FAR, 0.9)])
    assert (recall[:, 0, 0] == 0).all() and res["AP"] == 0
    # crowd IoU would be i / detection area = 1 for a detection inside the box; the plain union gives 25 / 100
    assert lo.bb_iou([[0., 0., 5., 5.]], [BOX])[0, 0] == 0.25


def test_two_detections_on_one_ground_truth():
    """No re-match: the second detection on a taken ground truth is a false positive.  Scores 0.9 tp, 0.8 fp (image 1), 0.5 tp (image 2):
    recall .5 .5 1, precision 1 1/2 2/3 -> from the right 1 2/3 2/3; recall thresholds 0 ... 0.5 (51 of them) read 1, the other 50 read 2/3."""
    dataset = _dataset([(1, [], []), (2, [], [])], [(1, "f")], [(1, 1, BOX), (2, 1, BOX)])
    ev, precision, recall, res, _ = _run(dataset, [_dt(1, 1, BOX, 0.9), _dt(1, 1, BOX, 0.8), _dt(2, 1, BOX, 0.5)])
    g = ev["groups"][(0, 0)]
    assert g["dt_match"][0, 0].tolist() == [1, 0] and g["dt_ignore"][0, 0].tolist() == [0, 0] and g["gt_match"][0, 0].tolist() == [1]
    assert ev["counters"]["matched_gt_skipped"] == 40                     # once per threshold and range: outside its range it is ignored, yet taken
    assert (precision[:, :51, 0, 0] == ONE).all() and (precision[:, 51:, 0, 0] == 2.0 / (1.0 + 2.0 + np.spacing(1))).all()
    assert res["AP"] == pytest.approx((51 + 50 * 2 / 3) / 101, abs=1e-12)


THREE = _dataset([(1, [2], []), (2, [], [])], [(1, "r"), (2, "c"), (3, "f")], [(1, 1, BOX), (2, 2, BOX), (2, 3, FAR)])
THREE_RESULTS = [_dt(1, 1, BOX, 0.5),                                     # category 1 (rare): one true positive, AP 1
                 _dt(1, 2, ELSE, 0.9), _dt(2, 2, BOX, 0.5)]               # category 2 (common): a negative-category false positive first, AP 1/2
                                                                          # category 3 (frequent): a ground truth and no detection, AP 0


def test_frequency_groups():
    ev, precision, recall, res, _ = _run(THREE, THREE_RESULTS)
    assert ev["freq_groups"] == [[0], [1], [2]]
    assert list(res) == list(lo.KEYS)
    assert res["APr"] == pytest.approx(1.0, abs=1e-12) and res["APc"] == 0.5 and res["APf"] == 0
    assert res["AP"] == pytest.approx(0.5, abs=1e-12) and res["AP50"] == pytest.approx(0.5, abs=1e-12) and res["APs"] == res["AP"]
    assert res["APm"] == -1 and res["APl"] == -1 and res["ARm@300"] == -1
    assert res["AR@300"] == pytest.approx(2 / 3, abs=1e-12) and res["ARs@300"] == res["AR@300"]


def test_a_frequency_group_without_categories():
    dataset = _dataset([(1, [], [])], [(1, "f"), (2, "f")], [(1, 1, BOX)])
    ev, _p, _r, res, _ = _run(dataset, [_dt(1, 1, BOX, 0.5)])
    assert ev["freq_groups"] == [[], [], [0, 1]]
    assert res["APr"] == -1 and res["APc"] == -1 and res["APf"] == pytest.approx(1.0, abs=1e-12)


def test_print_results_text():
    text = _run(THREE, THREE_RESULTS)[4]
    assert text == (" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=all] = 0.500\n"
                    " Average Precision  (AP) @[ IoU=0.50      | area=   all | maxDets=300 catIds=all] = 0.500\n"
                    " Average Precision  (AP) @[ IoU=0.75      | area=   all | maxDets=300 catIds=all] = 0.500\n"
                    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=     s | maxDets=300 catIds=all] = 0.500\n"
                    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=     m | maxDets=300 catIds=all] = -1.000\n"
                    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=     l | maxDets=300 catIds=all] = -1.000\n"
                    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  r] = 1.000\n"
                    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  c] = 0.500\n"
                    " Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=  f] = 0.000\n"
                    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=   all | maxDets=300 catIds=all] = 0.667\n"
                    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=     s | maxDets=300 catIds=all] = 0.667\n"
                    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=     m | maxDets=300 catIds=all] = -1.000\n"
                    " Average Recall     (AR) @[ IoU=0.50:0.95 | area=     l | maxDets=300 catIds=all] = -1.000\n")


def test_threshold_edges_and_the_ignore_stop():
    """IoU exactly 0.5 matches at 0.5 and not at 0.55; of two ground truths with equal IoU the later one takes over; a detection that holds a
    ground truth that counts stops at the first ignored one."""
    dataset = _dataset([(1, [], [])], [(1, "f")], [(1, 1, [0., 0., 12., 12.]), (1, 1, [0., 0., 12., 12.]), (1, 1, [0., 0., 12., 8.], {"ignore": 1})])
    ev, _p, _r, _res, _ = _run(dataset, [_dt(1, 1, [0., 0., 12., 6.], 0.9)])
    g = ev["groups"][(0, 0)]
    assert g["iou"].tolist() == [[0.5, 0.5, 0.75]]
    # at 0.5 both ground truths that count reach the threshold exactly and the later one takes over; the walk then stops in front of the
    # ignored one although its IoU is higher.  At 0.55 ... 0.75 nothing that counts is held, the walk goes on into the ignored ground truth
    # (0.75 >= the threshold) and the match is ignored.  From 0.8 on nothing matches.
    assert g["dt_match"][0, :, 0].tolist() == [2] + [3] * 5 + [0] * 4
    assert g["dt_ignore"][0, :, 0].tolist() == [0] + [1] * 5 + [0] * 4
    c = ev["counters"]
    assert c["iou_equals_threshold"] > 0 and c["equal_iou_takeover"] > 0 and c["ignore_stop"] == 2        # at 0.5, in "all" and "small"


def test_missing_fields_are_refused():
    dataset = _dataset([(1, [], [])], [(1, "f")], [(1, 1, BOX)])
    for field in ("neg_category_ids", "not_exhaustive_category_ids"):
        broken = dict(dataset, images=[{k: v for k, v in dataset["images"][0].items() if k != field}])
        with pytest.raises(ValueError, match=field):
            lo.evaluate(broken, [])
    with pytest.raises(ValueError, match="frequency"):
        lo.evaluate(dict(dataset, categories=[{"id": 1}]), [])
