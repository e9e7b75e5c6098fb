"""Host side of the COCO evaluator: the argument checks of the entry points (they refuse before any launch, so they run without a GPU), the
run-length statistics worked out on the host for ground truth read from json, and the accepted forms of the ground truth."""
import ctypes as C
import json

import numpy as np
import pytest


def _last_error():
    from object_detectors_amd._lib import lib
    return lib().mi355det_last_error().decode()


def test_coco_iou_refuses_mismatched_mask_sizes_before_any_launch():
    from object_detectors_amd._lib import lib
    L = lib()
    off = (C.c_int64 * 3)(0, 1, 2)                       # never dereferenced on the host: the refusal comes first
    p = C.cast(off, C.c_void_p)
    dt_sizes = np.asarray([[37, 53], [37, 53]], np.int32)
    gt_sizes = np.asarray([[37, 53], [37, 54]], np.int32)
    args = lambda a, b: (1, 2, p, p, p, 2, 2, 2, p, p, p, p, p, None, 2, 8, p, p, None, 2, 8, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), p, None)
    assert L.mi355det_coco_iou(*args(dt_sizes, gt_sizes)) == -1
    assert "group 1" in _last_error() and "size" in _last_error()
    gt_sizes[1] = [0, 0]                                 # a side without masks has no size to disagree with ...
    gt_sizes[0] = [-1, 5]                                # ... but a negative one is refused
    assert L.mi355det_coco_iou(*args(dt_sizes, gt_sizes)) == -1
    assert L.mi355det_coco_iou(2, 2, p, p, p, 2, 2, 2, p, p, p, None, None, None, 0, 0, None, None, None, 0, 0, None, None, p, None) == -1
    assert L.mi355det_coco_iou(0, -1, p, p, p, 2, 2, 2, p, p, p, None, None, None, 0, 0, None, None, None, 0, 0, None, None, p, None) == -1
    # no groups: nothing to do, nothing launched
    assert L.mi355det_coco_iou(0, 0, None, None, None, 0, 0, 0, None, None, None, None, None, None, 0, 0, None, None, None, 0, 0, None, None, None, None) == 0


def test_coco_match_and_accumulate_refuse_bad_parameters():
    from object_detectors_amd._lib import lib
    L = lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)
    # 7 area ranges x 10 thresholds do not fit one lane each
    assert L.mi355det_coco_match(1, p, p, p, 1, 1, 1, p, p, p, p, p, 10, p, 7, p, p, p, p, None) == -1
    assert "64" in _last_error()
    assert L.mi355det_coco_match(0, None, None, None, 0, 0, 0, None, None, None, None, None, 10, None, 4, None, None, None, None, None) == 0
    md = (C.c_int32 * 3)(1, 10, 100)
    assert L.mi355det_coco_accumulate(1, p, p, 0, 0, None, None, None, None, None, None, 10, 4, md, 9, p, 101, p, p, p, None) == -1      # 9 maxDets
    assert L.mi355det_coco_accumulate(1, p, p, 0, 0, None, None, None, None, None, None, 10, 4, md, 3, p, 0, p, p, p, None) == -1        # no recall thresholds
    assert L.mi355det_coco_accumulate(0, None, None, 0, 0, None, None, None, None, None, None, 10, 4, md, 3, None, 101, None, None, None, None) == 0


def _counts(bitmap):
    flat = np.concatenate([[0], np.asarray(bitmap, np.uint8).T.reshape(-1)])
    edges = np.flatnonzero(np.diff(flat) != 0)
    return np.diff(np.concatenate([[0], edges, [flat.size - 1]])).astype(np.int32)


def test_counts_stats_are_area_and_tight_box():
    from object_detectors_amd.rle import counts_stats
    rng = np.random.RandomState(4)
    h, w = 13, 9
    masks = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8), (rng.rand(h, w) < 0.1).astype(np.uint8)]
    one = np.zeros((h, w), np.uint8)
    one[h - 1, 2] = one[0, 3] = 1                        # a run that goes on from the bottom of a column into the top of the next
    col = np.zeros((h, w), np.uint8)
    col[4:9, 7] = 1
    masks += [one, col]
    counts = [_counts(m) for m in masks]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in counts])]).tolist()
    area, bbox = counts_stats(np.concatenate(counts), offsets, h)
    for j, m in enumerate(masks):
        ys, xs = np.nonzero(m)
        want = [0, 0, 0, 0] if len(ys) == 0 else [xs.min(), ys.min(), xs.max() - xs.min() + 1, ys.max() - ys.min() + 1]
        assert area[j] == m.sum() and bbox[j].tolist() == want, j


DATASET = {"images": [{"id": 1}], "categories": [{"id": 1}],
           "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100, "iscrowd": 0,
                            "segmentation": [[0.0, 0.0, 10.0, 0.0, 10.0, 10.0]]}]}


def test_ground_truth_forms(tmp_path):
    from object_detectors_amd.cocoeval import COCOEval, load_dataset

    class Holder:
        dataset = DATASET
    path = tmp_path / "gt.json"
    path.write_text(json.dumps(DATASET))
    for gt in (DATASET, Holder(), str(path), path):
        assert load_dataset(gt)["annotations"][0]["area"] == 100
    with pytest.raises(ValueError):
        load_dataset(3)
    e = COCOEval(DATASET, "bbox")                        # polygons do not matter for boxes
    assert e.img_ids == [1] and e.cat_ids == [1] and e.iou_thrs.shape == (10,) and e.rec_thrs.shape == (101,)
    with pytest.raises(NotImplementedError, match="polygon"):
        COCOEval(DATASET, "segm")
    with pytest.raises(ValueError):
        COCOEval(DATASET, "keypoints")


def test_evaluator_front_ends_refuse_what_is_out_of_scope():
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    from object_detectors_amd.yolo.procedures.eval_results import eval_results
    with pytest.raises(ValueError):
        CocoEvaluator(DATASET, ["bbox", "keypoints"])
    with pytest.raises(NotImplementedError):
        eval_results([{"image_id": 1}], "lvis", "unused.json")
    assert eval_results([], "coco", "unused.json") == 0
