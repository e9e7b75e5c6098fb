"""Host side of the evaluator core (object_detectors_amd/evalcore.py): the two sort helpers, the detection store and the front ends of both
evaluators on hand-worked data sets, on the CPU.  No kernel is called: _group() is torch plumbing, and every expected array is worked out in
the comment next to it."""
import numpy as np
import pytest
import torch

from object_detectors_amd import evalcore
from tests.test_lviseval_host import DATASET as LVIS_DATASET


@pytest.mark.parametrize("keys", [[], [4, 4, 4, 4], [3, 3, 3, 7, 9, 9], [0, 1, 5, 6, 8]])
def test_rank_in_run(keys):
    want, run = [], 0
    for j, k in enumerate(keys):                          # the position within the run of equal keys, counted by hand
        run = run + 1 if j and keys[j - 1] == k else 0
        want.append(run)
    got = evalcore.rank_in_run(torch.tensor(keys, dtype=torch.int64))
    assert got.dtype == torch.int64 and got.tolist() == want


def test_score_then_key_order():
    # key 0 owns inputs 1 (.9) and 4 (.1); key 1 owns inputs 0 (.5), 2 (.5) and 3 (.9): descending score puts 3 first, and the tie of 0 and 2
    # stays in input order
    score = torch.tensor([.5, .9, .5, .9, .1], dtype=torch.float64)
    key = torch.tensor([1, 0, 1, 1, 0])
    assert evalcore.score_then_key_order(score, key).tolist() == [1, 4, 3, 0, 2]
    assert evalcore.score_then_key_order(score[:0], key[:0]).tolist() == []


def _store(**kw):
    return evalcore.DetectionStore(torch.device("cpu"), [4, 7], {4: 0, 7: 1}, **kw)


def test_detection_store_forms_agree():
    cats, scores, boxes = [1, 2, 1], [.5, .25, .75], [[0, 0, 1, 1], [1, 2, 3, 4], [5, 5, 2, 2]]
    a, b, c = _store(), _store(), _store()
    a.add("T.add", 7, torch.tensor(cats), torch.tensor(scores, dtype=torch.float32), torch.tensor(boxes, dtype=torch.float32))
    b.add("T.add", torch.tensor([7, 7, 7]), cats, scores, boxes)
    c.add_results([{"image_id": 7, "category_id": k, "score": s, "bbox": bx} for k, s, bx in zip(cats, scores, boxes)])
    want = (torch.tensor([1, 1, 1]), torch.tensor(cats), torch.tensor(scores, dtype=torch.float64), torch.tensor(boxes, dtype=torch.float64))
    for store in (a, b, c):
        got = store.tensors()
        assert store.num_added == 3 and [g.dtype for g in got] == [torch.int64, torch.int64, torch.float64, torch.float64]
        assert all(torch.equal(g, w) for g, w in zip(got, want))


def test_detection_store_unknown_image_and_empty():
    s = _store()
    s.add("T.add", 99, [1], [.5], [[0, 0, 1, 1]])                                        # one id for all, unknown
    s.add("T.add", torch.tensor([7, 99, 4]), [1, 1, 1], [.5, .5, .5], [[0, 0, 1, 1]] * 3)
    s.add_results([{"image_id": 5, "category_id": 1, "score": .5, "bbox": [0, 0, 1, 1]}])
    assert s.tensors()[0].tolist() == [-1, 1, -1, 0, -1]
    none = evalcore.DetectionStore(torch.device("cpu"), [], {})                          # no image known at all
    none.add("T.add", torch.tensor([7, 4]), [1, 1], [.5, .5], [[0, 0, 1, 1]] * 2)
    assert none.tensors()[0].tolist() == [-1, -1]
    img, cat, score, box = _store().tensors()
    assert (img.dtype, cat.dtype, score.dtype, box.dtype) == (torch.int64, torch.int64, torch.float64, torch.float64)
    assert img.shape == cat.shape == score.shape == (0,) and box.shape == (0, 4)
    assert _store(with_boxes=False, with_masks=True).tensors()[3] is None
    s.add_results([])
    assert s.num_added == 5


def test_detection_store_refusals_carry_the_front_ends_name():
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.compare import Disagreement
    from object_detectors_amd.lviseval import LVISEval
    coco = dict(LVIS_DATASET)
    box = [[0, 0, 1, 1]]
    for what, add in (("COCOEval.add", COCOEval(coco, "bbox", device="cpu").add), ("LVISEval.add", LVISEval(LVIS_DATASET, device="cpu").add),
                      ("Disagreement.add", lambda *a, **k: Disagreement(coco, device="cpu").add(0, *a, **k))):
        with pytest.raises(ValueError, match=what + ": one score per detection"):
            add(7, [1, 2], [.5], box * 2)
        with pytest.raises(ValueError, match=what + ": one box per detection"):
            add(7, [1, 2], [.5, .5], box)
        with pytest.raises(ValueError, match=what + ": one image id per detection, or one for all"):
            add(torch.tensor([7, 4, 4]), [1, 2], [.5, .5], box * 2)
    with pytest.raises(ValueError, match="COCOEval.add: bbox evaluation needs boxes"):
        COCOEval(coco, "bbox", device="cpu").add(7, [1], [.5])
    segm = COCOEval(dict(coco, annotations=[]), "segm", device="cpu")
    with pytest.raises(ValueError, match="COCOEval.add: segm evaluation needs masks"):
        segm.add(7, [1], [.5])
    with pytest.raises(ValueError, match="T.add: one mask per detection"):
        _store(with_boxes=False, with_masks=True).add("T.add", 7, [1, 2], [.5, .5], masks=["one mask"])
    assert segm.num_added == 0 and segm._dets.tensors()[0].shape == (0,)                  # a refused call adds nothing


# images [10, 20] and categories [3, 5] -> indices 0, 1; group key = category index * 2 + image index
COCO_DATASET = {"images": [{"id": 20}, {"id": 10}], "categories": [{"id": 5}, {"id": 3}],
                "annotations": [{"id": 1, "image_id": 20, "category_id": 5, "bbox": [0, 0, 4, 4], "area": 16},                 # key 3
                                {"id": 2, "image_id": 10, "category_id": 3, "bbox": [0, 0, 2, 2], "area": 4},                  # key 0
                                {"id": 3, "image_id": 20, "category_id": 5, "bbox": [1, 1, 4, 4], "area": 16, "iscrowd": 1}]}  # key 3


def test_cocoeval_group_hand_worked():
    from object_detectors_amd.cocoeval import COCOEval
    e = COCOEval(COCO_DATASET, "bbox", device="cpu")
    # added 0..100: 101 detections of category 5 in image 10 (key 2) with one score - the cut keeps the first 100 in the order added
    e.add(torch.full((101,), 10), torch.full((101,), 5), torch.full((101,), .5), torch.tensor([[0., 0., 3., 2.]]).repeat(101, 1))
    e.add_results([{"image_id": 10, "category_id": 3, "score": .9, "bbox": [0, 0, 2, 2]},          # 101: key 0
                   {"image_id": 20, "category_id": 7, "score": .99, "bbox": [0, 0, 2, 2]},         # 102: unknown category, dropped
                   {"image_id": 20, "category_id": 5, "score": .2, "bbox": [0, 0, 2, 2]},          # 103: key 3, behind 104 by score
                   {"image_id": 20, "category_id": 5, "score": .8, "bbox": [0, 0, 5, 2]},          # 104: key 3
                   {"image_id": 99, "category_id": 3, "score": .7, "bbox": [0, 0, 2, 2]}])         # 105: unknown image, dropped
    iou_size = e._group()
    assert e.dt_index.tolist() == [101] + list(range(100)) + [104, 103]
    assert e.dt_rank.dtype == torch.int32 and e.dt_rank.tolist() == [0] + list(range(100)) + [0, 1]
    assert e.group_keys.tolist() == [0, 2, 3]                       # key 2 has detections only; key 3 both sides
    assert e.dt_offsets.tolist() == [0, 1, 101, 103] and e.gt_offsets.tolist() == [0, 1, 1, 3]
    assert e.iou_offsets.tolist() == [0, 1, 1, 5] and iou_size == 5                      # 1 x 1, 100 x 0, 2 x 2
    assert e.cat_dt_offsets.tolist() == [0, 1, 103] and e.cat_gt_offsets.tolist() == [0, 1, 3]
    assert e.gt_index.tolist() == [1, 0, 2] and e.gt_flag.tolist() == [0, 0, 1] and e.gt_crowd.tolist() == [0, 0, 1]
    assert e.dt_image.tolist() == [0] * 101 + [1, 1] and e.gt_image.tolist() == [0, 1, 1]
    assert e.dt_score.tolist() == [.9] + [.5] * 100 + [.8, .2] and e.dt_area.tolist() == [4.] + [6.] * 100 + [10., 4.]
    assert e.gt_boxes.tolist() == [[0, 0, 2, 2], [0, 0, 4, 4], [1, 1, 4, 4]] and e.gt_area.tolist() == [4., 16., 16.]
    assert (e.num_dt, e.num_gt, e.num_groups, e.num_added, e.kind) == (103, 3, 3, 106, "coco")


def test_lviseval_group_hand_worked():
    """tests/test_lviseval_host.py's data set: img_ids [4, 7], cat_ids [1, 2, 5], key = category index * 2 + image index; ground-truth keys
    [1, 1, 2]; filter keys {1, 2, 3} (3: category 2 is negative in image 7); category 1 is not exhaustive in image 7 (key 1)."""
    from object_detectors_amd.lviseval import LVISEval
    e = LVISEval(LVIS_DATASET, device="cpu")
    box = [0., 0., 3., 3.]
    # image 7 gets 301 detections.  Added 0..298: category 5 (key 5, which the filter drops) with the best score, so they fill ranks 0..298
    e.add(7, torch.full((299,), 5), torch.full((299,), .9), torch.tensor([box]).repeat(299, 1))
    e.add_results([{"image_id": 7, "category_id": 1, "score": .8, "bbox": box},        # 299: rank 299 passes the cut; key 1 passes the filter
                   {"image_id": 7, "category_id": 2, "score": .7, "bbox": box},        # 300: rank 300 is cut, though its key 3 would pass the filter
                   {"image_id": 4, "category_id": 2, "score": .6, "bbox": box},        # 301: key 2
                   {"image_id": 4, "category_id": 1, "score": .95, "bbox": box},       # 302: key 0, neither positive nor negative: dropped
                   {"image_id": 4, "category_id": 9, "score": .9, "bbox": box},        # 303: unknown category: dropped
                   {"image_id": 4, "category_id": 2, "score": .65, "bbox": box}])      # 304: key 2, ahead of 301 by score
    iou_size = e._group()
    assert e.dt_index.tolist() == [299, 304, 301]
    assert e.dt_rank.dtype == torch.int32 and e.dt_rank.tolist() == [0, 0, 0]            # no per-group cut
    assert e.group_keys.tolist() == [1, 2] and e.group_not_exhaustive.tolist() == [1, 0]
    assert e.group_not_exhaustive.dtype == torch.uint8
    assert e.dt_offsets.tolist() == [0, 1, 3] and e.gt_offsets.tolist() == [0, 2, 3]
    assert e.iou_offsets.tolist() == [0, 2, 4] and iou_size == 4                         # 1 x 2, 2 x 1
    assert e.cat_dt_offsets.tolist() == [0, 1, 3, 3] and e.cat_gt_offsets.tolist() == [0, 2, 3, 3]
    assert e.gt_index.tolist() == [0, 2, 1] and e.gt_flag.tolist() == [0, 0, 1] and e.gt_crowd.tolist() == [0, 0, 0]
    assert e.dt_image.tolist() == [1, 0, 0] and e.gt_image.tolist() == [1, 1, 0]
    assert e.dt_score.tolist() == [.8, .65, .6] and e.dt_area.tolist() == [9., 9., 9.]
    assert (e.num_dt, e.num_gt, e.num_groups, e.num_added, e.kind) == (3, 3, 2, 305, "lvis")


def test_names_stay_importable():
    from object_detectors_amd import cocoeval, lviseval, tide
    for name in ("load_dataset", "category_order", "group_offsets", "sort_ground_truth", "image_indices", "check_weights", "bootstrap_cells"):
        assert getattr(cocoeval, name) is getattr(evalcore, name), name
    assert cocoeval.REC_THRS is evalcore.REC_THRS and len(cocoeval.STAT_NAMES) == 12
    assert lviseval.NO_CUT is evalcore.NO_CUT is tide.NO_CUT and evalcore.NO_CUT == 2 ** 31 - 1
    assert not hasattr(cocoeval, "_is_polygon")
    assert evalcore.masked_mean(np.asarray([-1., .25, .75])) == .5 and evalcore.masked_mean(np.asarray([-1., -1.])) == -1
