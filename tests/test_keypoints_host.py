"""Host side of COCO keypoint evaluation: the argument checks of mi355det_coco_oks and mi355det_keypoints_match (they refuse before any
launch, so they run without a GPU), the refusals and parameters of COCOEval(gt, "keypoints"), the result rows of the torchvision-style
front end, and the condition on the data set of tests/test_gpu_keypoints.py under which its exact comparisons are valid."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import keypoint_cases as kc
from tests import oks_oracle as ko


def _last_error():
    from object_detectors_amd._lib import lib
    return lib().mi355det_last_error().decode()


def test_coco_oks_refuses_before_any_launch():
    from object_detectors_amd._lib import lib
    L = lib()
    buf = (C.c_int64 * 4)()                                # never dereferenced on the host: the refusals come first
    p = C.cast(buf, C.c_void_p)
    call = lambda ng, nd, ngt, size, K, *ops: L.mi355det_coco_oks(ng, p, p, p, nd, ngt, size, K, *ops, None)
    assert call(1, 1, 1, 1, 0, p, p, p, p, p, p) == -1
    assert "keypoints" in _last_error()
    assert call(1, 1, 1, 1, 65, p, p, p, p, p, p) == -1
    assert "64" in _last_error()
    for missing in range(6):                               # dt_kp, gt_kp, gt_boxes, gt_area, vars, oks
        ops = [p] * 6
        ops[missing] = None
        assert call(1, 1, 1, 1, 17, *ops) == -1, missing
        assert "missing" in _last_error()
    assert call(-1, 1, 1, 1, 17, p, p, p, p, p, p) == -1
    assert call(1, -1, 1, 1, 17, p, p, p, p, p, p) == -1
    assert call(1, 1, 1, -1, 17, p, p, p, p, p, p) == -1
    assert L.mi355det_coco_oks(1, None, p, p, 1, 1, 1, 17, p, p, p, p, p, p, None) == -1          # missing offsets
    # no groups: nothing to do, nothing launched
    assert L.mi355det_coco_oks(0, None, None, None, 0, 0, 0, 17, None, None, None, None, None, None, None) == 0


def test_keypoints_match_refuses_before_any_launch():
    from object_detectors_amd._lib import lib
    L = lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)
    assert L.mi355det_keypoints_match(1, p, p, p, 1, 1, 1, p, p, p, p, p, p, 10, p, 7, p, p, p, p, None) == -1      # 70 lanes
    assert "64" in _last_error()
    assert L.mi355det_keypoints_match(1, p, p, p, 1, 1, 1, p, p, p, p, None, p, 10, p, 3, p, p, p, p, None) == -1   # no gt_crowd
    assert "missing" in _last_error()
    assert L.mi355det_keypoints_match(0, None, None, None, 0, 0, 0, None, None, None, None, None, None, 10, None, 3, None, None, None, None,
                                      None) == 0


# the data set of tests/test_cocoeval_host.py, restated: it has no keypoint annotations
BOX_DATASET = {"images": [{"id": 1}], "categories": [{"id": 1}],
               "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100, "iscrowd": 0,
                                "segmentation": [[0.0, 0.0, 10.0, 0.0, 10.0, 10.0]]}]}
KP_DATASET = {"images": [{"id": 1}], "categories": [{"id": 1}],
              "annotations": [{"id": 7, "image_id": 1, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100, "iscrowd": 0, "num_keypoints": 2,
                               "keypoints": [1, 2, 2, 3, 4, 1, 0, 0, 0]}]}


def test_a_data_set_without_keypoints_is_refused():
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISEval
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    with pytest.raises(ValueError, match="keypoints"):
        COCOEval(BOX_DATASET, "keypoints")
    with pytest.raises(ValueError, match="keypoints"):
        CocoEvaluator(BOX_DATASET, ["bbox", "keypoints"])
    with pytest.raises(ValueError, match="Unknown iou type"):
        CocoEvaluator(KP_DATASET, ["bbox", "poses"])
    with pytest.raises(NotImplementedError):
        LVISEval(dict(KP_DATASET, images=[{"id": 1, "neg_category_ids": [], "not_exhaustive_category_ids": []}],
                      categories=[{"id": 1, "frequency": "f"}]), iou_type="keypoints")


def test_keypoint_parameters():
    """Fails before this evaluator existed: COCOEval refused `keypoints` outright."""
    from object_detectors_amd.cocoeval import KP_SIGMAS, COCOEval
    e = COCOEval(KP_DATASET, "keypoints", sigmas=[0.1, 0.2, 0.3])                 # no detections: nothing touches the device
    assert e.max_dets == [20] and e.cuts == [20]
    assert e.area_rng.tolist() == [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]] and e.area_labels == ["all", "medium", "large"]
    assert e.iou_thrs.shape == (10,) and e.rec_thrs.shape == (101,) and e.num_keypoints == 3
    assert e.stat_names == ["AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl"] and len(e.stat_rows) == 10
    assert KP_SIGMAS == ko.SIGMAS and len(KP_SIGMAS) == 17
    assert COCOEval(BOX_DATASET, "bbox").max_dets == [1, 10, 100] and len(COCOEval(BOX_DATASET, "bbox").stat_names) == 12
    from object_detectors_amd.compare import per_category_table
    with pytest.raises(NotImplementedError, match="keypoints"):               # its columns are the twelve bbox / segm names
        per_category_table({"model": e})
    seventeen = dict(KP_DATASET, annotations=[dict(KP_DATASET["annotations"][0], keypoints=[0] * 51)])
    assert COCOEval(seventeen, "keypoints").num_keypoints == 17


def test_wrong_lengths_are_refused():
    from object_detectors_amd.cocoeval import COCOEval
    with pytest.raises(ValueError, match="annotation 7"):                        # 3 keypoints against the 17 default sigmas
        COCOEval(KP_DATASET, "keypoints")
    missing = dict(KP_DATASET, annotations=KP_DATASET["annotations"] + [dict(BOX_DATASET["annotations"][0], id=8)])
    with pytest.raises(ValueError, match="annotation 8"):
        COCOEval(missing, "keypoints", sigmas=[0.1, 0.2, 0.3])
    for sigmas in ([], [0.1] * 65, [0.1, -0.2, 0.3], [0.1, float("nan"), 0.3]):
        with pytest.raises(ValueError, match="sigmas"):
            COCOEval(KP_DATASET, "keypoints", sigmas=sigmas)
    with pytest.raises(ValueError, match="sigmas"):
        COCOEval(KP_DATASET, "bbox", sigmas=[0.1, 0.2, 0.3])
    e = COCOEval(KP_DATASET, "keypoints", sigmas=[0.1, 0.2, 0.3], device="cpu")
    with pytest.raises(ValueError, match="keypoint"):
        e.add_results([{"image_id": 1, "category_id": 1, "score": 0.5, "keypoints": [0.0] * 8}])
    with pytest.raises(ValueError, match="keypoints"):
        e.add(1, torch.tensor([1]), torch.tensor([0.5]), keypoints=torch.zeros(1, 4, 3))
    with pytest.raises(ValueError, match="keypoints"):
        e.add(1, torch.tensor([1]), torch.tensor([0.5]))


def test_prepare_for_coco_keypoint_rows():
    from object_detectors_amd.tvision.coco_eval import prepare_for_coco_keypoint
    kp = torch.arange(2 * 3 * 3, dtype=torch.float32).reshape(2, 3, 3)
    rows = prepare_for_coco_keypoint({5: {"boxes": torch.zeros(2, 4), "scores": torch.tensor([0.75, 0.25]), "labels": torch.tensor([1, 1]),
                                          "keypoints": kp}, 6: {}})
    assert rows == [{"image_id": 5, "category_id": 1, "keypoints": [float(v) for v in range(9)], "score": 0.75},
                    {"image_id": 5, "category_id": 1, "keypoints": [float(v) for v in range(9, 18)], "score": 0.25}]
    assert [sorted(r) for r in rows] == [["category_id", "image_id", "keypoints", "score"]] * 2


@pytest.fixture(scope="module", params=sorted(kc.CASES))
def oracle(request):
    K, sigmas, seed = kc.CASES[request.param]
    dataset, rows = kc.build(K, seed)
    return dataset, rows, ko.evaluate(dataset, rows, sigmas)


def test_the_gpu_data_set_meets_the_separation_condition(oracle):
    """What tests/test_gpu_keypoints.py asserts first, checked here too: no similarity within 1e-9 of a threshold, no two unequal values of
    a row within 1e-9 of each other."""
    _dataset, _rows, ev = oracle
    assert ko.separation_violations(ev) == []


def test_the_gpu_data_set_holds_every_case(oracle):
    dataset, rows, ev = oracle
    g = ev["groups"]
    I, K = {v: i for i, v in enumerate(ev["img_ids"])}, {v: i for i, v in enumerate(ev["cat_ids"])}
    key = lambda c, i: (K[c], I[i])
    assert len(g[key(3, 11)]["gt"]) >= 65 and len(g[key(3, 11)]["dt"]) == 20 and sum(r["image_id"] == 11 and r["category_id"] == 3 for r in rows) > 20
    assert len(g[key(3, 4)]["dt"]) == 0 and len(g[key(3, 4)]["gt"]) > 0 and len(g[key(8, 4)]["gt"]) == 0 and len(g[key(8, 4)]["dt"]) > 0
    assert any(r["image_id"] not in I for r in rows) and any(r["category_id"] not in K for r in rows)
    assert ev["counters"]["crowd_rematch"] > 0 and ev["counters"]["ignore_stop"] > 0
    crowd = g[key(3, 7)]
    c = [j for j, a in enumerate(crowd["gt"]) if a["iscrowd"]][0]
    assert (crowd["dt_match"][0, 0] == c + 1).sum() == 2
    blank = g[key(3, 30)]
    b = [j for j, a in enumerate(blank["gt"]) if a["num_keypoints"] == 0 and not a["iscrowd"]][0]
    assert (blank["iou"][:, b] == 1.0).sum() == 2 and (blank["dt_match"][0, 0] == b + 1).sum() == 1       # two lie on it, one takes it
    assert blank["dt_ignore"][0, 0][blank["dt_match"][0, 0] == b + 1].tolist() == [1]
    areas = g[key(8, 2)]
    gt_area, dt_area = [a["area"] for a in areas["gt"]], areas["dt_area"]
    for bound in (32.0 ** 2, 96.0 ** 2):
        for side in (gt_area, dt_area):
            assert any(v == bound for v in side) and any(v < bound for v in side) and any(v > bound for v in side)
    assert any("num_keypoints" not in a for a in dataset["annotations"])
    stats = ko.summarize(*ko.accumulate(ev)[:2])
    assert ((stats > 0) & (stats < 1)).all()                                 # neither a perfect nor an empty result: the numbers can differ
