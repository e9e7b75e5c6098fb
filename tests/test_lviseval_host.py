"""Host side of the LVIS evaluator: the argument checks of mi355det_lvis_match (it refuses before any launch, so they run without a GPU), what
the LVISEval constructor accepts and refuses, and the plain helpers it shares with COCOEval."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

DATASET = {"images": [{"id": 7, "neg_category_ids": [2], "not_exhaustive_category_ids": [1]}, {"id": 4, "neg_category_ids": [], "not_exhaustive_category_ids": []}],
           "categories": [{"id": 2, "frequency": "c"}, {"id": 1, "frequency": "r"}, {"id": 5, "frequency": "c"}],
           "annotations": [{"id": 1, "image_id": 7, "category_id": 1, "bbox": [0, 0, 10, 10], "area": 100, "segmentation": [[0.0, 0.0, 10.0, 0.0, 10.0, 10.0]]},
                           {"id": 2, "image_id": 4, "category_id": 2, "bbox": [0, 0, 10, 10], "area": 100, "ignore": 1},
                           {"id": 3, "image_id": 7, "category_id": 1, "bbox": [5, 5, 10, 10], "area": 100}]}


def _last_error():
    from object_detectors_amd._lib import lib
    return lib().mi355det_last_error().decode()


def test_lvis_match_refuses_bad_arguments_before_any_launch():
    from object_detectors_amd._lib import lib
    L = lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)                          # never dereferenced on the host: the refusals come first
    # 7 area ranges x 10 thresholds do not fit one lane each
    assert L.mi355det_lvis_match(1, p, p, p, 1, 1, 1, p, p, p, p, p, p, 10, p, 7, p, p, p, p, None) == -1
    assert "lvis_match" in _last_error() and "64" in _last_error()
    # groups, and no flag for them
    assert L.mi355det_lvis_match(1, p, p, p, 1, 1, 1, p, p, p, p, None, p, 10, p, 4, p, p, p, p, None) == -1
    assert "group_not_exhaustive" in _last_error()
    assert L.mi355det_lvis_match(1, p, p, p, 1, 1, 1, p, p, p, None, p, p, 10, p, 4, p, p, p, p, None) == -1          # no gt_flag
    assert L.mi355det_lvis_match(-1, p, p, p, 1, 1, 1, p, p, p, p, p, p, 10, p, 4, p, p, p, p, None) == -1
    assert L.mi355det_lvis_match(1, p, None, p, 1, 1, 1, p, p, p, p, p, p, 10, p, 4, p, p, p, p, None) == -1          # missing offsets
    # no groups: nothing to do, nothing launched
    assert L.mi355det_lvis_match(0, None, None, None, 0, 0, 0, None, None, None, None, None, None, 10, None, 4, None, None, None, None, None) == 0


def test_ops_lvis_match_refuses_cpu_tensors():
    from object_detectors_amd import ops
    off, f, u = torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.lvis_match(off, off, off, f, f, f, u, u, torch.zeros(10, dtype=torch.float64), torch.zeros((4, 2), dtype=torch.float64))


def test_constructor_forms_and_refusals(tmp_path):
    from object_detectors_amd.lviseval import RESULT_KEYS, LVISEval

    class Holder:
        dataset = DATASET
    path = tmp_path / "lvis.json"
    path.write_text(json.dumps(DATASET))
    for gt in (DATASET, Holder(), str(path), path):
        e = LVISEval(gt)                                 # polygons do not matter for boxes; no detections: nothing touches the device
        assert e.img_ids == [4, 7] and e.cat_ids == [1, 2, 5] and e.max_dets == 300
        assert e.freq_groups == [[0], [1, 2], []]        # indices into cat_ids: rare, common, frequent
        assert e.iou_thrs.shape == (10,) and e.rec_thrs.shape == (101,) and e.area_rng[0].tolist() == [0, 1e10] and e.num_added == 0
    assert RESULT_KEYS == ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")
    for iou_type in ("segm", "keypoints"):
        with pytest.raises(NotImplementedError):
            LVISEval(DATASET, iou_type=iou_type)
    for field in ("neg_category_ids", "not_exhaustive_category_ids"):
        broken = dict(DATASET, images=[{k: v for k, v in im.items() if k != field} for im in DATASET["images"]])
        with pytest.raises(ValueError, match=field):
            LVISEval(broken)
    with pytest.raises(ValueError, match="frequency"):
        LVISEval(dict(DATASET, categories=[{"id": 1}, {"id": 2, "frequency": "c"}, {"id": 5, "frequency": "x"}]))
    with pytest.raises(ValueError):
        LVISEval(DATASET, lvis_dt={"not": "a list"})
    with pytest.raises(RuntimeError):
        LVISEval(DATASET).accumulate()
    with pytest.raises(RuntimeError):
        LVISEval(DATASET).get_results()


def test_key_tables_of_the_federated_rules():
    """key = category index * images + image index, in the sorted order of cat_ids [1, 2, 5] and img_ids [4, 7]."""
    from object_detectors_amd.lviseval import LVISEval
    e = LVISEval(DATASET, device="cpu")
    gt = e._ground_truth()
    assert gt["key"].tolist() == [1, 1, 2] and gt["index"].tolist() == [0, 2, 1]          # category 1 in image 7 twice, category 2 in image 4
    assert gt["flag"].tolist() == [0, 0, 1] and gt["crowd"].tolist() == [0, 0, 0]
    assert gt["filter_keys"].tolist() == [1, 2, 3]                                        # the two positive keys and (category 2, image 7) negative
    assert gt["nel_keys"].tolist() == [1]


def test_shared_layout_helpers():
    from object_detectors_amd.cocoeval import category_order, group_offsets, sort_ground_truth
    anns = [(0, {"category_id": 9, "image_id": 1}), (1, {"category_id": 3, "image_id": 2}), (2, {"category_id": 9, "image_id": 1}),
            (3, {"category_id": 3, "image_id": 1})]
    key, order = sort_ground_truth(anns, {3: 0, 9: 1}, {1: 0, 2: 1}, 2)
    assert key.tolist() == [0, 1, 2, 2] and order.tolist() == [3, 1, 0, 2]                # stable within a group
    keys = torch.tensor([0, 2, 5])
    counts, offsets = group_offsets(keys, torch.tensor([0, 0, 5]))
    assert counts.tolist() == [2, 0, 1] and offsets.tolist() == [0, 2, 2, 3]
    counts, offsets = group_offsets(keys[:0], keys[:0])
    assert counts.tolist() == [] and offsets.tolist() == [0]
    # two categories owning slots 0..2 and 3..4: descending score within each, ties in slot order
    order = category_order(torch.tensor([0, 3, 5]), torch.tensor([.5, .9, .5, .1, .7], dtype=torch.float64))
    assert order.tolist() == [1, 0, 2, 4, 3]
