"""tests/lvissegm_oracle.py pinned on a case worked out by hand, and the seeded data set of tests/test_gpu_lvissegm.py checked for the rules
it has to reach.  No GPU.

The case: 4 x 4 masks, images 1 and 2, categories 1 (r), 2 (c), 3 (f).  Image 1 lists category 3 as negative, image 2 lists category 2 as
not exhaustive.  Ground truth: A1 (image 1, category 1) = the polygon over columns 0 and 1 (8 pixels); A2 (image 2, category 2) = columns 2
and 3 as run lengths.  Detections:
  D1  image 1, category 1, 0.9: all 16 pixels       IoU with A1 = 8 / 16 = 0.5 exactly: a match at 0.5, a false positive above
  D2  image 1, category 1, 0.8: columns 0 and 1     IoU 1: at 0.5 A1 is taken (false positive), above it is the match
  D3  image 1, category 3, 0.7: one pixel           a false positive of a negative category; no ground truth anywhere: every cell -1
  D4  image 2, category 2, 0.6: column 0            IoU 0, unmatched in a not-exhaustive category: ignored
  D5  image 2, category 2, 0.5: columns 2 and 3     IoU 1: the true positive
  D6  image 2, category 1, 0.4                      image 2 lists category 1 nowhere: dropped by the federated filter
Category 1: at 0.5 the ranking is TP, FP, so precision 1 / (1 + eps) at every recall; above 0.5 it is FP, TP, precision 1 / (2 + eps) = 0.5
at every recall.  Category 2: ignored, TP: precision 1 / (1 + eps).  All areas are below 32^2: `small` equals `all`, the other two are -1."""
import numpy as np

from tests import lviseval_oracle as lo
from tests import lvissegm_oracle as so

COLS = lambda a, b: np.tile((np.arange(4) >= a) & (np.arange(4) < b), (4, 1)).astype(np.uint8)       # columns a .. b - 1 of a 4 x 4 mask
ONE = 1.0 / (1.0 + np.spacing(1))


def hand_case():
    images = [{"id": 1, "height": 4, "width": 4, "neg_category_ids": [3], "not_exhaustive_category_ids": []},
              {"id": 2, "height": 4, "width": 4, "neg_category_ids": [], "not_exhaustive_category_ids": [2]}]
    cats = [{"id": 1, "frequency": "r"}, {"id": 2, "frequency": "c"}, {"id": 3, "frequency": "f"}]
    anns = [{"id": 1, "image_id": 1, "category_id": 1, "area": 8.0, "segmentation": [[0.0, 0.0, 2.0, 0.0, 2.0, 4.0, 0.0, 4.0]]},
            {"id": 2, "image_id": 2, "category_id": 2, "area": 8.0, "segmentation": {"size": [4, 4], "counts": [8, 8]}}]
    one = np.zeros((4, 4), np.uint8)
    one[3, 3] = 1
    rows = [(1, 1, 0.9, COLS(0, 4)), (1, 1, 0.8, COLS(0, 2)), (1, 3, 0.7, one), (2, 2, 0.6, COLS(0, 1)), (2, 2, 0.5, COLS(2, 4)),
            (2, 1, 0.4, COLS(0, 2))]
    results = [{"image_id": i, "category_id": c, "score": s, "mask": m} for i, c, s, m in rows]
    return {"images": images, "categories": cats, "annotations": anns}, results


def test_masks_of_the_hand_case():
    dataset, results = hand_case()
    a1, a2 = dataset["annotations"]
    assert np.array_equal(so.segmentation_mask(a1["segmentation"], 4, 4), COLS(0, 2))
    assert np.array_equal(so.segmentation_mask(a2["segmentation"], 4, 4), COLS(2, 4))
    assert so.mask_area(results[0]["mask"]) == 16 and so.mask_box(results[0]["mask"]) == [0, 0, 4, 4]
    assert so.mask_area(results[2]["mask"]) == 1 and so.mask_box(results[2]["mask"]) == [3, 3, 1, 1]
    assert so.mask_box(np.zeros((4, 4), np.uint8)) == [0, 0, 0, 0]
    iou = so.mask_iou([r["mask"] for r in results[:2]], [COLS(0, 2)])
    assert iou.tolist() == [[0.5], [1.0]]
    assert so.to_result(results[0])["segmentation"] == {"size": [4, 4], "counts": "0`0"} and "mask" not in so.to_result(results[0])


def test_hand_case():
    dataset, results = hand_case()
    ev, precision, recall, res = so.run(dataset, results)
    assert sorted(ev["groups"]) == [(0, 0), (1, 1), (2, 0)]                          # (category index, image index)
    g = ev["groups"][(0, 0)]
    assert g["iou"].tolist() == [[0.5], [1.0]] and g["dt_area"].tolist() == [16.0, 8.0] and g["dt_box"].tolist() == [[0, 0, 4, 4], [0, 0, 2, 4]]
    assert g["dt_match"][0].tolist() == [[1, 0]] + [[0, 1]] * 9                         # `all`: D1 holds A1 at 0.5 only
    assert g["gt_match"][0].reshape(-1).tolist() == [1] + [2] * 9
    assert not g["dt_ignore"][:2].any() and g["dt_ignore"][2:].all()                  # `medium`, `large`: everything out of range
    g = ev["groups"][(1, 1)]
    assert g["not_exhaustive"] and g["iou"].tolist() == [[0.0], [1.0]]
    assert g["dt_match"][0].tolist() == [[0, 1]] * 10 and g["dt_ignore"][0].tolist() == [[1, 0]] * 10
    g = ev["groups"][(2, 0)]
    assert len(g["gt"]) == 0 and g["dt_match"].shape == (4, 10, 1) and not g["dt_ignore"][0].any()
    c = ev["counters"]
    assert c["federated_dropped"] == 1 and c["cut_dropped"] == 0 and c["neg_false_positive"] == 20        # `all` and `small`, ten thresholds
    assert c["nel_unmatched_ignored"] == 20 and c["nel_matched_tp"] == 20
    assert c["iou_equals_threshold"] == 4 and c["matched_gt_skipped"] == 4             # at 0.5, in each of the four area ranges
    want_p, want_r = np.full((10, 101, 3, 4), -1.0), np.full((10, 3, 4), -1.0)
    for a in (0, 1):
        want_p[0, :, 0, a], want_p[1:, :, 0, a], want_p[:, :, 1, a] = ONE, 0.5, ONE
        want_r[:, :2, a] = 1.0
    assert np.array_equal(precision, want_p) and np.array_equal(recall, want_r)
    assert list(res) == list(lo.KEYS)
    ap1, ap2 = (ONE + 9 * 0.5) / 10, ONE
    close = lambda got, want: abs(got - want) < 1e-12
    assert close(res["AP"], (ap1 + ap2) / 2) and close(res["AP50"], ONE) and close(res["AP75"], 0.75) and close(res["APs"], res["AP"])
    assert res["APm"] == -1 and res["APl"] == -1 and close(res["APr"], ap1) and close(res["APc"], ap2) and res["APf"] == -1
    assert res["AR@300"] == 1 and res["ARs@300"] == 1 and res["ARm@300"] == -1 and res["ARl@300"] == -1


def test_the_seeded_set_fires_every_branch():
    """The data set of tests/test_gpu_lvissegm.py reaches every rule, and holds what that test is about."""
    dataset, results = so.make_set()
    ev, precision, recall, res = so.run(dataset, results)
    counters = ev["counters"]
    assert all(counters[b] >= 1 for b in lo.BRANCHES), counters
    assert counters["cut_dropped"] == 10
    assert len(dataset["images"]) == 6 and len(set((im["height"], im["width"]) for im in dataset["images"])) == 6
    assert all(max(im["height"], im["width"]) <= 32 for im in dataset["images"])
    assert [len(c) for c in ev["freq_groups"]] == [1, 2, 2]
    assert any(im["neg_category_ids"] for im in dataset["images"]) and any(im["not_exhaustive_category_ids"] for im in dataset["images"])
    assert sum(1 for a in dataset["annotations"] if a.get("ignore")) == 1
    assert any(len(a["segmentation"]) > 1 for a in dataset["annotations"])              # annotations of several parts
    iou = np.concatenate([g["iou"].reshape(-1) for g in ev["groups"].values()])
    assert (iou == 0.5).any() and (iou == 1.0).any()
    assert any(len(g["dt"]) > 64 for g in ev["groups"].values())
    assert any(len(g["dt"]) == 0 for g in ev["groups"].values()) and any(len(g["gt"]) == 0 and len(g["dt"]) > 0 for g in ev["groups"].values())
    assert all(res[k] > 0 for k in ("AP", "APr", "APc", "APf", "AR@300"))
