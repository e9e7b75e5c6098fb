"""The device LVIS `segm` evaluator (lviseval.LVISSegmEval) against the literal form of the rules (tests/lvissegm_oracle.py).  Mask IoUs are
quotients of two pixel counts, done once on both sides, and everything else is integers or the float64 operations of the `bbox` evaluator in
the same order: every comparison is exact."""
import json

import numpy as np
import pytest
import torch

from tests import bootstrap_oracle as bo
from tests import lviseval_oracle as lo
from tests import lvissegm_oracle as so

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MATCH = ("iou", "dt_match", "dt_ignore", "gt_match", "gt_ignore")


def _flatten(ev):
    """The groups of the restated evaluation in the device's slot layout: category-major, image second."""
    keys = sorted(ev["groups"])
    groups = [ev["groups"][k] for k in keys]
    I = len(ev["img_ids"])
    A, T = len(lo.AREA_RNG), len(lo.IOU_THRS)
    none = {"dt_match": np.zeros((A, T, 0)), "dt_ignore": np.zeros((A, T, 0)), "gt_match": np.zeros((A, T, 0)), "gt_ignore": np.zeros((A, 0))}
    cat = lambda name, axis, dtype: np.concatenate([g[name] for g in groups] + [none[name]], axis).astype(dtype)
    return {"keys": np.asarray([k * I + i for k, i in keys], np.int64), "iou": np.concatenate([g["iou"].reshape(-1) for g in groups] + [np.zeros(0)]),
            "dt_offsets": np.cumsum([0] + [len(g["dt"]) for g in groups]), "gt_offsets": np.cumsum([0] + [len(g["gt"]) for g in groups]),
            "iou_offsets": np.cumsum([0] + [len(g["dt"]) * len(g["gt"]) for g in groups]),
            "not_exhaustive": np.asarray([g["not_exhaustive"] for g in groups], np.uint8),
            "dt_area": np.concatenate([g["dt_area"] for g in groups] + [np.zeros(0)]),
            "dt_boxes": np.concatenate([g["dt_box"] for g in groups] + [np.zeros((0, 4), np.int64)]).astype(np.float64),
            "dt_score": np.concatenate([g["scores"] for g in groups] + [np.zeros(0)]),
            "gt_area": np.asarray([a["area"] for g in groups for a in g["gt"]], np.float64),
            "dt_match": cat("dt_match", 2, np.int32), "dt_ignore": cat("dt_ignore", 2, np.uint8), "gt_match": cat("gt_match", 2, np.int32),
            "gt_ignore": cat("gt_ignore", 1, np.uint8)}


@pytest.fixture(scope="module")
def segm_set():
    """The seeded data set, its results as a results file holds them, and what the rules give: computed once."""
    dataset, results = so.make_set()
    ev, precision, recall, res = so.run(dataset, results)
    rows = [so.to_result(r) for r in results]
    return {"dataset": dataset, "results": results, "rows": rows, "ev": ev, "flat": _flatten(ev), "precision": precision, "recall": recall,
            "res": res}


@pytest.fixture(scope="module")
def evaluated(segm_set):
    """LVISSegmEval on the polygon ground truth and the list of result dicts with strings, run once."""
    from object_detectors_amd.lviseval import LVISSegmEval
    return LVISSegmEval(segm_set["dataset"], segm_set["rows"]).run()


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _same_bits(a, b):
    """Two evaluators hold the same slot layout, match arrays, tables and results."""
    for name in ("group_keys", "dt_offsets", "gt_offsets", "iou_offsets", "group_not_exhaustive", "dt_score", "dt_boxes", "dt_area", "gt_boxes",
                 "gt_area", "gt_flag") + MATCH:
        x, y = _host(getattr(a, name)), _host(getattr(b, name))
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert np.array_equal(a.precision, b.precision) and np.array_equal(a.recall, b.recall)
    assert list(a.get_results().items()) == list(b.get_results().items())


def test_evaluator_against_the_rules(segm_set, evaluated):
    """(i): the slot layout, the match arrays, precision, recall and the thirteen results."""
    e, flat = evaluated, segm_set["flat"]
    assert e.num_added == len(segm_set["rows"]) and e.num_dt == int(flat["dt_offsets"][-1]) and e.iou_type == "segm"
    assert np.array_equal(_host(e.group_keys), flat["keys"])
    for name in ("dt_offsets", "gt_offsets", "iou_offsets"):
        assert np.array_equal(_host(getattr(e, name)), flat[name]), name
    assert np.array_equal(_host(e.group_not_exhaustive), flat["not_exhaustive"])
    for name in ("dt_area", "dt_boxes", "dt_score", "gt_area"):                       # a detection's area and box are its mask's
        assert np.array_equal(_host(getattr(e, name)), flat[name]), name
    for name in MATCH:
        got = _host(getattr(e, name))
        assert got.dtype == flat[name].dtype and np.array_equal(got, flat[name]), name
    for name in ("precision", "recall"):
        got = getattr(e, name)
        assert got.dtype == np.float64 and got.shape == segm_set[name].shape and np.array_equal(got, segm_set[name]), name
    got = e.get_results()
    assert list(got) == list(lo.KEYS)
    for k in lo.KEYS:
        assert got[k] == segm_set["res"][k], k
    assert (flat["iou"] == 0.5).any() and (flat["iou"] == 1.0).any() and e.freq_groups == segm_set["ev"]["freq_groups"]


def test_polygon_and_run_length_ground_truth_agree(segm_set, evaluated):
    """(ii): the same data set passed through polygons.dataset_to_rle beforehand, and with only some annotations converted."""
    from object_detectors_amd.lviseval import LVISSegmEval
    from object_detectors_amd.polygons import dataset_to_rle
    converted = dataset_to_rle(segm_set["dataset"])
    assert all(isinstance(a["segmentation"], dict) for a in converted["annotations"])
    _same_bits(LVISSegmEval(converted, segm_set["rows"]).run(), evaluated)
    anns = [c if j % 2 else a for j, (a, c) in enumerate(zip(segm_set["dataset"]["annotations"], converted["annotations"]))]
    _same_bits(LVISSegmEval(dict(segm_set["dataset"], annotations=anns), segm_set["rows"]).run(), evaluated)


def test_detection_forms_agree(segm_set, evaluated, tmp_path):
    """(iii): per image as RLEBatch (and as dense probabilities), as a list of result dicts with strings, as a results file."""
    from object_detectors_amd import ops
    from object_detectors_amd.lviseval import LVISSegmEval
    dataset, results = segm_set["dataset"], segm_set["results"]
    gt_path, dt_path = tmp_path / "lvis_val.json", tmp_path / "results.json"
    gt_path.write_text(json.dumps(dataset))
    dt_path.write_text(json.dumps(segm_set["rows"]))
    _same_bits(LVISSegmEval(str(gt_path), str(dt_path)).run(), evaluated)
    by_image, dense = LVISSegmEval(dataset), LVISSegmEval(dataset)
    for i in sorted(set(r["image_id"] for r in results)):
        rows = [r for r in results if r["image_id"] == i]
        cats = torch.tensor([r["category_id"] for r in rows], device=DEV)
        scores = torch.tensor([r["score"] for r in rows], dtype=torch.float32, device=DEV)
        probs = torch.from_numpy(np.stack([r["mask"] for r in rows]).astype(np.float32)).to(DEV)
        by_image.add(i, cats, scores, masks=ops.mask_rle_dense(probs, 0.5))
        dense.add(i, cats, scores, masks=probs[:, None])
    assert by_image.num_added == dense.num_added == len(results)
    _same_bits(by_image.run(), evaluated)
    _same_bits(dense.run(), evaluated)
    again = LVISSegmEval(dataset)                                                     # in two lists, and once more after reset()
    again.add_results(segm_set["rows"][:100])
    again.add_results(segm_set["rows"][100:])
    _same_bits(again.run(), evaluated)
    again.reset()
    assert again.num_added == 0
    again.add_results(segm_set["rows"])
    _same_bits(again.run(), evaluated)


def _rect_counts(x, y, w, h, H, W):
    """The run lengths of the filled rectangle [x, x + w) x [y, y + h) in an H x W image."""
    m = np.zeros((H, W), np.uint8)
    m[y:y + h, x:x + w] = 1
    return so.ro.encode(m)


def test_rectangles_equal_the_box_evaluator(segm_set):
    """(iv): masks that are filled integer rectangles, annotation areas w*h: exactly the arrays of LVISEval on the rectangles."""
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    rng = np.random.default_rng(3)
    size = {im["id"]: (im["height"], im["width"]) for im in segm_set["dataset"]["images"]}

    def rect(img):
        H, W = size[img]
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        return [x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))]

    def near(img, box):
        H, W = size[img]
        x, y, w, h = (int(v) + int(rng.integers(-1, 2)) for v in box)
        x, y = min(max(x, 0), W - 1), min(max(y, 0), H - 1)
        return [x, y, min(max(w, 1), W - x), min(max(h, 1), H - y)]
    anns, rows_box, rows_segm = [], [], []
    for a in segm_set["dataset"]["annotations"]:
        b = rect(a["image_id"])
        H, W = size[a["image_id"]]
        anns.append(dict(a, bbox=[float(v) for v in b], area=float(b[2] * b[3]),
                         segmentation={"size": [H, W], "counts": _rect_counts(*b, H, W).tolist()}))
    by_image = {}
    for a in anns:
        by_image.setdefault(a["image_id"], []).append(a)
    for r in segm_set["results"]:
        if r["image_id"] not in size:
            continue
        H, W = size[r["image_id"]]
        pool = by_image.get(r["image_id"], [])
        b = near(r["image_id"], pool[int(rng.integers(0, len(pool)))]["bbox"]) if pool and rng.random() < 0.6 else rect(r["image_id"])
        row = {"image_id": r["image_id"], "category_id": r["category_id"], "score": r["score"]}
        rows_box.append(dict(row, bbox=[float(v) for v in b]))
        rows_segm.append(dict(row, bbox=[0.0, 0.0, 1.0, 1.0], segmentation={"size": [H, W], "counts": so.ro.to_string(_rect_counts(*b, H, W))}))
    dataset = dict(segm_set["dataset"], annotations=anns)
    box, segm = LVISEval(dataset, rows_box).run(), LVISSegmEval(dataset, rows_segm).run()
    _same_bits(segm, box)
    assert torch.equal(segm.dt_index, box.dt_index) and int((box.dt_match != 0).sum()) > 0 and (_host(box.iou) > 0.5).any()


def test_bootstrap_with_unit_weights_reproduces_the_results(segm_set, evaluated):
    e = evaluated
    stats, (ap, rc) = e.bootstrap(np.ones((2, len(e.img_ids)), np.int64), return_cells=True)
    assert stats.shape == (2, 13) and tuple(ap.shape) == (2, 10, len(e.cat_ids), 4, 1)
    assert np.array_equal(_host(rc[0])[..., 0], e.recall)
    assert np.array_equal(_host(ap[0])[..., 0], bo.ap_sum_of(e.precision[..., None], e.recall[..., None])[..., 0])
    want = np.asarray(list(e.get_results().values()))
    assert np.array_equal(stats[0], stats[1]) and np.array_equal(stats[0] == -1, want == -1)        # the statistics are means of those cells


def test_refusals(segm_set):
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    dataset = segm_set["dataset"]
    with pytest.raises(NotImplementedError, match="LVISSegmEval"):
        LVISEval(dataset, iou_type="segm")
    e = LVISSegmEval(dataset)
    with pytest.raises(ValueError, match="needs masks"):
        e.add(11, torch.tensor([1]), torch.tensor([0.5]))
    with pytest.raises(ValueError, match="a detection mask of image 11 is 4x4, the image 24x32"):
        e.add(11, torch.tensor([1]), torch.tensor([0.5]), masks=torch.ones((1, 4, 4)))
    with pytest.raises(ValueError, match="a detection mask of image 4 is"):
        e.add(torch.tensor([11, 4]), torch.tensor([1, 1]), torch.tensor([0.5, 0.5]), masks=torch.ones((2, 24, 32)))
    assert e.num_added == 0
    wrong = dict(dataset, annotations=[dict(dataset["annotations"][0], segmentation={"size": [5, 5], "counts": [25]})])
    with pytest.raises(ValueError, match="a ground-truth mask of image"):
        LVISSegmEval(wrong).evaluate()
