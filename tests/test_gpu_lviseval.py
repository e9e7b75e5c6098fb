"""The device LVIS evaluator (object_detectors_amd/lviseval.py, mi355det_lvis_match in csrc/cocoeval_kernels.hip) against the numpy restatement
of the rules (tests/lviseval_oracle.py).  Both sides do the same correctly rounded float64 operations in the same order and the match arrays
are integers, so every comparison is exact."""
import io
import json

import numpy as np
import pytest
import torch

from tests import lviseval_oracle as lo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")

IMG_IDS = [42, 3, 17, 8, 99, 23, 61, 70]                   # 42: no annotation, empty negative list
CATS = [(5, "r"), (2, "r"), (9, "c"), (11, "c"), (4, "f"), (7, "f")]          # 7 has no ground truth anywhere
SEED = 3


def _rand_box(rng):
    x, y = 4.0 * rng.randint(0, 30, 2)
    w, h = 4.0 * rng.randint(1, 30, 2)
    return [float(x), float(y), float(w), float(h)]


def _jitter(rng, box):
    step = lambda: 4.0 * rng.randint(-1, 2)
    x, y, w, h = box
    return [x + step(), y + step(), max(w + step(), 4.0), max(h + step(), 4.0)]


def _score(rng, lo_=1):
    return float(np.float32(rng.randint(lo_, 21) / 20))             # a float32 value: model scores are float32, widened exactly


def make_set(seed=SEED):
    """8 images, 6 categories (two rare, two common, two frequent), coordinates on a grid of 4 and scores on a grid of 1/20 (as float32), so that
    IoUs of exactly 0.5 / 0.75 and equal scores occur.  Image 3 gets 320 detections (the cut removes 20): 70 on the 70 ground truths of category
    4, 150 of category 5 (more than two chunks of the accumulate walk stay) and 100 of a category that image 3 does not list."""
    rng = np.random.RandomState(seed)
    anns, results = [], []
    images = {i: {"id": i, "neg_category_ids": [], "not_exhaustive_category_ids": []} for i in IMG_IDS}

    def gt(img, cat, box, ignore=None):
        a = {"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": box, "area": box[2] * box[3], "iscrowd": int(rng.rand() < 0.3)}
        if ignore is not None:
            a["ignore"] = ignore                                    # the field is absent from most annotations, as in LVIS
        anns.append(a)

    def dt(img, cat, box, score):
        results.append({"image_id": img, "category_id": cat, "bbox": box, "score": score})
    for img in IMG_IDS[1:]:
        cats = [5, 2, 9, 11, 4]
        positive = [c for c in cats if rng.rand() < 0.6]
        rest = [c for c in cats + [7] if c not in positive]
        negative = [c for c in rest if rng.rand() < 0.6]
        images[img]["neg_category_ids"] = negative
        images[img]["not_exhaustive_category_ids"] = [c for c in positive if rng.rand() < 0.4]
        for cat in positive:
            boxes = [_rand_box(rng) for _ in range(rng.randint(1, 6))]
            for b in boxes:
                gt(img, cat, b, ignore=1 if rng.rand() < 0.2 else None)
            for b in boxes:
                for _ in range(rng.randint(0, 4)):
                    dt(img, cat, _jitter(rng, b), _score(rng))
            for _ in range(rng.randint(0, 3)):
                dt(img, cat, _rand_box(rng), _score(rng))
        for cat in rest:                                            # negative ones: false positives; the others: dropped
            for _ in range(rng.randint(0, 3)):
                dt(img, cat, _rand_box(rng), _score(rng))
    # image 3: exactly 320 detections
    anns[:] = [a for a in anns if a["image_id"] != 3]
    results[:] = [r for r in results if r["image_id"] != 3]
    images[3]["neg_category_ids"], images[3]["not_exhaustive_category_ids"] = [7, 2], [4]
    for j in range(70):                                             # D = 70, G = 70, not exhaustive: past one wavefront in both loops
        b = _rand_box(rng)
        gt(3, 4, b, ignore=1 if j % 9 == 4 else None)
        dt(3, 4, _jitter(rng, b), _score(rng, 10))
    base = _rand_box(rng)
    gt(3, 5, base)
    for _ in range(148):                                            # 150 of category 5 with the two below, many of them low: the cut takes its 20 here
        dt(3, 5, _jitter(rng, base), _score(rng))
    for _ in range(100):                                            # neither positive nor negative in image 3: they count in the cut, then go
        dt(3, 11, _rand_box(rng), _score(rng, 10))
    gt(3, 5, [400.0, 400.0, 12.0, 12.0])                            # two ground truths with equal IoU, exactly 0.5: the later one takes over
    gt(3, 5, [400.0, 400.0, 12.0, 12.0])
    dt(3, 5, [400.0, 400.0, 12.0, 6.0], _score(rng, 19))
    dt(3, 5, [400.0, 400.0, 12.0, 9.0], _score(rng, 19))            # and IoU exactly 0.75
    if 7 not in images[70]["neg_category_ids"]:                     # a group with detections only (false positives in a negative category)
        images[70]["neg_category_ids"] = images[70]["neg_category_ids"] + [7]
    dt(70, 7, _rand_box(rng), _score(rng))
    alone = next(a["category_id"] for a in anns if a["image_id"] == 99)
    results[:] = [r for r in results if not (r["image_id"] == 99 and r["category_id"] == alone)]         # a group with ground truths only
    # image 42: nothing listed, so everything detected there is dropped
    for _ in range(5):
        dt(42, 5, _rand_box(rng), _score(rng))
    dt(1000, 5, [0., 0., 8., 8.], 0.5)                              # an unknown image
    dt(17, 77, [0., 0., 8., 8.], 0.5)                               # an unknown category
    images[17]["neg_category_ids"] = images[17]["neg_category_ids"] + [77]         # ... even where an image lists it
    anns.append({"id": 0, "image_id": 3, "category_id": 77, "bbox": [0., 0., 8., 8.], "area": 64.})       # an annotation outside the category list
    order = rng.permutation(len(results))                           # the order of arrival is not the order of the images
    results = [results[j] for j in order]
    for j, a in enumerate(anns):
        a["id"] = j + 1
    dataset = {"images": [images[i] for i in IMG_IDS], "categories": [{"id": c, "frequency": f} for c, f in CATS], "annotations": anns}
    return dataset, results


def _flatten(ev):
    """The groups of the restated evaluation in the device's slot layout: category-major, image second."""
    keys = sorted(ev["groups"])
    groups = [ev["groups"][k] for k in keys]
    I = len(ev["img_ids"])
    A, T = len(lo.AREA_RNG), len(lo.IOU_THRS)
    none = {"dt_match": np.zeros((A, T, 0)), "dt_ignore": np.zeros((A, T, 0)), "gt_match": np.zeros((A, T, 0)), "gt_ignore": np.zeros((A, 0))}
    cat = lambda name, axis, dtype: np.concatenate([g[name] for g in groups] + [none[name]], axis).astype(dtype)        # no group: empty arrays
    return {"keys": np.asarray([k * I + i for k, i in keys], np.int64), "iou": np.concatenate([g["iou"].reshape(-1) for g in groups] + [np.zeros(0)]),
            "dt_offsets": np.cumsum([0] + [len(g["dt"]) for g in groups]), "gt_offsets": np.cumsum([0] + [len(g["gt"]) for g in groups]),
            "iou_offsets": np.cumsum([0] + [len(g["dt"]) * len(g["gt"]) for g in groups]),
            "not_exhaustive": np.asarray([g["not_exhaustive"] for g in groups], np.uint8),
            "dt_area": np.asarray([np.float64(r["bbox"][2]) * np.float64(r["bbox"][3]) for g in groups for r in g["dt"]], np.float64),
            "gt_area": np.asarray([a["area"] for g in groups for a in g["gt"]], np.float64),
            "gt_flag": np.asarray([1 if a.get("ignore", 0) else 0 for g in groups for a in g["gt"]], np.uint8),
            "dt_match": cat("dt_match", 2, np.int32), "dt_ignore": cat("dt_ignore", 2, np.uint8), "gt_match": cat("gt_match", 2, np.int32),
            "gt_ignore": cat("gt_ignore", 1, np.uint8)}


def _want(dataset, results):
    ev, precision, recall, res, text = lo.run(dataset, results)
    return {"ev": ev, "flat": _flatten(ev), "precision": precision, "recall": recall, "results": res, "text": text}


@pytest.fixture(scope="module")
def lvis_set():
    dataset, results = make_set()
    return dataset, results, _want(dataset, results)


def _host(t):
    return t.cpu().numpy()


def _assert_equal(e, want):
    flat = want["flat"]
    assert np.array_equal(_host(e.group_keys), flat["keys"])
    for name in ("dt_offsets", "gt_offsets", "iou_offsets"):
        assert np.array_equal(_host(getattr(e, name)), flat[name]), name
    assert np.array_equal(_host(e.iou), flat["iou"])
    assert np.array_equal(_host(e.group_not_exhaustive), flat["not_exhaustive"])
    for name in ("dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        got = _host(getattr(e, name))
        assert got.dtype == flat[name].dtype and np.array_equal(got, flat[name]), name
    for name in ("precision", "recall"):
        got = getattr(e, name)
        assert got.dtype == np.float64 and got.shape == want[name].shape and np.array_equal(got, want[name]), name
    got = e.get_results()
    assert list(got) == list(lo.KEYS) == list(want["results"])
    for k in lo.KEYS:
        assert got[k] == want["results"][k], k
    out = io.StringIO()
    e.print_results(file=out)
    assert out.getvalue() == want["text"]


def test_the_set_fires_every_branch(lvis_set):
    """On the CPU restatement alone: the inputs reach every rule, and hold the shapes at which the device code changes path."""
    dataset, results, want = lvis_set
    counters = want["ev"]["counters"]
    assert all(counters[b] >= 1 for b in lo.BRANCHES), counters
    assert counters["cut_dropped"] == 20
    groups = want["ev"]["groups"]
    assert any(len(g["dt"]) == 70 and len(g["gt"]) == 70 for g in groups.values())
    assert any(len(g["dt"]) == 0 for g in groups.values()) and any(len(g["gt"]) == 0 and len(g["dt"]) > 0 for g in groups.values())
    I = len(IMG_IDS)
    per_cat = np.bincount([k for (k, _i), g in groups.items() for _ in g["dt"]], minlength=len(CATS))
    assert per_cat.max() > 128
    assert not any(i == sorted(IMG_IDS).index(42) for _k, i in groups)            # image 42 lists nothing: no group, its detections are dropped
    iou = want["flat"]["iou"]
    assert (iou == 0.5).any() and (iou == 0.75).any()
    assert (want["precision"][:, :, [c for c, _f in sorted(CATS)].index(7)] == -1).all()          # no ground truth anywhere: -1
    assert all(want["results"][k] > 0 for k in ("AP", "APr", "APc", "APf", "AR@300"))
    assert I == 8 and [len(c) for c in want["ev"]["freq_groups"]] == [2, 2, 2]


def test_lvis_match_entry_point(lvis_set):
    """ops.lvis_match on the groups laid out by the restatement."""
    from object_detectors_amd import ops
    flat = lvis_set[2]["flat"]
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    off = [t(flat[k].astype(np.int64)) for k in ("dt_offsets", "gt_offsets", "iou_offsets")]
    got = ops.lvis_match(*off, t(flat["iou"]), t(flat["dt_area"]), t(flat["gt_area"]), t(flat["gt_flag"]), t(flat["not_exhaustive"]),
                         t(lo.IOU_THRS), t(np.asarray(lo.AREA_RNG, np.float64)))
    for name, g in zip(("dt_match", "dt_ignore", "gt_match", "gt_ignore"), got):
        g = _host(g)
        assert g.dtype == flat[name].dtype and np.array_equal(g, flat[name]), name


def test_evaluator_against_the_rules(lvis_set):
    from object_detectors_amd.lviseval import LVISEval
    dataset, results, want = lvis_set
    e = LVISEval(dataset, results).run()
    assert e.precision.shape == (10, 101, 6, 4) and e.recall.shape == (10, 6, 4)
    assert e.freq_groups == want["ev"]["freq_groups"]
    assert e.num_dt == int(want["flat"]["dt_offsets"][-1]) and e.num_added == len(results)
    _assert_equal(e, want)


def test_add_with_device_tensors_equals_rows(lvis_set):
    """add() with float32 device tensors (all images at once, then image by image) and add_results() with rows give identical arrays."""
    from object_detectors_amd.lviseval import LVISEval
    dataset, results, want = lvis_set
    rows = LVISEval(dataset, results).run()
    col = lambda k, dt: torch.tensor([r[k] for r in results], dtype=dt, device=DEV)
    ids, cats, scores, boxes = col("image_id", torch.int64), col("category_id", torch.int64), col("score", torch.float32), col("bbox", torch.float32)
    at_once = LVISEval(dataset)
    at_once.add(ids, cats, scores, boxes)
    at_once.run()
    _assert_equal(at_once, want)
    assert torch.equal(at_once.dt_index, rows.dt_index)
    by_image = LVISEval(dataset)
    for i in sorted(set(r["image_id"] for r in results)):
        m = ids == i
        by_image.add(i, cats[m], scores[m], boxes[m])
    by_image.run()
    _assert_equal(by_image, want)
    for name in ("iou", "dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        assert torch.equal(getattr(by_image, name), getattr(rows, name)), name


def test_path_and_list_forms_agree(lvis_set, tmp_path):
    from object_detectors_amd.lviseval import LVISEval
    dataset, results, want = lvis_set
    gt_path, dt_path = tmp_path / "lvis_val.json", tmp_path / "results.json"
    gt_path.write_text(json.dumps(dataset))
    dt_path.write_text(json.dumps(results))
    from_paths = LVISEval(str(gt_path), str(dt_path), "bbox").run()
    _assert_equal(from_paths, want)


def test_run_twice_after_reset_is_bit_identical(lvis_set):
    from object_detectors_amd.lviseval import LVISEval
    dataset, results, _want_ = lvis_set
    e = LVISEval(dataset, results).run()
    first = (e.precision.tobytes(), e.recall.tobytes(), e.dt_match.clone(), e.dt_ignore.clone(), e.iou.clone(), list(e.get_results().items()))
    e.reset()
    assert e.num_added == 0
    e.add_results(results)
    e.run()
    assert e.precision.tobytes() == first[0] and e.recall.tobytes() == first[1]
    assert torch.equal(e.dt_match, first[2]) and torch.equal(e.dt_ignore, first[3]) and torch.equal(e.iou, first[4])
    assert list(e.get_results().items()) == first[5]


def test_empty_detections(lvis_set):
    from object_detectors_amd.lviseval import LVISEval
    dataset, _results, _want_ = lvis_set
    want = _want(dataset, [])
    assert want["results"]["AP"] == 0 and want["results"]["APm"] in (0, -1)
    for e in (LVISEval(dataset).run(), LVISEval(dataset, []).run()):
        _assert_equal(e, want)
    nothing = dict(dataset, annotations=[])                          # no ground truth either: no group at all, every statistic -1
    want = _want(nothing, [])
    assert want["results"]["AP"] == -1
    _assert_equal(LVISEval(nothing).run(), want)


def test_lvis_match_without_groups():
    from object_detectors_amd import ops
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt, device=DEV)
    off = z(torch.int64, 1)
    thr, rng = torch.from_numpy(lo.IOU_THRS).to(DEV), torch.from_numpy(np.asarray(lo.AREA_RNG, np.float64)).to(DEV)
    got = ops.lvis_match(off, off, off, z(torch.float64, 0), z(torch.float64, 0), z(torch.float64, 0), z(torch.uint8, 0), z(torch.uint8, 0), thr, rng)
    assert [tuple(g.shape) for g in got] == [(4, 10, 0), (4, 10, 0), (4, 10, 0), (4, 0)]


def test_refusals(lvis_set):
    from object_detectors_amd import ops
    from object_detectors_amd.lviseval import LVISEval
    dataset = lvis_set[0]
    off = torch.zeros(1, dtype=torch.int64)
    f, u = torch.zeros(0, dtype=torch.float64), torch.zeros(0, dtype=torch.uint8)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.lvis_match(off, off, off, f, f, f, u, u, torch.from_numpy(lo.IOU_THRS), torch.zeros((4, 2), dtype=torch.float64))
    broken = dict(dataset, images=[{k: v for k, v in im.items() if k != "neg_category_ids"} for im in dataset["images"]])
    with pytest.raises(ValueError, match="neg_category_ids"):
        LVISEval(broken)
    with pytest.raises(NotImplementedError):
        LVISEval(dataset, iou_type="segm")


def test_shared_walk_equals_coco_match():
    """With no flag set anywhere and no crowd, the LVIS variant of the walk is the COCO one: every output of ops.lvis_match equals ops.coco_match."""
    from object_detectors_amd import ops
    from tests import cocoeval_oracle as co
    from tests.test_gpu_cocoeval import _flatten as coco_flatten, make_bbox_set
    dataset, results = make_bbox_set(True, 5)
    for a in dataset["annotations"]:
        a["iscrowd"] = 0
    ev = co.evaluate(dataset, results)
    flat = coco_flatten(ev)
    groups = [ev["groups"][k] for k in sorted(ev["groups"])]
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x, dt))).to(DEV)
    off = [t(flat["dt_offsets"], np.int64), t(flat["gt_offsets"], np.int64), t(np.cumsum([0] + [len(g["dt"]) * len(g["gt"]) for g in groups]), np.int64)]
    dt_area = t([np.float64(r["bbox"][2]) * np.float64(r["bbox"][3]) for g in groups for r in g["dt"]], np.float64)
    gt_area = t([a["area"] for g in groups for a in g["gt"]], np.float64)
    zeros = torch.zeros(int(gt_area.shape[0]), dtype=torch.uint8, device=DEV)
    thr, rng = t(co.IOU_THRS, np.float64), t(co.AREA_RNG, np.float64)
    coco = ops.coco_match(*off, t(flat["iou"], np.float64), dt_area, gt_area, zeros, thr, rng)
    lvis = ops.lvis_match(*off, t(flat["iou"], np.float64), dt_area, gt_area, zeros, torch.zeros(len(groups), dtype=torch.uint8, device=DEV), thr, rng)
    for name, c, l in zip(("dt_match", "dt_ignore", "gt_match", "gt_ignore"), coco, lvis):
        assert c.dtype == l.dtype and torch.equal(c, l), name
        assert np.array_equal(_host(c), flat[name]), name
    assert int((coco[0] != 0).sum()) > 0 and int(coco[1].sum()) > 0
