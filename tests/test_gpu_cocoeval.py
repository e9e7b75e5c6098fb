"""The device COCO evaluator (object_detectors_amd/cocoeval.py, csrc/cocoeval_kernels.hip) against the numpy restatement of the rules
(tests/cocoeval_oracle.py).  Both sides do the same correctly rounded float64 operations in the same order and the match arrays are
integers, so every comparison is exact."""
import json

import numpy as np
import pytest
import torch

from tests import cocoeval_oracle as co

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------------------------- box IoU
def _boxes(rng, n, grid):
    if grid:
        b = np.concatenate([4.0 * rng.randint(0, 8, (n, 2)), 4.0 * rng.randint(0, 6, (n, 2))], 1)       # w or h = 0 occurs
    else:
        b = np.concatenate([rng.rand(n, 2) * 40, rng.rand(n, 2) * 30], 1)
    b[0] = [0, 0, 8, 8]
    b[1] = [8, 0, 8, 8]                # touches box 0
    b[2] = [100, 100, 4, 4]            # disjoint from everything
    b[3] = [4, 4, 0, 8]                # zero area
    b[4] = [0, 0, 8, 4]                # IoU exactly 0.5 with box 0
    return b.astype(np.float64)


@pytest.mark.parametrize("grid", [True, False])
def test_box_iou(grid):
    from object_detectors_amd import ops
    rng = np.random.RandomState(11 + grid)
    dt, gt = _boxes(rng, 70, grid), _boxes(rng, 70, grid)[::-1].copy()
    crowd = (rng.rand(70) < 0.3).astype(np.uint8)
    want = co.bb_iou(dt, gt, crowd)
    got = ops.coco_box_iou(torch.from_numpy(dt).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(crowd).to(DEV))
    assert got.dtype == torch.float64 and tuple(got.shape) == (70, 70)
    assert np.array_equal(got.cpu().numpy(), want)
    if grid:
        assert (want == 0.5).any() and (want == 0).any() and (want == 1).any()
    # float32 model outputs are widened exactly
    got32 = ops.coco_box_iou(torch.from_numpy(dt.astype(np.float32)).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(crowd).to(DEV))
    assert np.array_equal(got32.cpu().numpy(), co.bb_iou(dt.astype(np.float32).astype(np.float64), gt, crowd))


def test_box_iou_empty_sides():
    from object_detectors_amd import ops
    some = torch.tensor([[0., 0., 4., 4.]], dtype=torch.float64, device=DEV)
    none = torch.zeros((0, 4), dtype=torch.float64, device=DEV)
    flag = torch.zeros(1, dtype=torch.uint8, device=DEV)
    assert tuple(ops.coco_box_iou(none, some, flag).shape) == (0, 1)
    assert tuple(ops.coco_box_iou(some, none, flag[:0]).shape) == (1, 0)
    assert tuple(ops.coco_box_iou(none, none, flag[:0]).shape) == (0, 0)


# ---------------------------------------------------------------------------------------------------------------- mask IoU
def _blob(rng, h, w):
    m = np.zeros((h, w), np.uint8)
    y0, x0 = rng.randint(0, h - 2), rng.randint(0, w - 2)
    y1, x1 = rng.randint(y0 + 1, h + 1), rng.randint(x0 + 1, w + 1)
    yy, xx = np.mgrid[0:h, 0:w]
    cy, cx, ry, rx = (y0 + y1 - 1) / 2, (x0 + x1 - 1) / 2, (y1 - y0) / 2, (x1 - x0) / 2
    m[((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0] = 1
    m[y0:y1, x0:(x0 + x1) // 2] |= (rng.rand(y1 - y0, (x0 + x1) // 2 - x0) < 0.5).astype(np.uint8)
    return m


def _masks(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    empty, full = np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)
    pixel = empty.copy()
    pixel[h // 2, w // 3] = 1
    checker = ((yy + xx) % 2).astype(np.uint8)
    ell = empty.copy()                  # an L: its tight box is [2, 2, 20, 20] ...
    ell[2:22, 2] = 1
    ell[21, 2:22] = 1
    inside = empty.copy()               # ... and this square lies inside that box without touching the L
    inside[4:10, 8:16] = 1
    return [_blob(rng, h, w) for _ in range(6)] + [empty, full, pixel, checker, ell, inside]


def _rle_batch(bitmaps):
    from object_detectors_amd import ops
    return ops.mask_rle_dense(torch.from_numpy(np.stack(bitmaps).astype(np.float32)).to(DEV), 0.5)


@pytest.mark.parametrize("size", [(37, 53), (64, 300)])
def test_mask_iou(size):
    from object_detectors_amd import ops
    rng = np.random.RandomState(size[1])
    dt, gt = _masks(rng, *size), _masks(rng, *size)
    crowd = (np.arange(12) % 3 == 1).astype(np.uint8)
    want = co.mask_iou(dt, gt, crowd)
    assert want[10, 11] == 0 and co.bb_iou([[2, 2, 20, 20]], [[8, 4, 8, 6]], [0])[0, 0] > 0         # boxes overlap, pixels do not
    got = ops.coco_mask_iou(_rle_batch(dt), _rle_batch(gt), torch.from_numpy(crowd).to(DEV))
    assert got.dtype == torch.float64
    assert np.array_equal(got.cpu().numpy(), want)


def test_mask_iou_refuses_mismatched_sizes():
    from object_detectors_amd import ops
    rng = np.random.RandomState(0)
    a, b = _rle_batch(_masks(rng, 37, 53)), _rle_batch(_masks(rng, 37, 54))
    with pytest.raises(ValueError):
        ops.coco_mask_iou(a, b, torch.zeros(12, dtype=torch.uint8, device=DEV))


# ---------------------------------------------------------------------------------------------------------------- synthetic sets
IMG_IDS = [42, 3, 17, 8, 99, 23, 61]            # 42 stays empty
CAT_IDS = [5, 2, 9]                             # 9 has no ground truth anywhere


def _counts(bitmap):
    """Column-major run lengths of a bitmap, a zero run first."""
    flat = np.concatenate([[0], np.asarray(bitmap, np.uint8).T.reshape(-1)])
    edges = np.flatnonzero(np.diff(flat) != 0)
    return np.diff(np.concatenate([[0], edges, [flat.size - 1]])).astype(np.int32).tolist()


def _rand_box(rng, grid):
    if grid:
        x, y = 4.0 * rng.randint(0, 30, 2)
        w, h = 4.0 * rng.randint(1, 30, 2)
    else:
        x, y = rng.rand(2) * 120
        w, h = rng.rand(2) * 118 + 2
    return [float(x), float(y), float(w), float(h)]


def _jitter(rng, box, grid):
    step = (lambda: 4.0 * rng.randint(-1, 2)) if grid else (lambda: rng.randn() * 3)
    x, y, w, h = box
    return [x + step(), y + step(), max(w + step(), 1.0), max(h + step(), 1.0)]


def _score(rng, grid):
    return float(rng.randint(1, 21)) / 20 if grid else float(rng.rand())


def make_bbox_set(grid, seed):
    """7 images (one empty), 3 categories (one without ground truth); groups with only detections, only ground truths, 130 detections,
    70 ground truths; crowds; and, placed deliberately, one exact-threshold pair and one pair of ground truths with equal IoU."""
    rng = np.random.RandomState(seed)
    anns, results = [], []

    def gt(img, cat, box, crowd=0, area=None):
        anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": box, "area": box[2] * box[3] if area is None else area,
                     "iscrowd": crowd})

    def dt(img, cat, box, score):
        results.append({"image_id": img, "category_id": cat, "bbox": box, "score": score})
    for img in IMG_IDS[1:]:
        for cat in CAT_IDS[:2]:
            boxes = [_rand_box(rng, grid) for _ in range(rng.randint(2, 7))]
            for b in boxes:
                gt(img, cat, b, crowd=int(rng.rand() < 0.25))
            for b in boxes:
                for _ in range(rng.randint(0, 4)):
                    dt(img, cat, _jitter(rng, b, grid), _score(rng, grid))
            for _ in range(rng.randint(0, 3)):
                dt(img, cat, _rand_box(rng, grid), _score(rng, grid))
        for _ in range(rng.randint(1, 4)):
            dt(img, 9, _rand_box(rng, grid), _score(rng, grid))                    # category 9: detections only
    base = _rand_box(rng, grid)
    for _ in range(130):                                                           # one group with 130 detections (ties in the grid style)
        dt(3, 5, _jitter(rng, base, grid), _score(rng, grid))
    gt(3, 5, base)
    have = sum(1 for x in anns if x["image_id"] == 17 and x["category_id"] == 2)
    for j in range(70 - have):                                                     # one group with 70 ground truths
        gt(17, 2, _rand_box(rng, grid), crowd=int(j % 9 == 4))
    for a in [x for x in anns if x["image_id"] == 17 and x["category_id"] == 2][-12:]:
        dt(17, 2, _jitter(rng, a["bbox"], grid), _score(rng, grid))
    anns[:] = [a for a in anns if not (a["image_id"] == 8 and a["category_id"] == 2)]          # a group with only detections
    results[:] = [r for r in results if not (r["image_id"] == 99 and r["category_id"] == 5)]   # a group with only ground truths
    gt(23, 5, [400.0, 400.0, 10.0, 10.0])                                          # IoU exactly 0.5 with its detection
    dt(23, 5, [400.0, 400.0, 10.0, 5.0], 0.975)
    gt(61, 2, [500.0, 400.0, 12.0, 12.0])                                          # two ground truths, equal IoU: the later one takes over
    gt(61, 2, [500.0, 400.0, 12.0, 12.0])
    dt(61, 2, [500.0, 400.0, 12.0, 9.0], 0.985)
    for j, a in enumerate(anns):
        a["id"] = j + 1
    # an annotation outside the category list and a detection outside the image list: both dropped
    anns.append({"id": len(anns) + 1, "image_id": 3, "category_id": 77, "bbox": [0., 0., 5., 5.], "area": 25., "iscrowd": 0})
    dt(1000, 5, [0., 0., 5., 5.], 0.5)
    dataset = {"images": [{"id": i} for i in IMG_IDS], "categories": [{"id": c} for c in CAT_IDS], "annotations": anns}
    return dataset, results


def _flatten(ev):
    """The groups of the restated evaluation in the device's slot layout: category-major, image second."""
    keys = sorted(ev["groups"])
    groups = [ev["groups"][k] for k in keys]
    I = len(ev["img_ids"])
    cat = lambda name, axis, dtype: np.concatenate([g[name] for g in groups], axis).astype(dtype)
    return {"keys": np.asarray([k * I + i for k, i in keys], np.int64), "iou": np.concatenate([g["iou"].reshape(-1) for g in groups]),
            "dt_offsets": np.cumsum([0] + [len(g["dt"]) for g in groups]), "gt_offsets": np.cumsum([0] + [len(g["gt"]) for g in groups]),
            "dt_match": cat("dt_match", 2, np.int32), "dt_ignore": cat("dt_ignore", 2, np.uint8), "gt_match": cat("gt_match", 2, np.int32),
            "gt_ignore": cat("gt_ignore", 1, np.uint8)}


def _want(dataset, results, iou_type):
    ev = co.evaluate(dataset, results, iou_type)
    precision, recall, scores = co.accumulate(ev)
    return {"ev": ev, "flat": _flatten(ev), "precision": precision, "recall": recall, "scores": scores, "stats": co.summarize(precision, recall)}


def _run(dataset, results, iou_type):
    from object_detectors_amd.cocoeval import COCOEval
    e = COCOEval(dataset, iou_type)
    e.add_results(results)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


def _assert_equal(e, want):
    flat = want["flat"]
    host = lambda t: t.cpu().numpy()
    assert np.array_equal(host(e.group_keys), flat["keys"])
    assert np.array_equal(host(e.dt_offsets), flat["dt_offsets"]) and np.array_equal(host(e.gt_offsets), flat["gt_offsets"])
    assert np.array_equal(host(e.iou), flat["iou"])
    for name in ("dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        got = host(getattr(e, name))
        assert got.dtype == flat[name].dtype and np.array_equal(got, flat[name]), name
    for name in ("precision", "recall", "scores", "stats"):
        got = getattr(e, name)
        assert got.dtype == np.float64 and got.shape == want[name].shape and np.array_equal(got, want[name]), name


@pytest.fixture(scope="module")
def bbox_sets():
    out = {}
    for grid in (True, False):
        dataset, results = make_bbox_set(grid, 5 if grid else 6)
        out[grid] = (dataset, results, _want(dataset, results, "bbox"))
    return out


@pytest.mark.parametrize("grid", [True, False])
def test_bbox_matching_and_accumulate(bbox_sets, grid):
    dataset, results, want = bbox_sets[grid]
    groups = want["ev"]["groups"]
    sizes = [(len(g["dt"]), len(g["gt"])) for g in groups.values()]
    assert any(d == 100 for d, _g in sizes) and any(g == 70 for _d, g in sizes)
    assert any(d == 0 for d, _g in sizes) and any(g == 0 and d > 0 for d, g in sizes)
    assert (want["precision"][:, :, 2] == -1).all() and (want["precision"][:, :, :2, 0, 2] > 0).any()
    assert all(want["ev"]["counters"][b] > 0 for b in co.BRANCHES), want["ev"]["counters"]      # the inputs fire every branch of the match
    e = _run(dataset, results, "bbox")
    assert e.precision.shape == (10, 101, 3, 4, 3) and e.recall.shape == (10, 3, 4, 3)
    _assert_equal(e, want)


@pytest.mark.parametrize("n", [63, 64, 65, 128, 130])
def test_accumulate_chunk_edges(n):
    """One category whose detections just miss, exactly fill and just exceed the 64-wide chunks the accumulate kernel walks; in the last case a second
    detection on 32 images makes the maxDets = 1 subset differ from the whole."""
    rng = np.random.RandomState(n)
    images = list(range(1, n + 1))
    anns = [{"id": i, "image_id": i, "category_id": 1, "bbox": [0., 0., 10., 10.], "area": 100., "iscrowd": 0} for i in images]
    results = []
    for i in images:
        hit = [0., 0., 10., float(rng.randint(4, 11))]
        miss = [50., 50., 5., 5.]
        results.append({"image_id": i, "category_id": 1, "bbox": hit if rng.rand() < .7 else miss, "score": float(rng.randint(1, 11)) / 10})
    for i in images[:32] if n == 130 else []:
        results.append({"image_id": i, "category_id": 1, "bbox": [0., 0., 10., 10.], "score": 0.05})
    dataset = {"images": [{"id": i} for i in images], "categories": [{"id": 1}], "annotations": anns}
    assert len(results) in (63, 64, 65, 128, 162)
    _assert_equal(_run(dataset, results, "bbox"), _want(dataset, results, "bbox"))


def test_repeatable(bbox_sets):
    dataset, results, _want_ = bbox_sets[False]
    a, b = _run(dataset, results, "bbox"), _run(dataset, results, "bbox")
    assert a.precision.tobytes() == b.precision.tobytes() and a.scores.tobytes() == b.scores.tobytes()
    assert torch.equal(a.dt_match, b.dt_match) and torch.equal(a.iou, b.iou)


# ---------------------------------------------------------------------------------------------------------------- segm
H, W = 37, 53


def _shape(rng):
    m = np.zeros((H, W), np.uint8)
    y0, x0 = rng.randint(0, H - 6), rng.randint(0, W - 6)
    m[y0:y0 + rng.randint(3, 20), x0:x0 + rng.randint(3, 24)] = 1
    if rng.rand() < 0.5:
        m[y0 + 1:y0 + 3, x0 + 1:x0 + 3] = 0             # a hole
    return m


def _shift(rng, m):
    out = np.roll(m, (rng.randint(-2, 3), rng.randint(-2, 3)), (0, 1))
    out[rng.randint(0, H)] = 0
    return out


def make_segm_set(seed):
    rng = np.random.RandomState(seed)
    anns, results = [], []
    for img in IMG_IDS[1:]:
        for cat in CAT_IDS[:2]:
            masks = [_shape(rng) for _ in range(rng.randint(1, 5))]
            for j, m in enumerate(masks):
                # `area` decides the range a ground truth counts in: scaled so that small, medium and large all occur
                anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "mask": m, "bbox": [0, 0, 1, 1],
                             "area": float(m.sum()) * [1.0, 10.0, 100.0][j % 3], "iscrowd": int(rng.rand() < 0.25)})
                for _ in range(rng.randint(0, 3)):
                    results.append({"image_id": img, "category_id": cat, "mask": _shift(rng, m), "score": float(rng.randint(1, 21)) / 20})
            results.append({"image_id": img, "category_id": cat, "mask": _shape(rng), "score": float(rng.rand())})
        results.append({"image_id": img, "category_id": 9, "mask": _shape(rng), "score": 0.5})
    results.append({"image_id": 3, "category_id": 5, "mask": np.zeros((H, W), np.uint8), "score": 0.99})       # an empty detection mask
    for r in results:
        r["segmentation"] = {"size": [H, W], "counts": _counts(r["mask"])}                                     # uncompressed run lengths
    dataset = {"images": [{"id": i} for i in IMG_IDS], "categories": [{"id": c} for c in CAT_IDS], "annotations": anns}
    return dataset, results


def _with_segmentation(dataset, form):
    from object_detectors_amd.rle import counts_to_string
    anns = []
    for a in dataset["annotations"]:
        m = a["mask"]
        a = {k: v for k, v in a.items() if k != "mask"}
        a["segmentation"] = {"size": [H, W], "counts": counts_to_string(_counts(m))} if form == "string" else m
        anns.append(a)
    return dict(dataset, annotations=anns)


@pytest.fixture(scope="module")
def segm_set():
    dataset, results = make_segm_set(21)
    return dataset, results, _want(dataset, results, "segm")


def test_segm_end_to_end(segm_set):
    dataset, results, want = segm_set
    assert want["stats"][0] > 0 and want["ev"]["counters"]["crowd_rematch"] > 0
    rows = [{k: v for k, v in r.items() if k != "mask"} for r in results]
    from_strings = _run(_with_segmentation(dataset, "string"), rows, "segm")
    _assert_equal(from_strings, want)
    from_bitmaps = _run(_with_segmentation(dataset, "bitmap"), rows, "segm")
    _assert_equal(from_bitmaps, want)
    assert np.array_equal(from_strings.stats, from_bitmaps.stats)


def test_polygon_ground_truth_is_refused(segm_set):
    from object_detectors_amd.cocoeval import COCOEval
    dataset = _with_segmentation(segm_set[0], "string")
    dataset["annotations"][0] = dict(dataset["annotations"][0], segmentation=[[1.0, 1.0, 9.0, 1.0, 9.0, 9.0]])
    with pytest.raises(NotImplementedError, match="polygon"):
        COCOEval(dataset, "segm")


# ---------------------------------------------------------------------------------------------------------------- public interface
def _predictions(results, with_masks):
    """The result rows as the models hand them over: per image xyxy float32 boxes, scores, labels (and the masks as an RLEBatch)."""
    preds = {}
    for img in sorted(set(r["image_id"] for r in results)):
        rows = [r for r in results if r["image_id"] == img]
        p = {"scores": torch.tensor([r["score"] for r in rows], dtype=torch.float32, device=DEV),
             "labels": torch.tensor([r["category_id"] for r in rows], dtype=torch.int64, device=DEV)}
        if with_masks:
            p["masks"] = _rle_batch([r["mask"] for r in rows])
            stats = [np.argwhere(r["mask"]) for r in rows]
            p["boxes"] = torch.tensor([[0, 0, 1, 1] if len(s) == 0 else [s[:, 1].min(), s[:, 0].min(), s[:, 1].max() + 1, s[:, 0].max() + 1]
                                       for s in stats], dtype=torch.float32, device=DEV)
        else:
            b = torch.tensor([r["bbox"] for r in rows], dtype=torch.float32, device=DEV)
            p["boxes"] = torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], 1)
        preds[img] = p
    return preds


def _rows_of(preds):
    """What the evaluator sees of these predictions, as result rows for the restated rules (float32 values, widened)."""
    from object_detectors_amd.tvision.coco_eval import prepare_for_coco_detection
    return prepare_for_coco_detection(preds)


def test_coco_evaluator_bbox_two_updates_or_one(bbox_sets):
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    dataset, results, _w = bbox_sets[True]
    preds = _predictions([r for r in results if r["image_id"] != 1000], False)
    want = co.stats(dataset, _rows_of(preds))
    ids = list(preds)
    two = CocoEvaluator(dataset, ["bbox"])
    two.update({i: preds[i] for i in ids[:3]})
    two.update({i: preds[i] for i in ids[3:]})
    one = CocoEvaluator(dataset, ["bbox"])
    one.update(preds)
    for ev in (two, one):
        ev.synchronize_between_processes()              # no process group: a no-op
        ev.accumulate()
        ev.summarize()
    assert np.array_equal(two.coco_eval["bbox"].stats, one.coco_eval["bbox"].stats)
    assert np.array_equal(one.coco_eval["bbox"].stats, want)
    with pytest.raises(ValueError):
        CocoEvaluator(dataset, ["bbox", "keypoints"])


def test_coco_evaluator_bbox_and_segm_from_rle(segm_set, tmp_path):
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    dataset, results, want = segm_set
    preds = _predictions(results, True)
    gt = _with_segmentation(dataset, "string")
    ev = CocoEvaluator(gt, ["bbox", "segm"])
    ev.update(preds)
    ev.accumulate()
    ev.summarize()
    # the scores went through float32: restate with exactly those
    rows = []
    for img in preds:
        for r in [r for r in results if r["image_id"] == img]:
            rows.append(dict(r, score=float(np.float32(r["score"]))))
    assert np.array_equal(ev.coco_eval["segm"].stats, co.stats(dataset, rows, "segm"))
    assert np.array_equal(ev.coco_eval["bbox"].stats, co.stats(dataset, _rows_of(preds), "bbox"))
    path = tmp_path / "detections.json"
    ev.save_detections(str(path))
    saved = json.load(open(path))
    assert len(saved) == 2 * len(results) and "bbox" in saved[0] and isinstance(saved[-1]["segmentation"]["counts"], str)


def test_eval_results(bbox_sets, tmp_path, monkeypatch):
    from object_detectors_amd.yolo.procedures.eval_results import eval_partial_results, eval_results, save_partial_results
    dataset, results, want = bbox_sets[False]
    path = tmp_path / "val.json"
    path.write_text(json.dumps(dataset))
    monkeypatch.delenv("owd", raising=False)
    assert eval_results(results, "coco", str(path)) == want["stats"][0]
    assert eval_results(results, "drones", str(path)) == want["stats"][0]
    assert eval_results([], "coco", str(path)) == 0
    with pytest.raises(NotImplementedError):
        eval_results(results, "lvis", str(path))
    monkeypatch.chdir(tmp_path)                          # the file protocol of the partial results, under the working directory
    save_partial_results(results[:50], 0)
    save_partial_results(results[50:], 1)
    got = eval_partial_results(3, "coco", str(path))
    assert (tmp_path / "bbox_results" / "coco" / "results_3.json").exists()
    assert got == co.stats(dataset, json.load(open(tmp_path / "bbox_results" / "coco" / "results_3.json")))[0]
