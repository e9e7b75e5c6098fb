"""LVIS `segm` evaluation (lvis-api v0.5.3 with iou_type 'segm') as the literal form of the rules, for tests/test_oracle_lvissegm.py and
tests/test_gpu_lvissegm.py.  Everything after the IoU is tests/lviseval_oracle.py (match_group, accumulate, summarize), the mask IoU is
tests/cocoeval_oracle.py's, polygons become bitmaps through tests/poly_oracle.py and strings through tests/rle_oracle.py.  What differs
from `bbox` and is written here: a detection's area and box come from its bitmap (LVISResults: area = mask area, the tight box), the IoU
is the mask IoU with no crowd, and the grouping (cut, federated filter) runs over results that carry masks.

A result is a dict with `image_id`, `category_id`, `score` and `mask` (uint8 [h, w]); an annotation's mask comes from its `segmentation`
(polygons, or {"size", "counts"} with a list or a string) and its image's `height` / `width`; its area is its `area` field."""
from collections import defaultdict

import numpy as np

from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo
from tests import poly_oracle as po
from tests import rle_oracle as ro


def segmentation_mask(seg, h, w):
    if isinstance(seg, dict):
        assert list(seg["size"]) == [h, w]
        c = seg["counts"]
        return ro.decode(ro.from_string(c) if isinstance(c, str) else c, h, w)
    return po.annotation_mask(seg, h, w)


def mask_area(mask):
    return np.float64(int((np.asarray(mask) != 0).sum()))


def mask_box(mask):
    return ro.bbox(mask)


def mask_iou(dt, gt):
    """Bitmaps [D, h, w] against [G, h, w]: LVIS has no crowds, every union is the plain one."""
    return co.mask_iou(dt, gt, [0] * len(gt))


def to_result(res):
    """The result dict as a results file holds it: the mask as {"size", "counts": str}, no bitmap."""
    m = np.asarray(res["mask"])
    out = {k: v for k, v in res.items() if k != "mask"}
    out["segmentation"] = {"size": [int(m.shape[0]), int(m.shape[1])], "counts": ro.to_string(ro.encode(m))}
    return out


def evaluate(dataset, results, counters=None):
    """lviseval_oracle.evaluate over masks: the same dict, each group also with `dt_area` [D] and `dt_box` [D, 4]."""
    counters = lo.new_counters() if counters is None else counters
    lo.check_dataset(dataset)
    img_ids = sorted(set(im["id"] for im in dataset["images"]))
    cat_ids = sorted(c["id"] for c in dataset["categories"])
    img_index = {v: i for i, v in enumerate(img_ids)}
    cat_index = {v: i for i, v in enumerate(cat_ids)}
    size = {img_index[im["id"]]: (im["height"], im["width"]) for im in dataset["images"]}
    freq = {c["id"]: c["frequency"] for c in dataset["categories"]}
    freq_groups = [[k for k, c in enumerate(cat_ids) if freq[c] == f] for f in ("r", "c", "f")]
    neg = {img_index[im["id"]]: set(im["neg_category_ids"]) for im in dataset["images"]}
    nel = {img_index[im["id"]]: set(im["not_exhaustive_category_ids"]) for im in dataset["images"]}
    gts = defaultdict(list)
    for ann in dataset.get("annotations", []):
        if ann["image_id"] in img_index and ann["category_id"] in cat_index:
            gts[(cat_index[ann["category_id"]], img_index[ann["image_id"]])].append(ann)
    per_image = defaultdict(list)
    for res in results:
        if res["image_id"] in img_index:
            per_image[img_index[res["image_id"]]].append(res)
    dts = defaultdict(list)
    for i in sorted(per_image):                                     # the cut: per image, over all categories; then the federated filter
        rows = per_image[i]
        order = np.argsort(np.asarray([-float(r["score"]) for r in rows], np.float64), kind="mergesort")
        counters["cut_dropped"] += max(len(rows) - lo.MAX_DETS, 0)
        for j in order[:lo.MAX_DETS]:
            c = rows[j]["category_id"]
            if c in cat_index and (c in neg[i] or (cat_index[c], i) in gts):
                dts[(cat_index[c], i)].append(rows[j])
            else:
                counters["federated_dropped"] += 1
    groups = {}
    A, T = len(lo.AREA_RNG), len(lo.IOU_THRS)
    for key in sorted(set(gts) | set(dts)):
        k, i = key
        h, w = size[i]
        gt, dt = gts.get(key, []), dts.get(key, [])
        D, G = len(dt), len(gt)
        for r in dt:
            assert np.asarray(r["mask"]).shape == (h, w)
        dt_area = [mask_area(r["mask"]) for r in dt]
        iou = mask_iou([r["mask"] for r in dt], [segmentation_mask(a["segmentation"], h, w) for a in gt])
        not_exhaustive, negative = cat_ids[k] in nel[i], cat_ids[k] in neg[i]
        grp = {"dt": dt, "gt": gt, "iou": iou, "scores": np.asarray([float(r["score"]) for r in dt], np.float64), "not_exhaustive": not_exhaustive,
               "dt_area": np.asarray(dt_area, np.float64), "dt_box": np.asarray([mask_box(r["mask"]) for r in dt], np.int64).reshape(-1, 4),
               "gt_ignore": np.zeros((A, G), np.uint8), "dt_match": np.zeros((A, T, D), np.int32), "dt_ignore": np.zeros((A, T, D), np.uint8),
               "gt_match": np.zeros((A, T, G), np.int32)}
        for a, rng in enumerate(lo.AREA_RNG):
            for g, ann in enumerate(gt):
                flag = bool(ann.get("ignore", 0))
                inside = not (ann["area"] < rng[0] or ann["area"] > rng[1])
                if flag and inside:
                    counters["gt_flag_ignored"] += 1
                grp["gt_ignore"][a, g] = 1 if (flag or not inside) else 0
            for t, thr in enumerate(lo.IOU_THRS):
                grp["dt_match"][a, t], grp["dt_ignore"][a, t], grp["gt_match"][a, t] = lo.match_group(
                    iou, grp["gt_ignore"][a], dt_area, rng, thr, not_exhaustive, negative, counters)
        groups[key] = grp
    return {"img_ids": img_ids, "cat_ids": cat_ids, "freq_groups": freq_groups, "groups": groups, "counters": counters}


def run(dataset, results):
    """-> (ev, precision, recall, results dict)."""
    ev = evaluate(dataset, results)
    precision, recall = lo.accumulate(ev)
    return ev, precision, recall, lo.summarize(precision, recall, ev["freq_groups"])


# ---- the seeded data set of tests/test_gpu_lvissegm.py
SIZES = {11: (24, 32), 4: (16, 20), 7: (12, 12), 2: (24, 17), 9: (9, 31), 30: (20, 32)}
CATS = [(1, "r"), (2, "c"), (3, "c"), (4, "f"), (5, "f")]
CROWDED = 11                                                        # the image with more than 300 detections
SEED = 5


def _blob(rng, h, w):
    """A random filled rectangle with a few pixels knocked out: uint8 [h, w], at least one pixel set."""
    m = np.zeros((h, w), np.uint8)
    y, x = int(rng.integers(0, h)), int(rng.integers(0, w))
    m[y:y + int(rng.integers(1, h + 1)), x:x + int(rng.integers(1, w + 1))] = 1
    holes = rng.random((h, w)) < 0.1
    if (m & ~holes).any():
        m &= ~holes
    return m


def _half(mask):
    """The first half (column-major) of the set pixels of a mask with an even number of them: IoU with the mask exactly 0.5."""
    flat = np.asarray(mask).T.reshape(-1).copy()
    on = np.flatnonzero(flat)
    assert on.size % 2 == 0 and on.size >= 2
    flat[on[on.size // 2:]] = 0
    return np.ascontiguousarray(flat.reshape(mask.shape[1], mask.shape[0]).T)


def make_set(seed=SEED):
    """-> (dataset, results).  6 images of different sizes, 5 categories, polygon ground truth (poly_oracle.random_annotation, several parts
    among them), negative and not-exhaustive categories, one `ignore` annotation, image 11 with 310 detections, detections copied from
    ground-truth masks, halves of them (IoU exactly 0.5) and random blobs; scores on a grid of 1/20 as float32 values."""
    rng = np.random.default_rng(seed)
    anns, results = [], []
    images = {i: {"id": i, "height": h, "width": w, "neg_category_ids": [], "not_exhaustive_category_ids": []} for i, (h, w) in SIZES.items()}
    score = lambda lo_=1: float(np.float32(int(rng.integers(lo_, 21)) / 20))

    def gt(img, cat, seg=None, parts=None, ignore=None):
        h, w = SIZES[img]
        seg = po.random_annotation(rng, h, w, parts) if seg is None else seg
        a = {"id": len(anns) + 1, "image_id": img, "category_id": cat, "segmentation": seg, "area": float(po.annotation_mask(seg, h, w).sum()),
             "iscrowd": int(rng.random() < 0.3)}                    # iscrowd is never read
        if ignore is not None:
            a["ignore"] = ignore
        anns.append(a)
        return po.annotation_mask(seg, h, w)

    def dt(img, cat, mask, s):
        results.append({"image_id": img, "category_id": cat, "score": s, "mask": np.ascontiguousarray(mask, np.uint8), "bbox": [0.0, 0.0, 1.0, 1.0]})
    for img, (h, w) in SIZES.items():
        cats = [c for c, _f in CATS]
        positive = [c for c in cats if rng.random() < 0.6]
        rest = [c for c in cats if c not in positive]
        images[img]["neg_category_ids"] = [c for c in rest if rng.random() < 0.6]
        images[img]["not_exhaustive_category_ids"] = [c for c in positive if rng.random() < 0.4]
        for cat in positive:
            for _ in range(int(rng.integers(1, 4))):
                m = gt(img, cat)
                if rng.random() < 0.7:
                    dt(img, cat, m, score(10))                      # a copy: IoU 1
                if m.sum() >= 2 and m.sum() % 2 == 0:
                    dt(img, cat, _half(m), score())                 # IoU exactly 0.5
                for _ in range(int(rng.integers(0, 3))):
                    dt(img, cat, _blob(rng, h, w), score())
        for cat in rest:                                            # negative ones: false positives; the others: dropped
            for _ in range(int(rng.integers(1, 3))):
                dt(img, cat, _blob(rng, h, w), score())
    # image 4, category 2, not exhaustive: a twin pair of annotations (the copy's IoU is 1 with both: the later one takes over), an
    # ignored annotation behind a plain one (the walk stops there), a matched and an unmatched detection
    anns[:] = [a for a in anns if not (a["image_id"] == 4 and a["category_id"] == 2)]
    results[:] = [r for r in results if not (r["image_id"] == 4 and r["category_id"] == 2)]
    im = images[4]
    im["neg_category_ids"] = [c for c in im["neg_category_ids"] if c != 2]
    im["not_exhaustive_category_ids"] = sorted(set(im["not_exhaustive_category_ids"]) | {2})
    twin = po.random_annotation(rng, 16, 20, 3)
    m = gt(4, 2, twin)
    gt(4, 2, twin)
    gt(4, 2, ignore=1)
    dt(4, 2, m, 0.5)
    dt(4, 2, m, 0.5)
    dt(4, 2, 1 - m, score())                                        # the complement: IoU 0 with the twins
    # equal scores of one category in two images
    gt(7, 2)
    dt(7, 2, _blob(rng, 12, 12), 0.5)
    im = images[7]
    im["neg_category_ids"] = [c for c in im["neg_category_ids"] if c != 2]
    # the crowded image: 310 detections in all, most of them of a negative category
    im = images[CROWDED]
    anns[:] = [a for a in anns if not (a["image_id"] == CROWDED and a["category_id"] == 5)]
    im["neg_category_ids"] = sorted(set(im["neg_category_ids"]) | {5})
    im["not_exhaustive_category_ids"] = [c for c in im["not_exhaustive_category_ids"] if c != 5]
    have = sum(r["image_id"] == CROWDED for r in results)
    for _ in range(310 - have):
        dt(CROWDED, 5, _blob(rng, *SIZES[CROWDED]), score())
    gt(30, 1)                                                       # a group with ground truth only
    results[:] = [r for r in results if not (r["image_id"] == 30 and r["category_id"] == 1)]
    images[30]["neg_category_ids"] = [c for c in images[30]["neg_category_ids"] if c != 1]
    dt(1000, 1, np.ones((4, 4), np.uint8), 0.5)                     # an unknown image
    dt(9, 77, _blob(rng, *SIZES[9]), 0.5)                           # an unknown category
    results = [results[j] for j in rng.permutation(len(results))]   # the order of arrival is not the order of the images
    for j, a in enumerate(anns):
        a["id"] = j + 1
    dataset = {"images": [images[i] for i in SIZES], "categories": [{"id": c, "frequency": f} for c, f in CATS], "annotations": anns}
    return dataset, results
