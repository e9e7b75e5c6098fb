"""Boundary IoU and the `boundary` evaluations (lvis-api and the COCO boundary-IoU API, iou_type "boundary"; Cheng et al., "Boundary IoU")
as the literal form of the rule, in numpy with loops, for tests/test_oracle_boundary.py and tests/test_gpu_boundary.py.

    d          = int(round(ratio * sqrt(h^2 + w^2))) in float64, ties to even; 1 where that is below 1
    eroded     = 1 where the whole (2d+1) x (2d+1) window around the pixel lies inside the image and is all ones
                 (copyMakeBorder(1 px of 0) + cv2.erode(3x3 ones, iterations=d) + crop)
    boundary   = mask & ~eroded
    IoU        = min(mask IoU, IoU of the two boundaries with the same iscrowd flags), element by element

Everything else is `segm`: grouping, cuts, areas (a detection's is its mask's), match rules, accumulate and summarize come from
tests/cocoeval_oracle.py, tests/lviseval_oracle.py and tests/lvissegm_oracle.py; only the IoU of each group is replaced and the match
walked again.  The min rule and the mask area are restated from the two APIs from memory; neither API was run here."""
import numpy as np

from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo
from tests import lvissegm_oracle as so
from tests import poly_oracle as po
from tests import rle_oracle as ro


def dilation(h, w, ratio=0.02):
    d = int(round(ratio * np.sqrt(h ** 2 + w ** 2)))
    return 1 if d < 1 else d


def erode_loop(mask, d):
    """The window rule, pixel by pixel."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    out = np.zeros((h, w), np.uint8)
    for y in range(d, h - d):
        for x in range(d, w - d):
            out[y, x] = 1 if m[y - d:y + d + 1, x - d:x + d + 1].all() else 0
    return out


def erode(mask, d):
    """The window rule, window offset by window offset: a pixel whose window lies inside the image stays iff the mask is set at every one of
    the (2d+1)^2 offsets (the same as erode_loop, which tests/test_oracle_boundary.py checks; this one is quick enough for a data set)."""
    m = np.asarray(mask) != 0
    h, w = m.shape
    out = np.zeros((h, w), np.uint8)
    if h <= 2 * d or w <= 2 * d:
        return out
    inner = np.ones((h - 2 * d, w - 2 * d), bool)
    for dy in range(-d, d + 1):
        for dx in range(-d, d + 1):
            inner &= m[d + dy:h - d + dy, d + dx:w - d + dx]
    out[d:h - d, d:w - d] = inner
    return out


def boundary(mask, d):
    m = (np.asarray(mask) != 0).astype(np.uint8)
    return m & (1 - erode(m, d))


def boundary_of(mask, ratio=0.02):
    return boundary(mask, dilation(mask.shape[0], mask.shape[1], ratio))


def boundary_iou(dt, gt, iscrowd, ratio=0.02):
    """Bitmaps [D, h, w] against [G, h, w]: pycocotools' iou on the boundaries (a crowd divides by the detection's boundary area)."""
    return co.mask_iou([boundary_of(np.asarray(m), ratio) for m in dt], [boundary_of(np.asarray(m), ratio) for m in gt], iscrowd)


def combined_iou(dt, gt, iscrowd, ratio=0.02):
    return np.minimum(co.mask_iou(dt, gt, iscrowd), boundary_iou(dt, gt, iscrowd, ratio))


# ---- the two evaluations: the `segm` one, then every group's IoU replaced and its match walked again
def evaluate_coco(dataset, results, ratio=0.02):
    ev = co.evaluate(dataset, results, "segm")
    counters = co.new_counters()
    for grp in ev["groups"].values():
        dt, gt = grp["dt"], grp["gt"]
        crowd = [int(a.get("iscrowd", 0)) for a in gt]
        grp["mask_iou"] = grp["iou"]
        grp["iou"] = combined_iou([r["mask"] for r in dt], [a["mask"] for a in gt], crowd, ratio)
        grp["dt_area"] = np.asarray([so.mask_area(r["mask"]) for r in dt], np.float64)
        grp["dt_box"] = np.asarray([so.mask_box(r["mask"]) for r in dt], np.int64).reshape(-1, 4)
        for a, rng in enumerate(co.AREA_RNG):
            for t, thr in enumerate(co.IOU_THRS):
                grp["dt_match"][a, t], grp["dt_ignore"][a, t], grp["gt_match"][a, t] = co.match_group(
                    grp["iou"], grp["gt_ignore"][a], crowd, grp["dt_area"], rng, thr, counters)
    ev["counters"] = counters
    return ev


def run_coco(dataset, results, ratio=0.02):
    """-> (ev, precision, recall, the twelve statistics)."""
    ev = evaluate_coco(dataset, results, ratio)
    precision, recall, _scores = co.accumulate(ev)
    return ev, precision, recall, co.summarize(precision, recall)


def evaluate_lvis(dataset, results, ratio=0.02):
    ev = so.evaluate(dataset, results)
    counters = lo.new_counters()
    img_ids, cat_ids = ev["img_ids"], ev["cat_ids"]
    by_id = {im["id"]: im for im in dataset["images"]}
    for (k, i), grp in ev["groups"].items():
        im = by_id[img_ids[i]]
        h, w = im["height"], im["width"]
        dt, gt = grp["dt"], grp["gt"]
        grp["mask_iou"] = grp["iou"]
        grp["iou"] = combined_iou([r["mask"] for r in dt], [so.segmentation_mask(a["segmentation"], h, w) for a in gt], [0] * len(gt), ratio)
        negative = cat_ids[k] in set(im["neg_category_ids"])
        for a, rng in enumerate(lo.AREA_RNG):
            for t, thr in enumerate(lo.IOU_THRS):
                grp["dt_match"][a, t], grp["dt_ignore"][a, t], grp["gt_match"][a, t] = lo.match_group(
                    grp["iou"], grp["gt_ignore"][a], grp["dt_area"], rng, thr, grp["not_exhaustive"], negative, counters)
    ev["counters"] = counters
    return ev


def run_lvis(dataset, results, ratio=0.02):
    """-> (ev, precision, recall, results dict)."""
    ev = evaluate_lvis(dataset, results, ratio)
    precision, recall = lo.accumulate(ev)
    return ev, precision, recall, lo.summarize(precision, recall, ev["freq_groups"])


# ---- the seeded data set of tests/test_gpu_boundary.py
SIZES = {3: (30, 40), 5: (45, 60), 8: (75, 100), 13: (70, 45), 21: (100, 150)}       # d = 1, 2 (tie), 2 (tie), 2 (> 64 rows), 4
CATS = [(1, "r"), (2, "c"), (3, "f")]
POLYGON_IMAGE = 13                                                  # its ground truth is polygons where the evaluator takes them
SEED = 11


def _blob(rng, h, w, lo_=0.15, hi=0.4):
    """A filled ellipse with a wavy outline somewhere in (or over the edge of) the image: uint8 [h, w], at least 4 pixels."""
    while True:
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(lo_, hi) * h, rng.uniform(lo_, hi) * w
        y, x = np.mgrid[0:h, 0:w]
        ang = np.arctan2(y - cy, x - cx)
        r = 1 + 0.15 * np.sin(int(rng.integers(2, 7)) * ang + rng.uniform(0, 6.28))
        m = ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) <= r ** 2).astype(np.uint8)
        if m.sum() >= 4:
            return m


def _shift(mask, dy, dx):
    """The mask moved by (dy, dx); what leaves the image is lost."""
    h, w = mask.shape
    out = np.zeros_like(mask)
    out[max(dy, 0):h + min(dy, 0), max(dx, 0):w + min(dx, 0)] = mask[max(-dy, 0):h + min(-dy, 0), max(-dx, 0):w + min(-dx, 0)]
    return out


def _half(mask):
    """The first half (column-major) of the set pixels."""
    flat = np.asarray(mask).T.reshape(-1).copy()
    on = np.flatnonzero(flat)
    flat[on[on.size // 2:]] = 0
    return np.ascontiguousarray(flat.reshape(mask.shape[1], mask.shape[0]).T)


def _sliver(rng, h, w):
    """A bar one or two pixels thin: its own boundary at every d."""
    m = np.zeros((h, w), np.uint8)
    if rng.random() < 0.5:
        y = int(rng.integers(0, h - 1))
        m[y:y + int(rng.integers(1, 3)), int(rng.integers(0, w // 2)):int(rng.integers(w // 2, w + 1))] = 1
    else:
        x = int(rng.integers(0, w - 1))
        m[int(rng.integers(0, h // 2)):int(rng.integers(h // 2, h + 1)), x:x + int(rng.integers(1, 3))] = 1
    return m


def make_set(seed=SEED, polygons=False):
    """-> (dataset, results).  One data set for both evaluators: images with `height`, `width` and the LVIS fields, categories with a
    `frequency`, annotations with `mask` (the bitmap), `segmentation` (run lengths as a list of counts; polygons=True: the polygons of
    image 13 as polygons), `area`, `iscrowd` and sometimes `ignore`.  Results carry `mask`.  Detections are copies of ground truth, copies
    shifted by one to three pixels (the mask IoU stays high, the boundary IoU falls), halves, slivers and blobs of their own."""
    rng = np.random.default_rng(seed)
    anns, results = [], []
    images = {i: {"id": i, "height": h, "width": w, "neg_category_ids": [], "not_exhaustive_category_ids": []} for i, (h, w) in SIZES.items()}
    score = lambda lo_=1: float(np.float32(int(rng.integers(lo_, 21)) / 20))

    def gt(img, cat, crowd=0, ignore=None):
        h, w = SIZES[img]
        if img == POLYGON_IMAGE:
            seg = po.random_annotation(rng, h, w, int(rng.integers(1, 3)))
            m = po.annotation_mask(seg, h, w)
            if not polygons:
                seg = None
        else:
            seg, m = None, _blob(rng, h, w)
        if seg is None:
            seg = {"size": [h, w], "counts": [int(v) for v in ro.encode(m)]}
        a = {"id": len(anns) + 1, "image_id": img, "category_id": cat, "segmentation": seg, "mask": np.ascontiguousarray(m, np.uint8),
             "area": float(m.sum()), "iscrowd": crowd, "bbox": [float(v) for v in ro.bbox(m)]}
        if ignore is not None:
            a["ignore"] = ignore
        anns.append(a)
        return a["mask"]

    def dt(img, cat, mask, s):
        results.append({"image_id": img, "category_id": cat, "score": s, "mask": np.ascontiguousarray(mask, np.uint8), "bbox": [0.0, 0.0, 1.0, 1.0]})
    for img, (h, w) in SIZES.items():
        cats = [c for c, _f in CATS]
        positive = [c for c in cats if rng.random() < 0.75] or [1]
        rest = [c for c in cats if c not in positive]
        images[img]["neg_category_ids"] = [c for c in rest if rng.random() < 0.6]
        images[img]["not_exhaustive_category_ids"] = [c for c in positive if rng.random() < 0.3]
        for cat in positive:
            for _ in range(int(rng.integers(2, 4))):
                m = gt(img, cat, crowd=int(rng.random() < 0.15), ignore=1 if rng.random() < 0.1 else None)
                if rng.random() < 0.5:
                    dt(img, cat, m, score(10))
                for _ in range(int(rng.integers(1, 4))):
                    dt(img, cat, _shift(m, int(rng.integers(-3, 4)), int(rng.integers(-3, 4))), score(5))
                if rng.random() < 0.5:
                    dt(img, cat, _half(m), score())
                if rng.random() < 0.5:
                    dt(img, cat, _sliver(rng, h, w), score())
                if rng.random() < 0.7:
                    dt(img, cat, _blob(rng, h, w), score())
        for cat in rest:
            dt(img, cat, _blob(rng, h, w), score())
    dt(1000, 1, np.ones((4, 4), np.uint8), 0.5)                     # an unknown image
    dt(5, 77, _blob(rng, *SIZES[5]), 0.5)                           # an unknown category
    results = [results[j] for j in rng.permutation(len(results))]
    dataset = {"images": [images[i] for i in SIZES], "categories": [{"id": c, "frequency": f} for c, f in CATS], "annotations": anns}
    return dataset, results
