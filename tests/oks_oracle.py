"""COCO keypoint evaluation restated as Python loops, with no cleverness: the reference the device evaluator is compared against
(tests/test_gpu_keypoints.py) and that tests/test_oracle_oks.py pins with hand-checked cases.  Written from the definitions as
include/mi355det.h ("COCO keypoint evaluation") and DESIGN.md 7a.2 state them (pycocotools is not installed; they restate its computeOks,
loadRes and evaluateImg from memory): the object keypoint similarity pair by pair and keypoint by keypoint with math.exp, the same
left-to-right operations and the same ascending-order sum as the kernel; a result's area and box from its keypoints; the ignore rule; the
greedy match through tests/cocoeval_oracle.match_group, which takes the ignore and the crowd flags separately; and an accumulate and
ten-line summary of its own, because the constants of cocoeval_oracle.py are the bbox ones.

Inputs are plain Python: a COCO dataset dict whose annotations carry `keypoints` (3K numbers), `bbox`, `area`, `iscrowd` and possibly
`num_keypoints`, and a list of result dicts (`image_id`, `category_id`, `score`, `keypoints`)."""
import math
from collections import defaultdict

import numpy as np

from tests.cocoeval_oracle import match_group, new_counters

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [20]
AREA_RNG = [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
SIGMAS = [v / 10 for v in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89)]
EPS = 2.0 ** -52


def variances(sigmas):
    return [(float(s) * 2) ** 2 for s in sigmas]


def oks_pair(dt_kp, gt_kp, gt_box, gt_area, vars_):
    """One detection (flat x, y[, v] per keypoint; `stride` numbers each) against one ground truth (flat x, y, v) -> its similarity."""
    K = len(vars_)
    stride = len(dt_kp) // K
    k1 = sum(1 for i in range(K) if gt_kp[3 * i + 2] > 0)
    bx, by, bw, bh = (float(v) for v in gt_box)
    x0, x1, y0, y1 = bx - bw, bx + bw * 2, by - bh, by + bh * 2
    area_eps = float(gt_area) + EPS
    total, n = 0.0, 0
    for i in range(K):
        xd, yd = float(dt_kp[stride * i]), float(dt_kp[stride * i + 1])
        if k1 > 0:
            if not gt_kp[3 * i + 2] > 0:
                continue
            dx, dy = xd - float(gt_kp[3 * i]), yd - float(gt_kp[3 * i + 1])
        else:
            dx = max(0.0, x0 - xd) + max(0.0, xd - x1)
            dy = max(0.0, y0 - yd) + max(0.0, yd - y1)
        e = (dx * dx + dy * dy) / vars_[i] / area_eps / 2
        total += math.exp(-e)
        n += 1
    return total / n


def compute_oks(dts, gts, sigmas):
    """Result dicts [D] against annotations [G] -> float64 [D, G]."""
    vars_ = variances(sigmas)
    out = np.zeros((len(dts), len(gts)), np.float64)
    for d, r in enumerate(dts):
        for g, a in enumerate(gts):
            out[d, g] = oks_pair(r["keypoints"], a["keypoints"], a["bbox"], a["area"], vars_)
    return out


def result_area_box(keypoints, K):
    """loadRes: over all K keypoints, -> (area, [x, y, w, h])."""
    stride = len(keypoints) // K
    xs = [float(keypoints[stride * i]) for i in range(K)]
    ys = [float(keypoints[stride * i + 1]) for i in range(K)]
    x0, x1, y0, y1 = min(xs), max(xs), min(ys), max(ys)
    return (x1 - x0) * (y1 - y0), [x0, y0, x1 - x0, y1 - y0]


def gt_flags(ann, K):
    """-> (ignore, crowd): ignore = iscrowd or num_keypoints == 0 (the count of v > 0 where the field is missing); crowd = iscrowd."""
    crowd = 1 if ann.get("iscrowd", 0) else 0
    nk = ann["num_keypoints"] if "num_keypoints" in ann else sum(1 for i in range(K) if ann["keypoints"][3 * i + 2] > 0)
    return (1 if (crowd or nk == 0) else 0), crowd


def evaluate(dataset, results, sigmas=None, counters=None):
    """The layout of cocoeval_oracle.evaluate with 3 area ranges: {"img_ids", "cat_ids", "groups": {(category index, image index): group},
    "counters"}; a group holds `dt` (kept, in score order), `gt`, `iou` (the similarity) [D, G], `scores`, `dt_area`, `gt_ignore` [3, G],
    `dt_match` / `dt_ignore` [3, 10, D] and `gt_match` [3, 10, G]."""
    sigmas = SIGMAS if sigmas is None else sigmas
    K = len(sigmas)
    counters = new_counters() if counters is None else counters
    img_ids = sorted(set(im["id"] for im in dataset["images"]))
    cat_ids = sorted(c["id"] for c in dataset["categories"])
    img_index = {v: i for i, v in enumerate(img_ids)}
    cat_index = {v: i for i, v in enumerate(cat_ids)}
    gts, dts = defaultdict(list), defaultdict(list)
    for ann in dataset["annotations"]:
        if ann["image_id"] in img_index and ann["category_id"] in cat_index:
            gts[(cat_index[ann["category_id"]], img_index[ann["image_id"]])].append(ann)
    for res in results:
        if res["image_id"] in img_index and res["category_id"] in cat_index:
            dts[(cat_index[res["category_id"]], img_index[res["image_id"]])].append(res)
    groups = {}
    for key in sorted(set(gts) | set(dts)):
        gt, dt = gts.get(key, []), dts.get(key, [])
        keep = np.argsort(np.asarray([-float(r["score"]) for r in dt], np.float64), kind="mergesort")[:MAX_DETS[-1]]
        dt = [dt[j] for j in keep]
        flags = [gt_flags(a, K) for a in gt]
        crowd = [c for _i, c in flags]
        iou = compute_oks(dt, gt, sigmas)
        dt_area = [result_area_box(r["keypoints"], K)[0] for r in dt]
        A, T, D, G = len(AREA_RNG), len(IOU_THRS), len(dt), len(gt)
        grp = {"dt": dt, "gt": gt, "iou": iou, "scores": np.asarray([float(r["score"]) for r in dt], np.float64), "dt_area": dt_area,
               "gt_ignore": np.zeros((A, G), np.uint8), "dt_match": np.zeros((A, T, D), np.int32), "dt_ignore": np.zeros((A, T, D), np.uint8),
               "gt_match": np.zeros((A, T, G), np.int32)}
        for a, rng in enumerate(AREA_RNG):
            for g, ann in enumerate(gt):
                grp["gt_ignore"][a, g] = 1 if (flags[g][0] or ann["area"] < rng[0] or ann["area"] > rng[1]) else 0
            for t, thr in enumerate(IOU_THRS):
                dtm, dtig, gtm = match_group(iou, grp["gt_ignore"][a], crowd, dt_area, rng, thr, counters)
                grp["dt_match"][a, t], grp["dt_ignore"][a, t], grp["gt_match"][a, t] = dtm, dtig, gtm
        groups[key] = grp
    return {"img_ids": img_ids, "cat_ids": cat_ids, "groups": groups, "counters": counters}


def accumulate(ev):
    """-> precision [10, 101, K, 3, 1], recall [10, K, 3, 1], scores [10, 101, K, 3, 1]: COCOeval.accumulate, one detection at a time."""
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(ev["cat_ids"]), len(AREA_RNG), len(MAX_DETS)
    precision = -np.ones((T, R, K, A, M), np.float64)
    recall = -np.ones((T, K, A, M), np.float64)
    scores = -np.ones((T, R, K, A, M), np.float64)
    for k in range(K):
        groups = [ev["groups"][key] for key in sorted(ev["groups"]) if key[0] == k]        # image order
        for a in range(A):
            npig = sum(int((g["gt_ignore"][a] == 0).sum()) for g in groups)
            if npig == 0:
                continue
            for m, max_det in enumerate(MAX_DETS):
                sc = np.concatenate([g["scores"][:max_det] for g in groups] + [np.zeros(0)])
                order = np.argsort(-sc, kind="mergesort")
                sc = sc[order]
                nd = len(sc)
                for t in range(T):
                    dtm = np.concatenate([g["dt_match"][a, t][:max_det] for g in groups] + [np.zeros(0, np.int32)])[order]
                    dtig = np.concatenate([g["dt_ignore"][a, t][:max_det] for g in groups] + [np.zeros(0, np.uint8)])[order]
                    tp_sum, fp_sum = 0, 0
                    rc, pr = np.zeros(nd, np.float64), np.zeros(nd, np.float64)
                    for i in range(nd):
                        tp_sum += 1 if (dtm[i] != 0 and not dtig[i]) else 0
                        fp_sum += 1 if (dtm[i] == 0 and not dtig[i]) else 0
                        rc[i] = np.float64(tp_sum) / npig
                        pr[i] = np.float64(tp_sum) / (np.float64(fp_sum) + np.float64(tp_sum) + np.spacing(1))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    first = np.searchsorted(rc, REC_THRS, side="left")      # the first index with rc >= thr, nd if there is none
                    for r, pi in enumerate(first):
                        if pi < nd:
                            precision[t, r, k, a, m], scores[t, r, k, a, m] = pr[pi], sc[pi]
                        else:
                            precision[t, r, k, a, m], scores[t, r, k, a, m] = 0.0, 0.0
    return precision, recall, scores


def _mean(x):
    x = x[x > -1]
    return np.float64(-1) if x.size == 0 else np.mean(x)


def summarize(precision, recall):
    """The ten keypoint statistics, all at maxDets = 20: AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl."""
    def stat(table, thr=None, a=0):
        s = table if thr is None else table[np.isclose(IOU_THRS, thr)]
        return _mean(s[..., a, 0])
    p, r = precision, recall
    return np.asarray([stat(p), stat(p, .5), stat(p, .75), stat(p, a=1), stat(p, a=2),
                       stat(r), stat(r, .5), stat(r, .75), stat(r, a=1), stat(r, a=2)], np.float64)


def stats(dataset, results, sigmas=None):
    precision, recall, _ = accumulate(evaluate(dataset, results, sigmas))
    return summarize(precision, recall)


def separation_violations(ev, tol=1e-9):
    """The condition under which the match arrays of two float64 routes that agree to 1e-13 must be equal: in every group's matrix no value
    lies within `tol` of min(thr, 1 - 1e-10) for any threshold, and no two unequal values of one detection's row lie within `tol` of each
    other.  -> the list of violations (empty: the condition holds)."""
    bad = []
    cuts = [min(float(t), 1 - 1e-10) for t in IOU_THRS]
    for key, g in ev["groups"].items():
        m = g["iou"]
        for d in range(m.shape[0]):
            row = np.sort(m[d])
            for x in row:
                if any(abs(float(x) - c) <= tol for c in cuts):
                    bad.append((key, d, "threshold", float(x)))
            gaps = np.diff(row)
            if ((gaps > 0) & (gaps <= tol)).any():
                bad.append((key, d, "row", None))
    return bad
