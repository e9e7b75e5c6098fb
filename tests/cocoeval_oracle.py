"""The COCO evaluation rules restated in numpy, with loops and no cleverness: the reference the device evaluator is compared against bit for bit
(tests/test_gpu_cocoeval.py) and that tests/test_oracle_cocoeval.py pins with hand-checked cases.  Written from the definitions: box and
mask IoU as pycocotools' maskUtils.iou defines them, the greedy match of COCOeval.evaluateImg, the precision/recall tables of
COCOeval.accumulate and the twelve numbers of COCOeval.summarize.

Inputs are plain Python: a COCO dataset dict (`images`, `annotations`, `categories`) and a list of result dicts (`image_id`, `category_id`,
`score`, `bbox`).  For `segm` every annotation and every result additionally carries `mask`, a uint8 bitmap [H, W]."""
from collections import defaultdict

import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
BRANCHES = ("crowd_rematch", "ignore_stop", "iou_equals_threshold", "equal_iou_takeover")


def new_counters():
    return {b: 0 for b in BRANCHES}


def bb_iou(dt, gt, iscrowd):
    """[D, 4] against [G, 4] boxes [x, y, w, h] -> float64 [D, G]."""
    dt = np.asarray(dt, np.float64).reshape(-1, 4)
    gt = np.asarray(gt, np.float64).reshape(-1, 4)
    out = np.zeros((dt.shape[0], gt.shape[0]), np.float64)
    for d in range(dt.shape[0]):
        dx, dy, dw, dh = dt[d]
        da = dw * dh
        for g in range(gt.shape[0]):
            gx, gy, gw, gh = gt[g]
            ga = gw * gh
            w = min(dx + dw, gx + gw) - max(dx, gx)
            if w <= 0:
                continue
            h = min(dy + dh, gy + gh) - max(dy, gy)
            if h <= 0:
                continue
            i = w * h
            u = da if iscrowd[g] else da + ga - i
            out[d, g] = i / u
    return out


def mask_iou(dt, gt, iscrowd):
    """uint8 bitmaps [D, H, W] against [G, H, W] -> float64 [D, G]."""
    out = np.zeros((len(dt), len(gt)), np.float64)
    for d in range(len(dt)):
        a = np.asarray(dt[d]) != 0
        for g in range(len(gt)):
            b = np.asarray(gt[g]) != 0
            i = int((a & b).sum())
            if i == 0:
                continue
            u = int(a.sum()) if iscrowd[g] else int((a | b).sum())
            out[d, g] = np.float64(i) / np.float64(u)
    return out


def match_group(iou, gt_ignore, gt_crowd, dt_area, area_rng, thr, counters):
    """One group, one area range, one threshold.  -> dt_match [D] (ground truth index + 1, or 0), dt_ignore [D], gt_match [G]."""
    D, G = iou.shape
    order = np.argsort(np.asarray(gt_ignore, np.int64), kind="mergesort")          # non-ignored first, annotation order within
    dtm, dtig, gtm = np.zeros(D, np.int32), np.zeros(D, np.uint8), np.zeros(G, np.int32)
    for d in range(D):
        best = min(thr, 1 - 1e-10)
        m = -1
        for g in order:
            if gtm[g] > 0:
                if not gt_crowd[g]:
                    continue
                counters["crowd_rematch"] += 1
            if m > -1 and not gt_ignore[m] and gt_ignore[g]:
                counters["ignore_stop"] += 1
                break
            if iou[d, g] < best:
                continue
            if iou[d, g] == best:
                counters["iou_equals_threshold" if m == -1 else "equal_iou_takeover"] += 1
            best = iou[d, g]
            m = int(g)
        if m > -1:
            dtm[d] = m + 1
            dtig[d] = gt_ignore[m]
            gtm[m] = d + 1
    for d in range(D):
        if dtm[d] == 0 and (dt_area[d] < area_rng[0] or dt_area[d] > area_rng[1]):
            dtig[d] = 1
    return dtm, dtig, gtm


def evaluate(dataset, results, iou_type="bbox", counters=None):
    """-> {"img_ids", "cat_ids", "groups": {(category index, image index): group}, "counters"}; a group holds `dt` (the results kept, in score
    order), `gt`, `iou` [D, G], `scores` [D], `gt_ignore` [4, G], `dt_match` / `dt_ignore` [4, 10, D] and `gt_match` [4, 10, G]."""
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
        crowd = [int(a.get("iscrowd", 0)) for a in gt]
        if iou_type == "bbox":
            iou = bb_iou([r["bbox"] for r in dt], [a["bbox"] for a in gt], crowd)
            dt_area = [np.float64(r["bbox"][2]) * np.float64(r["bbox"][3]) for r in dt]
        else:
            iou = mask_iou([r["mask"] for r in dt], [a["mask"] for a in gt], crowd)
            dt_area = [np.float64(int((np.asarray(r["mask"]) != 0).sum())) for r in dt]
        A, T, D, G = len(AREA_RNG), len(IOU_THRS), len(dt), len(gt)
        grp = {"dt": dt, "gt": gt, "iou": iou, "scores": np.asarray([float(r["score"]) for r in dt], np.float64),
               "gt_ignore": np.zeros((A, G), np.uint8), "dt_match": np.zeros((A, T, D), np.int32), "dt_ignore": np.zeros((A, T, D), np.uint8),
               "gt_match": np.zeros((A, T, G), np.int32)}
        for a, rng in enumerate(AREA_RNG):
            for g, ann in enumerate(gt):
                grp["gt_ignore"][a, g] = 1 if (crowd[g] or ann["area"] < rng[0] or ann["area"] > rng[1]) else 0
            for t, thr in enumerate(IOU_THRS):
                dtm, dtig, gtm = match_group(iou, grp["gt_ignore"][a], crowd, dt_area, rng, thr, counters)
                grp["dt_match"][a, t], grp["dt_ignore"][a, t], grp["gt_match"][a, t] = dtm, dtig, gtm
        groups[key] = grp
    return {"img_ids": img_ids, "cat_ids": cat_ids, "groups": groups, "counters": counters}


def accumulate(ev):
    """-> precision [10, 101, K, 4, 3], recall [10, K, 4, 3], scores [10, 101, K, 4, 3]."""
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
    """The twelve COCO statistics as a float64 array."""
    def ap(thr=None, a=0, m=2):
        p = precision if thr is None else precision[np.isclose(IOU_THRS, thr)]
        return _mean(p[:, :, :, a, m])

    def ar(a=0, m=2):
        return _mean(recall[:, :, a, m])
    return np.asarray([ap(), ap(.5), ap(.75), ap(a=1), ap(a=2), ap(a=3), ar(m=0), ar(m=1), ar(m=2), ar(a=1), ar(a=2), ar(a=3)], np.float64)


def stats(dataset, results, iou_type="bbox"):
    precision, recall, _ = accumulate(evaluate(dataset, results, iou_type))
    return summarize(precision, recall)
