"""Weighted boxes fusion, the literal host form in numpy float64 (the rule of include/mi355det.h, "Weighted boxes fusion").  A cluster is a
MEMBER LIST and is recomputed from its list on every join, as the `ensemble-boxes` package does it; no running sums here, so that this form
does not copy the kernel.  Contains the candidate filter, the fusion order, the scores and the output order.  Nothing is imported from the
package under test."""
import numpy as np

DROP_REASONS = ("unknown_image", "below_skip_box_thr", "score_not_positive", "box_not_finite", "box_empty")


def overlap(F, b):
    """The rule's overlap of a fused box and a candidate, both corner arrays."""
    iw = min(F[2], b[2]) - max(F[0], b[0])
    if iw <= 0:
        return np.float64(0)
    ih = min(F[3], b[3]) - max(F[1], b[1])
    if ih <= 0:
        return np.float64(0)
    i = iw * ih
    return i / ((F[2] - F[0]) * (F[3] - F[1]) + (b[2] - b[0]) * (b[3] - b[1]) - i)


def fused_box(members, boxes, scores):
    """The fused box of a member list, recomputed from the list: a lone member's box as it is, else sum(s' * box) / sum(s') in join order."""
    if len(members) == 1:
        return boxes[members[0]].copy()
    S, C = scores[members[0]] * boxes[members[0]], scores[members[0]]
    for m in members[1:]:
        S, C = S + scores[m] * boxes[m], C + scores[m]
    return S / C


def cluster_group(boxes, scores, iou_thr):
    """One group's candidates in fusion order (boxes float64 [n, 4] corners, scores float64 [n] = s') -> (member lists in creation order,
    the fused boxes, per candidate its cluster)."""
    lists, fused, of = [], [], []
    for j in range(len(scores)):
        best, at = np.float64(0), -1
        for c, F in enumerate(fused):
            v = overlap(F, boxes[j])
            if v > best:
                best, at = v, c
        if at >= 0 and best > iou_thr:
            lists[at].append(j)
            fused[at] = fused_box(lists[at], boxes, scores)
        else:
            at = len(lists)
            lists.append([j])
            fused.append(fused_box(lists[at], boxes, scores))
        of.append(at)
    return lists, fused, of


def cluster_score(members, scores, conf_type, W, wmax):
    if conf_type == "max":
        return max(scores[m] for m in members) / wmax
    if conf_type != "avg":
        raise ValueError("conf_type")
    C = scores[members[0]]
    for m in members[1:]:
        C = C + scores[m]
    n = np.float64(len(members))
    return ((C / n) * min(n, W)) / W


def candidates(models, image_ids, weights, skip_box_thr):
    """The model-major concatenation -> per detection (image, category, s', corners) with `keep`, and the dropped counts."""
    known = set(image_ids)
    rows = [(m, r) for m, res in enumerate(models) for r in res]
    n = len(rows)
    img = np.asarray([r["image_id"] for _m, r in rows], np.int64).reshape(n)
    cat = np.asarray([r["category_id"] for _m, r in rows], np.int64).reshape(n)
    s = np.asarray([r["score"] for _m, r in rows], np.float64).reshape(n)
    box = np.asarray([r["bbox"] for _m, r in rows], np.float64).reshape(n, 4)
    w = np.asarray([weights[m] for m, _r in rows], np.float64).reshape(n)
    with np.errstate(all="ignore"):
        sp = s * w
        corners = np.stack([box[:, 0], box[:, 1], box[:, 0] + box[:, 2], box[:, 1] + box[:, 3]], 1)
        reasons = [np.asarray([i not in known for i in img.tolist()], bool).reshape(n), s < skip_box_thr, ~(np.isfinite(sp) & (sp > 0)),
                   ~(np.isfinite(box).all(1) & np.isfinite(corners).all(1)), (box[:, 2] <= 0) | (box[:, 3] <= 0)]
    keep, dropped = np.ones(n, bool), {}
    for name, r in zip(DROP_REASONS, reasons):
        dropped[name] = int((keep & r).sum())
        keep &= ~r
    return img, cat, sp, corners, keep, dropped


def groups(models, image_ids, weights, skip_box_thr):
    """-> ([(image, category, candidate indices in fusion order)], sorted by image then category; the candidates arrays; dropped)."""
    img, cat, sp, corners, keep, dropped = candidates(models, image_ids, weights, skip_box_thr)
    idx = np.flatnonzero(keep)
    idx = idx[np.argsort(-sp[idx], kind="stable")]                 # descending s', ties in model-major order
    by = {}
    for j in idx.tolist():
        by.setdefault((int(img[j]), int(cat[j])), []).append(j)
    return [(k[0], k[1], by[k]) for k in sorted(by)], (img, cat, sp, corners), dropped


def fuse(models, image_ids, weights=None, iou_thr=0.55, skip_box_thr=0.0, conf_type="avg", cluster=cluster_group):
    """models: a list of COCO result lists -> {"image_id", "category_id" int64 [K], "score" float64 [K], "box" float64 [K, 4] as
    [x, y, w, h], "members" int64 [K], "cluster_of" int64 [all detections, model-major; -1: dropped], "dropped": {reason: count}} in the
    output order: image-major, descending score, ties by category, then creation order.  `cluster`: the clustering of one group."""
    weights = [1.0] * len(models) if weights is None else [float(w) for w in weights]
    W = np.float64(weights[0])
    for w in weights[1:]:
        W = W + np.float64(w)
    wmax = np.float64(max(weights))
    gs, (img, cat, sp, corners), dropped = groups(models, image_ids, weights, skip_box_thr)
    rows, member_rows = [], []
    for image, category, idx in gs:
        lists, fused, _of = cluster(corners[idx], sp[idx], iou_thr)
        for members, F in zip(lists, fused):
            rows.append((image, category, cluster_score(members, sp[idx], conf_type, W, wmax), F, len(members)))
            member_rows.append([idx[m] for m in members])
    # rows stand image-major, category second, creation order third; a stable sort by descending score inside each image keeps the ties so
    order = sorted(range(len(rows)), key=lambda r: (rows[r][0], -rows[r][2]))
    cluster_of = -np.ones(len(img), np.int64)
    for pos, r in enumerate(order):
        cluster_of[member_rows[r]] = pos
    F = np.asarray([rows[r][3] for r in order], np.float64).reshape(-1, 4)
    return {"image_id": np.asarray([rows[r][0] for r in order], np.int64), "category_id": np.asarray([rows[r][1] for r in order], np.int64),
            "score": np.asarray([rows[r][2] for r in order], np.float64),
            "box": np.stack([F[:, 0], F[:, 1], F[:, 2] - F[:, 0], F[:, 3] - F[:, 1]], 1) if len(order) else np.zeros((0, 4)),
            "members": np.asarray([rows[r][4] for r in order], np.int64), "cluster_of": cluster_of, "dropped": dropped}
