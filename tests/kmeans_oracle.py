"""The literal slow form of the anchor k-means rules (include/mi355det.h, "Anchor k-means"), for the tests only.

box_features   the feature, selection and band loop of the reference's yolo/utilities/kmeans_anchors.py:20-61 over a dataset dict.
lloyd          Lloyd's iteration exactly as the header states it, for both distances: distances element by element in float64 in the stated
               operation order (numpy's elementwise operations are the IEEE ones), the first minimum (ties to the lowest index), sums by
               math.fsum (correctly rounded, so any summation order is within its own error of them), an empty cluster keeps its centre.
kmeans         restarts and problems on top of lloyd, with the same torch.randperm initialisation as the product.
Every lloyd result carries `gap`: the smallest difference between the best and the second-best distance of any point in any pass, relative
to the largest distance of that pass - how far rounding is from flipping a label."""
import math

import numpy as np
import torch


def box_features(dataset):
    """-> features float64 [A, 4], band int8 [A], over the annotations of listed images in the file's order."""
    size = {im["id"]: (im["width"], im["height"]) for im in dataset["images"]}
    feats, band = [], []
    with np.errstate(all="ignore"):
        for ann in dataset["annotations"]:
            if ann["image_id"] not in size:
                continue
            W, H = size[ann["image_id"]]
            width = np.float64(ann["bbox"][2]) / np.float64(W)
            height = np.float64(ann["bbox"][3]) / np.float64(H)
            aspect = width / height
            area = width * height
            b = -1
            if aspect > 0.2 and aspect < 5:
                if area < 0.01:
                    b = 0
                elif area > 0.01 and area < 0.1:
                    b = 1
                elif area > 0.1:
                    b = 2
            feats.append([width, height, aspect, area])
            band.append(b)
    return np.asarray(feats, np.float64).reshape(-1, 4), np.asarray(band, np.int8)


def distances(X, C, metric):
    """float64 [N, k]: every point against every centre."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    if metric == "iou":
        w, h, cw, ch = X[:, None, 0], X[:, None, 1], C[None, :, 0], C[None, :, 1]
        i = np.minimum(w, cw) * np.minimum(h, ch)
        return 1.0 - i / (w * h + cw * ch - i)
    d = (X[:, None, 0] - C[None, :, 0]) * (X[:, None, 0] - C[None, :, 0])
    for j in range(1, X.shape[1]):
        d = d + (X[:, None, j] - C[None, :, j]) * (X[:, None, j] - C[None, :, j])
    return d


def one_pass(X, C, metric):
    """One assignment: labels, minimal distances, per-cluster counts and fsum coordinate sums, the fsum inertia, and the pass's gap."""
    X = np.asarray(X, np.float64)
    d = distances(X, C, metric)
    labels = np.argmin(d, axis=1)                              # the first minimum: ties to the lowest centre index
    dmin = d[np.arange(len(X)), labels]
    k = len(C)
    counts = np.bincount(labels, minlength=k)
    sums = np.array([[math.fsum(X[labels == c, j]) for j in range(X.shape[1])] for c in range(k)], np.float64).reshape(k, X.shape[1])
    gap = math.inf
    if k > 1:
        s = np.sort(d, axis=1)
        gap = float((s[:, 1] - s[:, 0]).min() / d.max()) if d.max() > 0 else 0.0
    return {"labels": labels, "dmin": dmin, "counts": counts, "sums": sums, "inertia": math.fsum(dmin), "gap": gap}


def lloyd(X, C0, metric="euclid", max_iter=300):
    X = np.asarray(X, np.float64)
    C = np.array(C0, np.float64)
    prev, gap, n_iter = None, math.inf, 0
    # of the pass that last moved each centre: the cluster's size and its sum of |x| per feature (0: the centre still is the initial one)
    from_count, from_abs = np.zeros(len(C), np.int64), np.zeros(C.shape, np.float64)
    while True:
        p = one_pass(X, C, metric)
        n_iter += 1
        gap = min(gap, p["gap"])
        changed = len(X) if prev is None else int((p["labels"] != prev).sum())
        prev = p["labels"]
        if changed == 0 or n_iter >= max_iter:
            break
        for c in range(len(C)):
            if p["counts"][c] > 0:                               # an empty cluster keeps its centre
                C[c] = p["sums"][c] / np.float64(p["counts"][c])
                from_count[c] = p["counts"][c]
                from_abs[c] = [math.fsum(np.abs(X[prev == c, j])) for j in range(X.shape[1])]
    return {"centers": C, "from_count": from_count, "from_abs": from_abs, "labels": prev, "counts": p["counts"], "sums": p["sums"], "inertia": p["inertia"], "n_iter": n_iter,
            "changed": changed, "gap": gap}


def seeded_init(points_per_problem, k, n_init, seed):
    """[P][R] arrays [k, F]: rows torch.randperm(N_p, generator=g)[:k] of each problem's points, problem-major, one CPU generator."""
    g = torch.Generator().manual_seed(seed)
    return [[np.asarray(Xp)[torch.randperm(len(Xp), generator=g)[:k].numpy()] for _ in range(n_init)] for Xp in points_per_problem]


def kmeans(X, k, problem=None, n_problems=1, metric="euclid", init=None, n_init=10, seed=0, max_iter=300):
    """The product's kmeans() on the host.  init: None or [P][R] arrays [k, F]."""
    X = np.asarray(X, np.float64)
    problem = np.zeros(len(X), np.int64) if problem is None else np.asarray(problem, np.int64)
    idx = [np.nonzero(problem == p)[0] for p in range(n_problems)]
    if init is None:
        init = seeded_init([X[i] for i in idx], k, n_init, seed)
    runs = [[lloyd(X[idx[p]], init[p][r], metric, max_iter) for r in range(len(init[p]))] for p in range(n_problems)]
    best = [min(range(len(rs)), key=lambda r: (rs[r]["inertia"], r)) for rs in runs]
    labels = np.full(len(X), -1, np.int64)
    for p in range(n_problems):
        labels[idx[p]] = runs[p][best[p]]["labels"]
    return {"runs": runs, "best": best, "labels": labels, "gap": min(r["gap"] for rs in runs for r in rs)}
