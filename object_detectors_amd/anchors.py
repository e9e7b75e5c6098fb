"""The anchor list of a dataset from its annotations, on the device (csrc/kmeans_kernels.hip; include/mi355det.h, "Anchor k-means").

The reference's LVIS recipe trains with six anchors per scale (yolo/hydra/dataset/lvis.yaml): three centres that
yolo/utilities/kmeans_anchors.py found in the training boxes - Euclidean k-means on (width, height, aspect, area) in three area bands, with
lvis, pandas, tqdm and scikit-learn - in front of the stock three.  Here:

    found = reference_anchors("lvis_v1_train.json", "lvis", 416)            # the script's rule: 3 bands x k = 3, ten restarts, one sweep per pass
    anchors = extend_anchors(STOCK_ANCHORS, found["anchors"])               # the layout of lvis.yaml: YOLOForw(anchors=anchors, ...)
    yolo = iou_anchors("instances_train2017.json", "coco", 416, k=9)        # what YOLO users expect: k-means on (w, h) under 1 - IoU
    fitness(wh, yolo["anchors"])                                            # mean best IoU, share of boxes with a best IoU >= 0.5

Lloyd's iteration is batched over problems (bands) and restarts: a pass reads every point once.  Tensors must live on the GPU and nothing falls
back to torch ops.  One deviation from scikit-learn: an empty cluster keeps its centre (scikit-learn relocates it)."""
import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr
from .dataset_stats import listed_annotations, load_dataset

METRICS = {"euclid": 0, "iou": 1}
# the nine anchors of the reference's coco.yaml, scale 0 (the coarsest grid, the largest boxes) first
STOCK_ANCHORS = [[[116, 90], [156, 198], [373, 326]], [[30, 61], [62, 45], [59, 119]], [[10, 13], [16, 30], [33, 23]]]


def limits():
    """{'problems', 'restarts', 'k', 'features', 'assign_k', 'points_per_workgroup'} of the library (mi355det_kmeans_limit)."""
    L = _lib.lib()
    names = ("problems", "restarts", "k", "features", "assign_k", "points_per_workgroup")
    return {n: int(L.mi355det_kmeans_limit(i)) for i, n in enumerate(names)}


# the limits restated for the refusals that must not need the library (tests/test_anchors_host.py compares them with limits() on the GPU)
MAX_PROBLEMS, MAX_RESTARTS, MAX_K, MAX_FEATURES, MAX_ASSIGN_K = 4, 16, 16, 4, 64


def box_arrays(dataset, dset_name="coco"):
    """A COCO or LVIS annotation dict (or the path of its JSON) -> {'box_wh': float64 numpy [A, 2] = (bbox[2], bbox[3]), 'image_index': int32
    [A], 'image_size': int32 [n_images, 2] = (width, height), 'n_images'}: one row per annotation of a listed image, in the file's order
    (annotations of an image id that `images` does not list are dropped, as dataset_stats.dataset_arrays does).  ValueError if none is left."""
    dataset = load_dataset(dataset)
    if dset_name not in ("coco", "lvis"):
        raise ValueError("dset_name must be 'coco' or 'lvis'")
    img_ids, keep, pos = listed_annotations(dataset)
    if pos.size == 0:
        raise ValueError("box_arrays: no annotation of a listed image, nothing to cluster")
    size = np.zeros((img_ids.size, 2), np.int32)
    for im in dataset["images"]:
        size[np.searchsorted(img_ids, int(im["id"]))] = (int(im["width"]), int(im["height"]))
    wh = np.asarray([(a["bbox"][2], a["bbox"][3]) for a in dataset["annotations"]], dtype=np.float64).reshape(-1, 2)[keep]
    return {"box_wh": wh, "image_index": pos.astype(np.int32), "image_size": size, "n_images": int(img_ids.size)}


def box_features(dataset_or_arrays, dset_name="coco", device="cuda"):
    """mi355det_box_features: {'features': float64 [A, 4] = (width, height, aspect, area) of kmeans_anchors.py:20-49, 'band': int8 [A] (0 small,
    1 medium, 2 large, -1 dropped or on a band edge), 'keep': bool [A] (0.2 < aspect < 5), 'n_images'}, tensors on `device`.  Takes what
    box_arrays takes, or its result."""
    a = dataset_or_arrays
    if not (isinstance(a, dict) and "box_wh" in a):
        a = box_arrays(a, dset_name)
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("box_features needs a CUDA/HIP device (no CPU fallback)")
    wh = torch.as_tensor(a["box_wh"]).to(device=dev, dtype=torch.float64).contiguous()
    idx = torch.as_tensor(a["image_index"]).to(device=dev, dtype=torch.int32).contiguous()
    size = torch.as_tensor(a["image_size"]).to(device=dev, dtype=torch.int32).contiguous()
    if wh.dim() != 2 or wh.shape[1] != 2 or idx.shape != wh.shape[:1] or size.dim() != 2 or size.shape[1] != 2 or wh.shape[0] == 0:
        raise ValueError("box_features: box_wh [A, 2], image_index [A], image_size [n_images, 2] expected, A > 0")
    A = int(wh.shape[0])
    feats = torch.empty((A, 4), dtype=torch.float64, device=dev)
    band = torch.empty(A, dtype=torch.int8, device=dev)
    errors = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().mi355det_box_features(ptr(wh), ptr(idx), ptr(size), A, int(size.shape[0]), ptr(feats), ptr(band), ptr(errors),
                                               stream_ptr()), "box_features")
    bad = int(errors.item())
    if bad:
        raise ValueError(f"box_features: {bad} annotation(s) with an image index outside [0, {int(size.shape[0])})")
    keep = (feats[:, 2] > 0.2) & (feats[:, 2] < 5)
    return {"features": feats, "band": band, "keep": keep, "n_images": int(size.shape[0])}


def _points(X, what):
    if not (torch.is_tensor(X) and X.is_cuda):
        raise ValueError(f"{what} needs CUDA/HIP tensors (no CPU fallback)")
    if X.dtype != torch.float64 or X.dim() != 2:
        raise ValueError(f"{what}: float64 points [N, F] expected")
    if not 1 <= X.shape[1] <= MAX_FEATURES:
        raise ValueError(f"{what}: 1 to {MAX_FEATURES} features")
    if X.shape[0] == 0:
        raise ValueError(f"{what}: no points")
    return X.contiguous()


def _metric(metric, F, what):
    if metric not in METRICS:
        raise ValueError(f"{what}: metric must be 'euclid' or 'iou'")
    if metric == "iou" and F != 2:
        raise ValueError(f"{what}: the iou distance takes (w, h) points, F = 2")
    return METRICS[metric]


def _problem(problem, n_problems, X, what):
    n_problems = int(n_problems)
    if not 1 <= n_problems <= MAX_PROBLEMS:
        raise ValueError(f"{what}: 1 to {MAX_PROBLEMS} problems")
    if problem is None:
        if n_problems != 1:
            raise ValueError(f"{what}: n_problems > 1 needs a problem index per point")
        return None, n_problems
    if not (torch.is_tensor(problem) and problem.is_cuda):
        raise ValueError(f"{what} needs CUDA/HIP tensors (no CPU fallback)")
    if problem.dim() != 1 or problem.shape[0] != X.shape[0] or problem.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64):
        raise ValueError(f"{what}: one integer problem index per point")
    if problem.dtype != torch.int8:
        problem = problem.clamp(-1, 127)
    return problem.to(torch.int8).contiguous(), n_problems


def _check_points(X, problem, P, metric_id, what):
    errors = torch.empty(2, dtype=torch.int32, device=X.device)
    with torch.cuda.device(X.device):
        check(_lib.lib().mi355det_kmeans_check(ptr(X), ptr(problem), int(X.shape[0]), P, int(X.shape[1]), metric_id, ptr(errors), stream_ptr()),
              "kmeans_check")
    bad, outside = (int(v) for v in errors.tolist())
    if outside:
        raise ValueError(f"{what}: {outside} point(s) with a problem index >= {P}")
    if bad:
        raise ValueError(f"{what}: {bad} point(s) with a non-finite feature" + (" or a non-positive width or height" if metric_id else ""))


def assign(X, centers, *, problem=None, metric="euclid"):
    """mi355det_kmeans_assign: the nearest centre of every point (ties to the lowest index) and its distance.  centers float64 [P, k, F] or
    [k, F]; -> labels int32 [N] (-1 for a point with problem < 0), distance float64 [N]."""
    X = _points(X, "assign")
    metric_id = _metric(metric, X.shape[1], "assign")
    if not (torch.is_tensor(centers) and centers.is_cuda and centers.dtype == torch.float64):
        raise ValueError("assign: float64 CUDA/HIP centres expected")
    if centers.dim() == 2:
        centers = centers[None]
    if centers.dim() != 3 or centers.shape[2] != X.shape[1] or not 1 <= centers.shape[1] <= MAX_ASSIGN_K:
        raise ValueError(f"assign: centres [P, k, F] with F = {X.shape[1]} and k <= {MAX_ASSIGN_K} expected")
    problem, P = _problem(problem, centers.shape[0], X, "assign")
    centers = centers.contiguous()
    N = int(X.shape[0])
    labels = torch.empty(N, dtype=torch.int32, device=X.device)
    dist = torch.empty(N, dtype=torch.float64, device=X.device)
    with torch.cuda.device(X.device):
        check(_lib.lib().mi355det_kmeans_assign(ptr(X), ptr(problem), N, P, int(centers.shape[1]), int(X.shape[1]), metric_id, ptr(centers),
                                                ptr(labels), ptr(dist), stream_ptr()), "kmeans_assign")
    return labels, dist


def seeded_rows(counts, k, n_init, seed):
    """The seeded initialisation: per (problem, restart), problem-major, the first k entries of torch.randperm(N_p, generator=g) with
    g = torch.Generator().manual_seed(seed) on the CPU -> int64 [P, R, k] row numbers within each problem's points."""
    g = torch.Generator().manual_seed(int(seed))
    return torch.stack([torch.stack([torch.randperm(int(n), generator=g)[:k] for _ in range(n_init)]) for n in counts])


def kmeans(X, k, *, problem=None, n_problems=1, metric="euclid", init=None, n_init=10, seed=0, max_iter=300, check_every=8):
    """Lloyd's k-means of float64 device points X [N, F], for n_problems disjoint point sets (problem int [N]: a point's set, < 0 = takes
    part in nothing) and n_init restarts each, all in one sweep of X per pass.  init: None (seeded_rows picks rows of each problem's
    points in their stored order) or float64 [P, R, k, F].  The host enqueues check_every passes, reads one flag, and repeats up to max_iter.
    -> {'centers' [P, k, F], 'labels' int32 [N] (-1 where problem < 0), 'counts' int32 [P, k], 'inertia' [P]: the restart with the lowest
        inertia (ties to the lowest restart), 'best' int64 [P];
        'all_centers' [P, R, k, F], 'all_counts' [P, R, k], 'all_inertia' [P, R], 'n_iter' int32 [P, R], and of every restart's last pass
        'all_sums' [P, R, k, F] and 'changed' int32 [P, R]}."""
    X = _points(X, "kmeans")
    N, F = int(X.shape[0]), int(X.shape[1])
    metric_id = _metric(metric, F, "kmeans")
    k, max_iter, check_every = int(k), int(max_iter), int(check_every)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"kmeans: 1 <= k <= {MAX_K}")
    if max_iter < 1 or check_every < 1:
        raise ValueError("kmeans: max_iter and check_every must be positive")
    problem, P = _problem(problem, n_problems, X, "kmeans")
    if init is not None:
        if not (torch.is_tensor(init) and init.dtype == torch.float64 and init.dim() == 4 and init.shape[0] == P and init.shape[2] == k
                and init.shape[3] == F and 1 <= init.shape[1] <= MAX_RESTARTS):
            raise ValueError(f"kmeans: init must be float64 [{P}, R <= {MAX_RESTARTS}, {k}, {F}]")
        R = int(init.shape[1])
    else:
        R = int(n_init)
        if not 1 <= R <= MAX_RESTARTS:
            raise ValueError(f"kmeans: 1 <= n_init <= {MAX_RESTARTS}")
    dev = X.device
    _check_points(X, problem, P, metric_id, "kmeans")
    rows = [None] if problem is None else [torch.nonzero(problem == p).flatten() for p in range(P)]
    counts = [N] if problem is None else [int(r.numel()) for r in rows]
    for p, n in enumerate(counts):
        if n < k:
            raise ValueError(f"kmeans: problem {p} has {n} point(s), fewer than k = {k}")
    if init is None:
        sel = seeded_rows(counts, k, R, seed).to(dev)
        centers = torch.stack([X[sel[p]] if rows[p] is None else X[rows[p][sel[p]]] for p in range(P)]).contiguous()
    else:
        centers = init.to(dev).contiguous().clone()
        if not bool(torch.isfinite(centers).all()):
            raise ValueError("kmeans: non-finite init")
    L = _lib.lib()
    ws_bytes = int(L.mi355det_kmeans_workspace(N, P, R, k, F))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    sums = torch.zeros((P, R, k, F), dtype=torch.float64, device=dev)
    all_counts = torch.zeros((P, R, k), dtype=torch.int32, device=dev)
    inertia = torch.zeros((P, R), dtype=torch.float64, device=dev)
    n_iter = torch.empty((P, R), dtype=torch.int32, device=dev)
    changed = torch.zeros((P, R), dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.mi355det_kmeans_begin(N, P, R, k, F, ptr(n_iter), ptr(status), ptr(ws), ws_bytes, stream_ptr()), "kmeans_begin")
        enqueued = 0
        while enqueued < max_iter:
            n = min(check_every, max_iter - enqueued)
            check(L.mi355det_kmeans_passes(ptr(X), ptr(problem), N, P, R, k, F, metric_id, max_iter, n, ptr(centers), ptr(sums), ptr(all_counts),
                                           ptr(inertia), ptr(n_iter), ptr(changed), ptr(status), ptr(ws), ws_bytes, stream_ptr()), "kmeans_passes")
            enqueued += n
            if int(status.item()) >= P * R:
                break
    host_inertia = inertia.cpu().tolist()
    best = torch.tensor([min(range(R), key=lambda r: (row[r], r)) for row in host_inertia], dtype=torch.int64, device=dev)
    pick = torch.arange(P, device=dev)
    win = centers[pick, best].contiguous()
    labels, _ = assign(X, win, problem=problem, metric=metric)
    return {"centers": win, "labels": labels, "counts": all_counts[pick, best], "inertia": inertia[pick, best], "best": best,
            "all_centers": centers, "all_counts": all_counts, "all_inertia": inertia, "n_iter": n_iter, "all_sums": sums, "changed": changed}


def anchor_lists(centers_wh, inp_dim):
    """[[w, h], ...] in units of 1 / inp_dim -> [[w * inp_dim, h * inp_dim], ...] as plain floats, in the given order."""
    return [[float(w) * inp_dim, float(h) * inp_dim] for w, h in centers_wh]


def reference_anchors(dataset, dset_name="coco", inp_dim=416, k=3, **kmeans_args):
    """The rule of kmeans_anchors.py: the selected boxes (0.2 < aspect < 5) in three area bands, Euclidean k-means with k centres on
    (width, height, aspect, area) per band.  -> {'centers': float64 [3, k, 4] (band 0 = small), 'anchors': the nested list of the hydra
    dataset files, scale 0 = the large band, scale 2 = the small band, each entry [w * inp_dim, h * inp_dim] in cluster order, plus the
    fields of kmeans()}."""
    if kmeans_args.get("metric", "euclid") != "euclid":
        raise ValueError("reference_anchors: the script's rule is Euclidean; iou_anchors clusters under the iou distance")
    f = dataset if isinstance(dataset, dict) and "features" in dataset else box_features(dataset, dset_name)
    out = kmeans(f["features"], k, problem=f["band"], n_problems=3, **kmeans_args)
    centers = out["centers"].cpu().numpy()
    out["anchors"] = [anchor_lists(centers[band][:, :2], inp_dim) for band in (2, 1, 0)]
    return out


def split_anchors(centers_wh, inp_dim, scales=3):
    """Centres [k, 2] (w, h) in units of 1 / inp_dim -> the nested anchor list: ordered by descending area w * h (ties keep the given
    order) and split evenly over `scales`, scale 0 taking the largest."""
    c = np.asarray(centers_wh, dtype=np.float64).reshape(-1, 2)
    scales = int(scales)
    if scales < 1 or c.shape[0] == 0 or c.shape[0] % scales:
        raise ValueError(f"split_anchors: {c.shape[0]} centres do not split evenly over {scales} scales")
    order = np.argsort(-(c[:, 0] * c[:, 1]), kind="stable")
    per = c.shape[0] // scales
    return [anchor_lists(c[order[s * per:(s + 1) * per]], inp_dim) for s in range(scales)]


def iou_anchors(dataset, dset_name="coco", inp_dim=416, k=9, scales=3, **kmeans_args):
    """k-means on (w, h) of the selected boxes under the 1 - IoU distance -> kmeans()'s fields plus 'anchors' (split_anchors) and 'wh'
    (the selected boxes, float64 [M, 2] in units of 1 / inp_dim)."""
    if int(scales) < 1 or int(k) % int(scales):
        raise ValueError(f"iou_anchors: k = {k} does not split evenly over {scales} scales")
    if kmeans_args.setdefault("metric", "iou") != "iou":
        raise ValueError("iou_anchors clusters under the iou distance")
    f = dataset if isinstance(dataset, dict) and "features" in dataset else box_features(dataset, dset_name)
    wh = f["features"][f["keep"]][:, :2].contiguous()
    out = kmeans(wh, k, **kmeans_args)
    out["anchors"] = split_anchors(out["centers"][0].cpu().numpy(), inp_dim, scales)
    out["wh"] = wh
    return out


def extend_anchors(base, extra):
    """extra[s] + base[s] per scale: how the reference's lvis.yaml puts its three found centres in front of the stock three."""
    if len(base) != len(extra):
        raise ValueError("extend_anchors: one list per scale in both")
    return [[list(a) for a in e] + [list(a) for a in b] for b, e in zip(base, extra)]


def fitness(wh, anchors, threshold=0.5):
    """(mean over boxes of the best (w, h)-IoU over all anchors, share of boxes whose best IoU >= threshold).  wh float64 device [N, 2];
    anchors: a nested per-scale list or [M, 2], in wh's units.  From mi355det_kmeans_assign with the iou distance."""
    wh = _points(wh, "fitness")
    a = torch.as_tensor(np.asarray([p for s in anchors for p in s] if isinstance(anchors, (list, tuple)) and np.ndim(anchors) == 3 else
                                   (anchors.cpu().numpy() if torch.is_tensor(anchors) else anchors), dtype=np.float64).reshape(-1, 2))
    if not 1 <= a.shape[0] <= MAX_ASSIGN_K:
        raise ValueError(f"fitness: 1 to {MAX_ASSIGN_K} anchors")
    if not bool((a > 0).all()):
        raise ValueError("fitness: anchors must be positive")
    _check_points(wh, None, 1, METRICS["iou"], "fitness")
    _, dist = assign(wh, a.to(wh.device), metric="iou")
    best = 1.0 - dist
    return float(best.mean()), float((best >= threshold).double().mean())
