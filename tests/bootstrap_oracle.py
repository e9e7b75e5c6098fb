"""Bootstrap replicates of the COCO / LVIS accumulate pass, restated twice on the `ev["groups"]` of tests/cocoeval_oracle.py and
tests/lviseval_oracle.py (kind "coco" / "lvis"); the device code (object_detectors_amd/csrc/bootstrap_kernels.hip) is compared against both.

A replicate is one row `w` of non-negative integer weights, one per image: the evaluation of the data set in which image i occurs w[i] times.

  replicated(ev, w, kind)   the definition, literally: every group of image i is repeated w[i] times, the copies adjacent in image order, and
                            the existing accumulate() of the kind runs on the result.  Pure Python loops: for a handful of rows.
  weighted(ev, W, kind)     the closed form in numpy, for all rows of W at once: tp and fp advance by the slot's weight, rc and pr are taken at
                            the end of each slot with accumulate()'s float64 expressions, running maximum from the right, searchsorted 'left'.
                            A slot of weight 0 is not dropped but advances nothing, which gives the same tables: its rc equals that of the
                            slot before it, so it is never the first to reach a threshold, except in front of the first kept slot, where its
                            envelope is the first kept slot's.  With no kept slot at all pr[0] = 0 / 2^-52 = 0: precision 0, recall 0.

The two differ only where two kept detections of one group have equal scores and different flags (tests/test_oracle_bootstrap.py pins it).
Both return precision [T, R, K, A, M] and recall [T, K, A, M] per row (M = 1 for LVIS); weighted() adds ap_sum and the statistics."""
import numpy as np

from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo

T, R, A = len(co.IOU_THRS), len(co.REC_THRS), len(co.AREA_RNG)


def max_dets_of(kind):
    return list(co.MAX_DETS) if kind == "coco" else [None]              # None: no cut


def replicated(ev, w, kind="coco"):
    """-> precision [T, R, K, A, M], recall [T, K, A, M] of the literally replicated data set."""
    w = np.asarray(w, np.int64)
    assert w.shape == (len(ev["img_ids"]),) and (w >= 0).all()
    start = np.concatenate([[0], np.cumsum(w)])
    groups = {}
    for (k, i), g in ev["groups"].items():
        for j in range(int(w[i])):
            groups[(k, int(start[i]) + j)] = g
    rep = dict(ev, img_ids=list(range(int(start[-1]))), groups=groups)
    if kind == "coco":
        precision, recall, _scores = co.accumulate(rep)
        return precision, recall
    precision, recall = lo.accumulate(dict(rep, counters=lo.new_counters()))
    return precision[..., None], recall[..., None]


def ap_sum_of(precision, recall):
    """precision [..., T, R, K, A, M] -> the sum over R, added one threshold at a time from the highest recall threshold down; -1 where the
    cell has no ground truth (recall == -1)."""
    s = np.zeros(recall.shape, np.float64)
    for r in range(R - 1, -1, -1):
        s = s + precision[..., :, r, :, :, :]
    return np.where(recall == -1, -1.0, s)


def stats_of(precision, recall, ev, kind):
    """pycocotools' / lvis-api's summary of one replicate's tables: float64 [12] or [13]."""
    if kind == "coco":
        return co.summarize(precision, recall)
    return np.asarray(list(lo.summarize(precision[..., 0], recall[..., 0], ev["freq_groups"]).values()), np.float64)


def weighted(ev, W, kind="coco"):
    """The closed form for every row of W [B, images] (or one row [images]) -> {"precision" [B, T, R, K, A, M], "recall" [B, T, K, A, M],
    "ap_sum" [B, T, K, A, M], "stats" [B, 12 or 13]}."""
    W = np.asarray(W, np.int64)
    W = W[None] if W.ndim == 1 else W
    assert W.shape[1] == len(ev["img_ids"]) and (W >= 0).all()
    B, K, cuts = W.shape[0], len(ev["cat_ids"]), max_dets_of(kind)
    M = len(cuts)
    precision = -np.ones((B, T, R, K, A, M), np.float64)
    recall = -np.ones((B, T, K, A, M), np.float64)
    thr = co.REC_THRS
    for k in range(K):
        keys = [key for key in sorted(ev["groups"]) if key[0] == k]                    # image order
        groups = [ev["groups"][key] for key in keys]
        for a in range(A):
            npig = np.zeros(B, np.int64)
            for key, g in zip(keys, groups):
                npig += W[:, key[1]] * int((g["gt_ignore"][a] == 0).sum())
            live = npig > 0
            if not live.any():
                continue
            for m, cut in enumerate(cuts):
                sc = np.concatenate([g["scores"][:cut] for g in groups] + [np.zeros(0)])
                image = np.concatenate([np.full(len(g["scores"][:cut]), key[1], np.int64) for key, g in zip(keys, groups)] + [np.zeros(0, np.int64)])
                order = np.argsort(-sc, kind="mergesort")
                nd = len(sc)
                dtm = np.concatenate([g["dt_match"][a][:, :cut] for g in groups] + [np.zeros((T, 0), np.int32)], 1)[:, order]      # [T, nd]
                dtig = np.concatenate([g["dt_ignore"][a][:, :cut] for g in groups] + [np.zeros((T, 0), np.uint8)], 1)[:, order]
                wv = W[:, image[order]]                                               # [B, nd]
                if nd == 0:
                    precision[live, :, :, k, a, m], recall[live, :, k, a, m] = 0.0, 0.0
                    continue
                tp = np.cumsum(wv[:, None, :] * ((dtm != 0) & (dtig == 0))[None], 2).astype(np.float64)         # [B, T, nd]: exact integers
                fp = np.cumsum(wv[:, None, :] * ((dtm == 0) & (dtig == 0))[None], 2).astype(np.float64)
                with np.errstate(divide="ignore", invalid="ignore"):
                    rc = tp / npig.astype(np.float64)[:, None, None]
                pr = tp / (fp + tp + np.spacing(1))
                pr = np.maximum.accumulate(pr[:, :, ::-1], 2)[:, :, ::-1]
                first = (rc[:, :, :, None] < thr[None, None, None, :]).sum(2)          # rc never falls: searchsorted(rc, thr, 'left')
                value = np.take_along_axis(pr, np.minimum(first, nd - 1), 2)
                value = np.where(first < nd, value, 0.0)                               # [B, T, R]
                precision[live, :, :, k, a, m] = value[live]
                recall[live, :, k, a, m] = rc[live, :, -1]
    out = {"precision": precision, "recall": recall, "ap_sum": ap_sum_of(precision, recall)}
    out["stats"] = np.stack([stats_of(precision[b], recall[b], ev, kind) for b in range(B)])
    return out
