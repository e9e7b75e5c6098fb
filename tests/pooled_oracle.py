"""AP-pool and AP-fixed (Dave et al., "Evaluating Large-Vocabulary Object Detectors: The Devil is in the Details", 2021) restated in numpy: the
reference of tests/test_gpu_pooled_ap.py, pinned by the hand-checked cases of tests/test_oracle_pooled.py.  The paper's fork of lvis-api is
not installed here: the rules are restated from memory of the paper and of that fork, as include/mi355det.h ("Pooled precision-recall") states
them.

AP-pool.  A pool is a set of categories; its list is every detection slot of those categories below the evaluator's largest cut, in descending
score, stable over the slot index.  Per (pool s, area range a, threshold t), walking the list: tp counts the slots that are matched and not
ignored, fp those unmatched and not ignored; rc = tp / npig (npig: the pool's ground truths not ignored at a); pr = tp / (fp + tp + 2^-52),
made non-increasing from the right; precision / scores [T, R, S, A] = pr and the score at the first position with rc >= rec_thrs[r], 0 past the
end; recall [T, S, A] = the last rc, 0 for an empty list; everything -1 where npig == 0.

AP-fixed.  Among the results of known images every category_id (known or not) keeps its K best (descending score, stable over the order of
arrival), then the per-image cut, if any, then the rules of tests/lviseval_oracle.py unchanged.  run_cut() parametrises that file's MAX_DETS
constant for the length of one call and puts it back."""
import sys
from collections import OrderedDict, defaultdict

import numpy as np

from tests import lviseval_oracle as lo

EPS = np.spacing(1)                       # 2^-52


def pool_list(scores, cat_of, rank, cut, cats):
    """The list of one pool: the slots (indices into `scores`) of the categories `cats` with rank < cut, descending score, stable."""
    slots = np.flatnonzero(np.isin(cat_of, np.asarray(cats, np.int64)) & (np.asarray(rank) < cut))
    return slots[np.argsort(-np.asarray(scores, np.float64)[slots], kind="mergesort")]


def _empty(T, R, S, A):
    return -np.ones((T, R, S, A), np.float64), -np.ones((T, S, A), np.float64), -np.ones((T, R, S, A), np.float64)


def pooled_loops(lists, npig, dt_score, dt_match, dt_ignore, rec_thrs):
    """The literal form.  lists: per pool its slots in list order; npig [S, A]; dt_score [ND]; dt_match, dt_ignore [A, T, ND]; rec_thrs [R]
    -> precision [T, R, S, A], recall [T, S, A], scores [T, R, S, A]."""
    A, T, _nd = dt_match.shape
    R, S = len(rec_thrs), len(lists)
    precision, recall, scores = _empty(T, R, S, A)
    for s, order in enumerate(lists):
        n = len(order)
        for a in range(A):
            if npig[s][a] == 0:
                continue
            for t in range(T):
                tp, fp = 0, 0
                rc, pr = np.zeros(n, np.float64), np.zeros(n, np.float64)
                for i, slot in enumerate(order):
                    matched, ignored = dt_match[a, t, slot] != 0, dt_ignore[a, t, slot] != 0
                    tp += 1 if (matched and not ignored) else 0
                    fp += 1 if (not matched and not ignored) else 0
                    rc[i] = np.float64(tp) / np.float64(npig[s][a])
                    pr[i] = np.float64(tp) / (np.float64(fp) + np.float64(tp) + EPS)
                recall[t, s, a] = rc[-1] if n else 0.0
                for i in range(n - 1, 0, -1):
                    if pr[i] > pr[i - 1]:
                        pr[i - 1] = pr[i]
                for r, want in enumerate(rec_thrs):
                    first = 0
                    while first < n and rc[first] < want:
                        first += 1
                    precision[t, r, s, a] = pr[first] if first < n else 0.0
                    scores[t, r, s, a] = dt_score[order[first]] if first < n else 0.0
    return precision, recall, scores


def pooled_vectorised(lists, npig, dt_score, dt_match, dt_ignore, rec_thrs):
    """pooled_loops for long lists: cumsum, reversed maximum.accumulate, searchsorted(rc, thr, "left")."""
    A, T, _nd = dt_match.shape
    R, S = len(rec_thrs), len(lists)
    precision, recall, scores = _empty(T, R, S, A)
    dt_score, rec_thrs = np.asarray(dt_score, np.float64), np.asarray(rec_thrs, np.float64)
    for s, order in enumerate(lists):
        order = np.asarray(order, np.int64)
        n = len(order)
        sc = dt_score[order]
        for a in range(A):
            if npig[s][a] == 0:
                continue
            for t in range(T):
                matched, ignored = dt_match[a, t, order] != 0, dt_ignore[a, t, order] != 0
                tp = np.cumsum(matched & ~ignored).astype(np.float64)
                fp = np.cumsum(~matched & ~ignored).astype(np.float64)
                rc = tp / np.float64(npig[s][a])
                pr = tp / (fp + tp + EPS)
                pr = np.maximum.accumulate(pr[::-1])[::-1]
                recall[t, s, a] = rc[-1] if n else 0.0
                first = np.searchsorted(rc, rec_thrs, side="left")
                inside = first < n
                precision[t, :, s, a] = np.where(inside, np.append(pr, 0.0)[first], 0.0)
                scores[t, :, s, a] = np.where(inside, np.append(sc, 0.0)[first], 0.0)
    return precision, recall, scores


def summarize(precision, recall, names=("",), iou_thrs=lo.IOU_THRS):
    """The pooled statistics as a list of (key, value): APpool, APpool50, APpool75, APpools / m / l, APpool<name> per further pool, ARpool."""
    at = lambda thr: np.isclose(iou_thrs, thr)
    out = [("APpool", lo._mean(precision[:, :, 0, 0])), ("APpool50", lo._mean(precision[at(.5)][:, :, 0, 0])),
           ("APpool75", lo._mean(precision[at(.75)][:, :, 0, 0]))]
    out += [("APpool" + "sml"[a - 1], lo._mean(precision[:, :, 0, a])) for a in (1, 2, 3)]
    out += [("APpool" + names[s], lo._mean(precision[:, :, s, 0])) for s in range(1, precision.shape[2])]
    return out + [("ARpool", lo._mean(recall[:, 0, 0]))]


# ---- the groups of a restated evaluation (tests/lviseval_oracle.py, tests/cocoeval_oracle.py) as slot arrays
def slots_of(ev):
    """Category-major, image second, each group in score order, the device's slot layout -> dict(score [ND], cat [ND], dt_match / dt_ignore
    [A, T, ND], gt_cat [NG], gt_ignore [A, NG])."""
    keys = sorted(ev["groups"])
    groups = [ev["groups"][k] for k in keys]
    A, T = 4, 10
    cat = lambda name, axis, empty: np.concatenate([g[name] for g in groups] + [empty], axis)
    return {"score": cat("scores", 0, np.zeros(0)),
            "cat": np.asarray([k for (k, _i), g in zip(keys, groups) for _ in g["dt"]], np.int64),
            "dt_match": cat("dt_match", 2, np.zeros((A, T, 0), np.int32)), "dt_ignore": cat("dt_ignore", 2, np.zeros((A, T, 0), np.uint8)),
            "gt_cat": np.asarray([k for (k, _i), g in zip(keys, groups) for _ in g["gt"]], np.int64),
            "gt_ignore": cat("gt_ignore", 1, np.zeros((A, 0), np.uint8))}


def pooled_of_groups(ev, pools, rec_thrs=lo.REC_THRS, rank=None, cut=1):
    """AP-pool of a restated evaluation for `pools` (lists of category indices); the groups hold only what the evaluator's cut kept, unless
    `rank` [ND] and `cut` say which slots to leave out."""
    f = slots_of(ev)
    rank = np.zeros(len(f["score"]), np.int64) if rank is None else rank
    lists = [pool_list(f["score"], f["cat"], rank, cut, cats) for cats in pools]
    npig = [[int(((f["gt_ignore"][a] == 0) & np.isin(f["gt_cat"], np.asarray(cats, np.int64))).sum()) for a in range(f["gt_ignore"].shape[0])]
            for cats in pools]
    return pooled_loops(lists, npig, f["score"], f["dt_match"], f["dt_ignore"], rec_thrs)


# ---- AP-fixed: the cut, round the LVIS rules
def category_cut(dataset, results, max_dets_per_cat):
    """Among the results of known images every category_id keeps its best `max_dets_per_cat` (descending score, stable over the order of
    arrival); the survivors stay in the order of arrival.  -> (results, {category_id: number removed})."""
    known = set(im["id"] for im in dataset["images"])
    by_cat = defaultdict(list)
    for j, res in enumerate(results):
        if res["image_id"] in known:
            by_cat[res["category_id"]].append(j)
    keep, removed = set(), {}
    for c, rows in by_cat.items():
        order = np.argsort(np.asarray([-float(results[j]["score"]) for j in rows], np.float64), kind="mergesort")
        keep.update(rows[o] for o in order[:max_dets_per_cat])
        removed[c] = max(len(rows) - max_dets_per_cat, 0)
    return [res for j, res in enumerate(results) if j in keep], removed


def run_cut(dataset, results, max_dets=lo.MAX_DETS, max_dets_per_cat=None):
    """lviseval_oracle.run under (max_dets, max_dets_per_cat); max_dets None or -1: no per-image cut, printed and keyed as -1.
    -> (ev, precision, recall, results dict, printed text)."""
    if max_dets_per_cat is not None:
        results, _removed = category_cut(dataset, results, max_dets_per_cat)
    shown = -1 if max_dets in (None, -1) else max_dets
    before = lo.MAX_DETS
    try:
        lo.MAX_DETS = sys.maxsize if shown == -1 else shown           # evaluate() and format_results() read the module's constant
        ev = lo.evaluate(dataset, results)
        precision, recall = lo.accumulate(ev)
        res = OrderedDict((k.replace("@300", f"@{shown}"), v) for k, v in lo.summarize(precision, recall, ev["freq_groups"]).items())
        lo.MAX_DETS = shown
        text = lo.format_results(res)
    finally:
        lo.MAX_DETS = before
    return ev, precision, recall, res, text
