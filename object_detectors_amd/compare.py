"""Model comparison on the device: which ground-truth instances two result sets get right (the 2 x 2 contingency table and McNemar's test of
the reference's notebooks/get_disagreement.py) and the twelve COCO statistics per category (its notebooks/get_map.py), without pycocotools,
torchvision or statsmodels.

    d = Disagreement(gt)                      ground truth per image: EVERY annotation of the image in dataset order (any category, crowd or
                                              not), as the notebook takes them
    d.add(model, ...) / d.add_results(model, results)      model 0 is the notebook's baseline, model 1 its second experiment
    d.run(iou_threshold, confidence)          torch filters and sorts (plumbing) -> mi355det_box_disagreement (csrc/compare_kernels.hip,
                                              include/mi355det.h "Model comparison") -> four sums, one host read
    d.report(alpha)                           the table, McNemar's test and the verdict line

An instance is right for a model when the detection with the best class-agnostic box overlap reaches the threshold and carries the instance's
label.  An image counts only if it has an annotation and both models keep a detection on it (the notebook's `except IndexError` path);
every other image adds one to `missed`.

Beyond the notebooks: bootstrap_weights / interval / paired_bootstrap turn the replicates of COCOEval.bootstrap and LVISEval.bootstrap
(resampled images, all replicates in one kernel) into percentile intervals and a paired test on AP itself.

Deviations from the notebooks, both deliberate: mcnemar(0, 0) returns (0.0, 1.0) where the bare formula divides by zero, and
per_category_table returns the chosen metric columns where get_map.py:59-60 reads stats[position in the list]."""
import math
import sys

import numpy as np
import torch

from . import ops
from .cocoeval import STAT_NAMES
from .evalcore import DetectionStore, load_dataset, rank_in_run, score_then_key_order


def mcnemar(yes_no, no_yes):
    """McNemar's test as both notebooks call it (statsmodels mcnemar(table, exact=False, correction=True)) -> (statistic, pvalue):
    statistic = (|b - c| - 1)^2 / (b + c), pvalue = the chi-square survival function at one degree of freedom = erfc(sqrt(statistic / 2)).
    b + c == 0 (no discordant instance: nothing to test) returns (0.0, 1.0); the bare formula divides by zero there."""
    b, c = int(yes_no), int(no_yes)
    if b < 0 or c < 0:
        raise ValueError("mcnemar: counts must not be negative")
    if b + c == 0:
        return 0.0, 1.0
    statistic = (abs(b - c) - 1) ** 2 / (b + c)
    return statistic, math.erfc(math.sqrt(statistic / 2))


class Disagreement:
    """get_disagreement.py on the device.  `gt`: see evalcore.load_dataset.  `max_dets`: keep each model's `max_dets` best-scored detections
    of an image, in descending score order (300 is what LVISResults applies); None keeps all, in input order."""

    def __init__(self, gt, device=None, max_dets=None):
        self.dataset = load_dataset(gt)
        self.device = dev = torch.device("cuda:0" if device is None else device)
        if max_dets is not None and int(max_dets) < 1:
            raise ValueError("Disagreement: max_dets must be at least 1 (or None)")
        self.max_dets = None if max_dets is None else int(max_dets)
        self.img_ids = sorted(set(im["id"] for im in self.dataset["images"]))
        self._img_index = {v: i for i, v in enumerate(self.img_ids)}
        anns = [(j, a) for j, a in enumerate(self.dataset.get("annotations", [])) if a["image_id"] in self._img_index]
        img = np.asarray([self._img_index[a["image_id"]] for _j, a in anns], np.int64)
        order = np.argsort(img, kind="mergesort")                                # image-major, dataset order within an image
        self.gt_index = np.asarray([anns[o][0] for o in order], np.int64)       # slot -> position in dataset["annotations"]
        count = np.bincount(img, minlength=len(self.img_ids)).astype(np.int64)
        self.gt_count = torch.from_numpy(count).to(dev)
        self.gt_offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(count)]).astype(np.int64)).to(dev)
        self.gt_box = torch.from_numpy(np.asarray([anns[o][1]["bbox"] for o in order], np.float64).reshape(-1, 4)).to(dev)
        self.gt_label = torch.from_numpy(np.asarray([anns[o][1]["category_id"] for o in order], np.int64)).to(dev)
        self.num_gt = int(self.gt_index.shape[0])
        self.reset()

    def reset(self):
        """Forget the detections of both models (the ground truth stays)."""
        self._det = [DetectionStore(self.device, self.img_ids, self._img_index) for _ in range(2)]
        self.result = None
        self.best_iou = self.best_index = self.correct = self.dt_offsets = None

    num_added = property(lambda self: [side.num_added for side in self._det])

    # ---- detections
    def _side(self, model):
        if isinstance(model, bool) or model not in (0, 1):
            raise ValueError(f"Disagreement: model must be 0 or 1, not {model!r}")
        return self._det[model]

    def add(self, model, image_id, category_ids, scores, boxes):
        """The detections of `model` (0 or 1) on one image (or, with image_id a tensor [n], on many): category_ids [n], scores [n], boxes [n, 4]
        as [x, y, w, h].  Tensors stay on the device; float32 is widened exactly."""
        self._side(model).add("Disagreement.add", image_id, category_ids, scores, boxes)

    def add_results(self, model, results):
        """COCO result dicts (`image_id`, `category_id`, `score`, `bbox`) of `model` (0 or 1), e.g. a loaded results json."""
        self._side(model).add_results(results)

    def _kept(self, side, confidence):
        """One model's detections (its DetectionStore) as the kernel takes them: (offsets [I + 1], boxes, labels, per-image counts),
        image-major; within an image in input order, or with max_dets in descending score order (stable) cut to max_dets."""
        dev, I = self.device, len(self.img_ids)
        img, cat, score, box = side.tensors()
        src = torch.nonzero((img >= 0) & (score > confidence)).reshape(-1)      # strict; a detection on an unknown image is dropped
        key = img[src]
        if self.max_dets is None:
            perm = torch.sort(key, stable=True).indices
            key = key[perm]
        else:
            perm = score_then_key_order(score[src], key)
            key = key[perm]
            top = rank_in_run(key) < self.max_dets
            perm, key = perm[top], key[top]
        index = src[perm]
        count = torch.bincount(key, minlength=I) if I else torch.zeros(0, dtype=torch.int64, device=dev)
        offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(count, 0)])
        return offsets.contiguous(), box[index].contiguous(), cat[index].contiguous(), count, index

    def _tally(self, count_a, count_b):
        """[yes_yes, yes_no, no_yes, total, missed] on the device from `correct` and the two models' per-image detection counts."""
        counted = (self.gt_count > 0) & (count_a > 0) & (count_b > 0)                        # per image
        on = torch.repeat_interleave(counted, self.gt_count, output_size=self.num_gt)        # per ground truth
        c0, c1 = self.correct[0].bool() & on, self.correct[1].bool() & on
        return torch.stack([(c0 & c1).sum(), (c0 & ~c1).sum(), (~c0 & c1).sum(), on.sum(), len(self.img_ids) - counted.sum()])

    def run(self, iou_threshold=0.5, confidence=0.0):
        """-> {"yes_yes", "yes_no", "no_yes", "no_no", "total", "missed"} (ints) and "correct" (uint8 [2, G] on the device, slot order: gt_index).
        yes_no: right for model 0 only; no_yes: right for model 1 only.  May be called again with other thresholds without re-adding.
        Leaves best_iou / best_index / correct [2, G], dt_offsets and dt_index (per model: slot -> position in the order added) behind; the
        rows of `correct` of an image that is not counted are still each model's own answer."""
        a, b = self._kept(self._det[0], confidence), self._kept(self._det[1], confidence)
        self.dt_offsets, self.dt_index = (a[0], b[0]), (a[4], b[4])
        self.best_iou, self.best_index, self.correct = ops.box_disagreement(self.gt_offsets, self.gt_box, self.gt_label, a[:3], b[:3],
                                                                            iou_threshold)
        yes_yes, yes_no, no_yes, total, missed = (int(v) for v in self._tally(a[3], b[3]).cpu().tolist())        # the one host read
        self.result = {"yes_yes": yes_yes, "yes_no": yes_no, "no_yes": no_yes, "no_no": total - yes_yes - yes_no - no_yes, "total": total,
                       "missed": missed, "correct": self.correct, "iou_threshold": float(iou_threshold), "confidence": float(confidence)}
        return self.result

    def report(self, alpha=0.05, file=None):
        """Prints the contingency table of the last run(), McNemar's test and the verdict line, as the notebook does; -> (statistic, pvalue)."""
        if self.result is None:
            raise RuntimeError("Disagreement.report: call run() first")
        r, out = self.result, (sys.stdout if file is None else file)
        rows = [[f"IoU@{r['iou_threshold']}", "Correct2", "Incorrect2"], ["Correct1", str(r["yes_yes"]), str(r["yes_no"])],
                ["Incorrect1", str(r["no_yes"]), str(r["no_no"])]]
        width = [max(len(row[c]) for row in rows) + 2 for c in range(3)]
        rule = "+" + "+".join("-" * w for w in width) + "+"
        print(rule, file=out)
        for n, row in enumerate(rows):
            print("|" + "|".join(cell.center(w) for cell, w in zip(row, width)) + "|", file=out)
            if n == 0 or n == len(rows) - 1:
                print(rule, file=out)
        statistic, pvalue = mcnemar(r["yes_no"], r["no_yes"])
        print("McNemar's test:", file=out)
        print("statistic=%.4f, p-value=%.4f" % (statistic, pvalue), file=out)
        print("Same proportions of errors (fail to reject H0)" if pvalue > alpha else "Different proportions of errors (reject H0)", file=out)
        return statistic, pvalue


# ---- bootstrap over images: is a difference in AP more than noise?  (host code; the replicates are COCOEval.bootstrap / LVISEval.bootstrap)
def bootstrap_weights(num_images, replicates, seed):
    """`replicates` resamples of `num_images` images with replacement as counts: int32 [replicates, num_images], every row sums to
    num_images.  The same seed gives the same array; two evaluators compared with paired_bootstrap must be given the same one."""
    n, b = int(num_images), int(replicates)
    if n < 1 or b < 0:
        raise ValueError("bootstrap_weights: at least one image, and no negative number of replicates")
    return np.random.default_rng(seed).multinomial(n, [1 / n] * n, size=b).astype(np.int32)


def interval(values, level=0.95):
    """The percentile interval of one statistic over its replicates (a replicate of value -1 has no valid cell and is dropped) ->
    {"mean", "lo", "hi", "n_used"}: np.quantile at (1 - level) / 2 and 1 - (1 - level) / 2; NaN when no replicate is left."""
    if not 0 < level < 1:
        raise ValueError("interval: level must lie in (0, 1)")
    v = np.asarray(values, np.float64).reshape(-1)
    v = v[v != -1]
    if v.size == 0:
        return {"mean": float("nan"), "lo": float("nan"), "hi": float("nan"), "n_used": 0}
    lo, hi = np.quantile(v, [(1 - level) / 2, 1 - (1 - level) / 2])
    return {"mean": float(v.mean()), "lo": float(lo), "hi": float(hi), "n_used": int(v.size)}


def paired_bootstrap(a, b, level=0.95):
    """Two bootstrap() results [B, n] of two evaluators run with the SAME weights -> per column {"delta_mean", "lo", "hi", "n_used", "p"} as
    arrays [n] (a [B] input is one column).  Pairs where either value is -1 are dropped; d = b - a; lo / hi as in interval();
    p = min(1, 2 * min((#(d <= 0) + 1) / (n + 1), (#(d >= 0) + 1) / (n + 1))), the two-sided percentile test with the add-one correction.
    No pair left: NaN for the mean and the bounds, p = 1."""
    if not 0 < level < 1:
        raise ValueError("paired_bootstrap: level must lie in (0, 1)")
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.shape != b.shape or a.ndim not in (1, 2):
        raise ValueError("paired_bootstrap: two arrays of the same shape [replicates] or [replicates, statistics]")
    a, b = a.reshape(a.shape[0], -1), b.reshape(b.shape[0], -1)
    cols = a.shape[1]
    out = {"delta_mean": np.full(cols, np.nan), "lo": np.full(cols, np.nan), "hi": np.full(cols, np.nan), "n_used": np.zeros(cols, np.int64),
           "p": np.ones(cols, np.float64)}
    for c in range(cols):
        keep = (a[:, c] != -1) & (b[:, c] != -1)
        d = b[keep, c] - a[keep, c]
        n = int(d.size)
        if n == 0:
            continue
        out["delta_mean"][c], out["n_used"][c] = d.mean(), n
        out["lo"][c], out["hi"][c] = np.quantile(d, [(1 - level) / 2, 1 - (1 - level) / 2])
        out["p"][c] = min(1.0, 2 * min((int((d <= 0).sum()) + 1) / (n + 1), (int((d >= 0).sum()) + 1) / (n + 1)))
    return out


def per_category_table(evaluators, metric_columns=(0,)):
    """get_map.py's `results` dict for accumulated COCOEval objects {experiment name: COCOEval}: "columns" = the names of the chosen
    statistics (indices into AP, AP50, AP75, APs, APm, APl, AR1, AR10, AR100, ARs, ARm, ARl) and, per experiment, {name of the statistic:
    its value for every category, in the order of cat_ids}.  The chosen columns are returned; get_map.py:59-60 reads stats[position in the
    list] instead, which is statistic 0 whatever was asked for."""
    cols = [int(c) for c in metric_columns]
    if any(c < 0 or c >= len(STAT_NAMES) for c in cols):
        raise ValueError(f"per_category_table: metric_columns must index the {len(STAT_NAMES)} COCO statistics")
    table = {"columns": [STAT_NAMES[c] for c in cols]}
    for name, ev in evaluators.items():
        if name == "columns":
            raise ValueError("per_category_table: an experiment cannot be named 'columns'")
        if getattr(ev, "iou_type", None) == "keypoints":          # ten statistics under other names (COCOEval.stat_names)
            raise NotImplementedError("per_category_table: the columns are the twelve bbox / segm statistics; for a keypoints evaluator "
                                      "read summarize_per_category() with its stat_names")
        stats = ev.summarize_per_category()
        table[name] = {STAT_NAMES[c]: [float(v) for v in stats[:, c]] for c in cols}
    return table
