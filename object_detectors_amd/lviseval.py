"""LVIS evaluation on the device: what lvis-api's `LVISEval(gt, results, 'bbox').run()` computes (v0.5.3, lvis/eval.py and lvis/results.py),
without the `lvis` package.  The slot layout, the detection lists, the IoU pass and the accumulate and bootstrap passes are evalcore.py
(GroupedEval), shared with cocoeval.py; LVIS adds a front end and a match rule (csrc/cocoeval_kernels.hip, `mi355det_lvis_match`: the COCO
walk with a compile-time switch):

    add(...)        detections stay device tensors (boxes, scores, labels)
    evaluate()      torch sorts (plumbing): the CUT - per image, over all categories, the 300 best by score (stable) - and only then the
                    FEDERATED FILTER: a detection of category c in image i stays if c is a negative category of i or i has an annotation of c;
                    every other one (unknown categories too) is dropped, neither false positive nor ignored.  Then coco_iou (no crowds: always
                    the plain union) and lvis_match: no re-match of a taken ground truth, the annotation's `ignore` flag where COCO has
                    iscrowd, and an unmatched detection is ignored where its category is in the image's not_exhaustive_category_ids.
    accumulate()    coco_accumulate with one maxDets that cuts nothing -> precision [10, 101, K, 4], recall [10, K, 4] on the host
    summarize()     numpy: AP, AP50, AP75, APs, APm, APl, APr, APc, APf (categories by `frequency`), AR@300, ARs@300, ARm@300, ARl@300
    bootstrap(w)    after evaluate(): the thirteen numbers of resampled data sets, in RESULT_KEYS order (csrc/bootstrap_kernels.hip)

After evaluate() there is no per-group cut (`dt_rank` is zero), and `group_not_exhaustive` [groups] uint8 joins the slot layout.

`bbox` only: LVIS segmentations are polygons; polygons.dataset_to_rle converts them, and wiring that in is a later change."""
import json
import sys
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .evalcore import NO_CUT, GroupedEval, cell_mean, lookup, masked_mean, member, rank_in_run, score_then_key_order

MAX_DETS = 300
RESULT_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")


class LVISEval(GroupedEval):
    """LVISEval for `bbox` on the device.  `lvis_gt`: a path to an LVIS json, a dataset dict or an object with `.dataset`; `lvis_dt`: None, a
    path to a results json or a list of result dicts (more come in through add() / add_results()).  run() = evaluate(), accumulate(),
    summarize(); get_results() / print_results() as in lvis-api."""
    kind, flag_field, stat_names, cuts = "lvis", "ignore", RESULT_KEYS, [NO_CUT]

    def __init__(self, lvis_gt, lvis_dt=None, iou_type="bbox", device=None):
        if iou_type != "bbox":
            raise NotImplementedError(f"LVISEval: iou_type {iou_type!r}: only bbox is evaluated here (LVIS segmentations are polygons, and the "
                                      "polygon-to-mask conversion is out of scope: DESIGN.md)")
        super().__init__(lvis_gt, iou_type, device, MAX_DETS)
        for im in self.dataset["images"]:
            for field in ("neg_category_ids", "not_exhaustive_category_ids"):
                if field not in im:
                    raise ValueError(f"LVISEval: image {im.get('id')} of the ground truth has no {field}")
        for c in self.dataset["categories"]:
            if c.get("frequency") not in ("r", "c", "f"):
                raise ValueError(f"LVISEval: category {c.get('id')} of the ground truth has no frequency in r / c / f")
        freq = {c["id"]: c["frequency"] for c in self.dataset["categories"]}
        self.freq_groups = [[k for k, c in enumerate(self.cat_ids) if freq[c] == f] for f in ("r", "c", "f")]
        if lvis_dt is not None:
            if isinstance(lvis_dt, (str, bytes)) or hasattr(lvis_dt, "__fspath__"):
                with open(lvis_dt) as f:
                    lvis_dt = json.load(f)
            if not isinstance(lvis_dt, (list, tuple)):
                raise ValueError("LVISEval: the detections must be a results json path or a list of result dicts")
            self.add_results(lvis_dt)

    def reset(self):
        super().reset()
        self.results = OrderedDict()

    def _build_ground_truth(self):
        """Adds the key tables of the federated rules (key = category index * images + image index)."""
        gt, I = super()._build_ground_truth(), len(self.img_ids)

        def keys_of(field):
            return [self._cat_index[c] * I + self._img_index[im["id"]] for im in self.dataset["images"] for c in im[field] if c in self._cat_index]
        table = lambda ks: torch.from_numpy(np.unique(np.asarray(ks, np.int64))).to(self.device)
        gt["filter_keys"] = table(gt["key"].tolist() + keys_of("neg_category_ids"))       # positive keys and negative keys
        gt["nel_keys"] = table(keys_of("not_exhaustive_category_ids"))
        return gt

    def _group(self):
        """The front end: cut, filter, group."""
        I, gt = len(self.img_ids), self._ground_truth()
        img, cat_id, score, box = self._dets.tensors()
        # the cut: descending score (stable), then by image (stable): each image's detections of all categories in score order; rank < 300
        src = torch.nonzero(img >= 0).reshape(-1)
        sel = src[score_then_key_order(score[src], img[src])]
        sel = sel[rank_in_run(img[sel]) < self.max_dets]
        # the federated filter, after the cut: known category, and (category, image) among the positive or negative keys
        cat, known = lookup(torch.tensor(self.cat_ids, dtype=torch.int64, device=self.device), cat_id[sel])
        key = cat * I + img[sel]
        keep = known & member(gt["filter_keys"], key)
        sel, key = sel[keep], key[keep]
        # group: a stable sort by key keeps each group's detections in score order
        o = torch.sort(key, stable=True).indices
        iou_size = self._layout(key[o].contiguous(), sel[o], score, box)
        self.group_not_exhaustive = member(gt["nel_keys"], self.group_keys).to(torch.uint8).contiguous()
        return iou_size

    def _match(self, iou_size):
        """coco_iou with an all-zero crowd array (never the ignore flags), then lvis_match."""
        thr, rng, _rec = self._params()
        self.iou = ops.coco_iou(self.dt_offsets, self.gt_offsets, self.iou_offsets, iou_size, self.dt_boxes, self.gt_boxes, self.gt_crowd)
        self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore = ops.lvis_match(
            self.dt_offsets, self.gt_offsets, self.iou_offsets, self.iou, self.dt_area, self.gt_area, self.gt_flag, self.group_not_exhaustive,
            thr, rng)

    def accumulate(self):
        """precision [10, 101, K, 4], recall [10, K, 4] as float64 numpy arrays."""
        p, r, _scores = self._accumulate()
        self.precision, self.recall = p[..., 0].cpu().numpy(), r[..., 0].cpu().numpy()
        return self

    def _stat_rows(self, ap_sum, recall):
        """bootstrap(): the thirteen statistics in RESULT_KEYS order (APr / APc / APf over freq_groups)."""
        ap = lambda cells: cell_mean(cells, len(self.rec_thrs))
        pick = lambda dim, idx: ap_sum.index_select(dim, torch.tensor([int(j) for j in idx], dtype=torch.int64, device=ap_sum.device))
        at = lambda thr: pick(1, np.flatnonzero(np.isclose(self.iou_thrs, thr)))
        return ([ap(ap_sum[:, :, :, 0]), ap(at(.5)[:, :, :, 0]), ap(at(.75)[:, :, :, 0])] + [ap(ap_sum[:, :, :, a]) for a in (1, 2, 3)] +
                [ap(pick(2, c)[:, :, :, 0]) for c in self.freq_groups] + [cell_mean(recall[:, :, :, a], 1) for a in (0, 1, 2, 3)])

    def _stat(self, ap, iou_thr=None, area=0, cats=None):
        s = self.precision if ap else self.recall
        if iou_thr is not None:
            s = s[np.isclose(self.iou_thrs, iou_thr)]
        if ap:
            return masked_mean(s[:, :, :, area] if cats is None else s[:, :, np.asarray(cats, np.int64), area])
        return masked_mean(s[:, :, area])

    def summarize(self):
        """Sets and returns .results: the thirteen LVIS statistics, an ordered dict."""
        if self.precision is None:
            raise RuntimeError("LVISEval.summarize: call accumulate() first")
        res = OrderedDict()
        res["AP"], res["AP50"], res["AP75"] = self._stat(1), self._stat(1, .5), self._stat(1, .75)
        res["APs"], res["APm"], res["APl"] = (self._stat(1, area=a) for a in (1, 2, 3))
        res["APr"], res["APc"], res["APf"] = (self._stat(1, cats=c) for c in self.freq_groups)
        res["AR@300"] = self._stat(0)
        res["ARs@300"], res["ARm@300"], res["ARl@300"] = (self._stat(0, area=a) for a in (1, 2, 3))
        assert tuple(res) == RESULT_KEYS
        self.results = res
        return res

    def run(self):
        self.evaluate()
        self.accumulate()
        self.summarize()
        return self

    def get_results(self):
        if not self.results:
            raise RuntimeError("LVISEval.get_results: call run() first")
        return self.results

    def print_results(self, file=None):
        """One line per statistic, in lvis-api's format."""
        template = " {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} catIds={:>3s}] = {:0.3f}"
        span = f"{self.iou_thrs[0]:0.2f}:{self.iou_thrs[-1]:0.2f}"
        rows = {"AP50": ("0.50", "all", "all"), "AP75": ("0.75", "all", "all"), "APs": (span, "s", "all"), "APm": (span, "m", "all"),
                "APl": (span, "l", "all"), "APr": (span, "all", "r"), "APc": (span, "all", "c"), "APf": (span, "all", "f"),
                "ARs@300": (span, "s", "all"), "ARm@300": (span, "m", "all"), "ARl@300": (span, "l", "all")}
        for key, value in self.get_results().items():
            title, kind = ("Average Precision", "(AP)") if key.startswith("AP") else ("Average Recall", "(AR)")
            iou, area, cats = rows.get(key, (span, "all", "all"))
            print(template.format(title, kind, iou, area, self.max_dets, cats, value), file=sys.stdout if file is None else file)
