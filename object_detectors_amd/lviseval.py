"""LVIS evaluation on the device: what lvis-api's `LVISEval(gt, results, 'bbox').run()` computes (v0.5.3, lvis/eval.py and lvis/results.py),
without the `lvis` package.  The slot layout, the IoU pass and the accumulate pass are those of cocoeval.py; LVIS adds a front end and a match
rule (csrc/cocoeval_kernels.hip, `mi355det_lvis_match`: the COCO walk with a compile-time switch):

    add(...)        detections stay device tensors (boxes, scores, labels)
    evaluate()      torch sorts (plumbing): the CUT - per image, over all categories, the 300 best by score (stable) - and only then the
                    FEDERATED FILTER: a detection of category c in image i stays if c is a negative category of i or i has an annotation of c;
                    every other one (unknown categories too) is dropped, neither false positive nor ignored.  Then coco_iou (no crowds: always
                    the plain union) and lvis_match: no re-match of a taken ground truth, the annotation's `ignore` flag where COCO has
                    iscrowd, and an unmatched detection is ignored where its category is in the image's not_exhaustive_category_ids.
    accumulate()    coco_accumulate with one maxDets that cuts nothing -> precision [10, 101, K, 4], recall [10, K, 4] on the host
    summarize()     numpy: AP, AP50, AP75, APs, APm, APl, APr, APc, APf (categories by `frequency`), AR@300, ARs@300, ARm@300, ARl@300
    bootstrap(w)    after evaluate(): the thirteen numbers of resampled data sets (cocoeval.py, csrc/bootstrap_kernels.hip)

Slot layout after evaluate(): as in cocoeval.py (category-major, image second; `group_keys`, the three offset arrays, `dt_index`, `gt_index`,
`iou`, `dt_match`, `dt_ignore`, `gt_match`, `gt_ignore`), with no per-group cut, plus `group_not_exhaustive` [groups] uint8.

`bbox` only: LVIS segmentations are polygons, and the polygon-to-mask conversion is out of scope here as it is in COCOEval."""
import json
import sys
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .cocoeval import AREA_RNG, IOU_THRS, REC_THRS, category_order, cell_mean, group_offsets, load_dataset, run_bootstrap, sort_ground_truth

MAX_DETS = 300
RESULT_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")
NO_CUT = 2 ** 31 - 1                      # the single "maxDets" of the accumulate pass: every rank passes


def _member(table, keys):
    """keys in the sorted table, elementwise (both int64 on the device)."""
    if int(table.shape[0]) == 0:
        return torch.zeros_like(keys, dtype=torch.bool)
    return table[torch.searchsorted(table, keys).clamp_(max=int(table.shape[0]) - 1)] == keys


class LVISEval:
    """LVISEval for `bbox` on the device.  `lvis_gt`: a path to an LVIS json, a dataset dict or an object with `.dataset`; `lvis_dt`: None, a
    path to a results json or a list of result dicts (more come in through add() / add_results()).  run() = evaluate(), accumulate(),
    summarize(); get_results() / print_results() as in lvis-api."""

    def __init__(self, lvis_gt, lvis_dt=None, iou_type="bbox", device=None):
        if iou_type != "bbox":
            raise NotImplementedError(f"LVISEval: iou_type {iou_type!r}: only bbox is evaluated here (LVIS segmentations are polygons, and the "
                                      "polygon-to-mask conversion is out of scope: DESIGN.md)")
        self.iou_type = iou_type
        self.dataset = load_dataset(lvis_gt)
        self.device = torch.device("cuda:0" if device is None else device)
        for im in self.dataset["images"]:
            for field in ("neg_category_ids", "not_exhaustive_category_ids"):
                if field not in im:
                    raise ValueError(f"LVISEval: image {im.get('id')} of the ground truth has no {field}")
        for c in self.dataset["categories"]:
            if c.get("frequency") not in ("r", "c", "f"):
                raise ValueError(f"LVISEval: category {c.get('id')} of the ground truth has no frequency in r / c / f")
        self.img_ids = sorted(set(im["id"] for im in self.dataset["images"]))
        self.cat_ids = sorted(c["id"] for c in self.dataset["categories"])
        self._img_index = {v: i for i, v in enumerate(self.img_ids)}
        self._cat_index = {v: i for i, v in enumerate(self.cat_ids)}
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rng = IOU_THRS, REC_THRS, MAX_DETS, np.asarray(AREA_RNG, np.float64)
        freq = {c["id"]: c["frequency"] for c in self.dataset["categories"]}
        self.freq_groups = [[k for k, c in enumerate(self.cat_ids) if freq[c] == f] for f in ("r", "c", "f")]
        self._anns = [(j, a) for j, a in enumerate(self.dataset.get("annotations", []))
                      if a["image_id"] in self._img_index and a["category_id"] in self._cat_index]
        self._gt = None
        self.reset()
        if lvis_dt is not None:
            if isinstance(lvis_dt, (str, bytes)) or hasattr(lvis_dt, "__fspath__"):
                with open(lvis_dt) as f:
                    lvis_dt = json.load(f)
            if not isinstance(lvis_dt, (list, tuple)):
                raise ValueError("LVISEval: the detections must be a results json path or a list of result dicts")
            self.add_results(lvis_dt)

    def reset(self):
        """Forget the detections (the ground truth stays)."""
        self._img, self._cat, self._score, self._box = [], [], [], []
        self.num_added = 0
        self.precision = self.recall = None
        self.results = OrderedDict()
        self.iou = None

    # ---- detections
    def add(self, image_id, category_ids, scores, boxes):
        """The detections of one image (or, with image_id a tensor [n], of many): category_ids [n], scores [n], boxes [n, 4] as [x, y, w, h].
        Tensors stay on the device; float32 is widened exactly."""
        dev = self.device
        cat = torch.as_tensor(category_ids, device=dev).to(torch.int64).reshape(-1)
        n = int(cat.shape[0])
        score = torch.as_tensor(scores, device=dev).to(torch.float64).reshape(-1)
        box = torch.as_tensor(boxes, device=dev).to(torch.float64).reshape(-1, 4)
        if score.shape[0] != n or box.shape[0] != n:
            raise ValueError("LVISEval.add: one score and one box per detection")
        if torch.is_tensor(image_id) and image_id.dim() > 0:
            ids = image_id.to(dev).to(torch.int64).reshape(-1)
            if ids.shape[0] != n:
                raise ValueError("LVISEval.add: one image id per detection, or one for all")
            table = torch.tensor(self.img_ids, dtype=torch.int64, device=dev)
            self._img.append(torch.where(_member(table, ids), torch.searchsorted(table, ids), torch.full_like(ids, -1)))
        else:
            i = self._img_index.get(image_id.item() if torch.is_tensor(image_id) else image_id, -1)
            self._img.append(torch.full((n,), i, dtype=torch.int64, device=dev))
        self._cat.append(cat)
        self._score.append(score)
        self._box.append(box)
        self.num_added += n

    def add_results(self, results):
        """LVIS result dicts (`image_id`, `category_id`, `score`, `bbox`), e.g. the rows of to_coco_results(..., "lvis")."""
        if not results:
            return
        dev = self.device
        self._box.append(torch.tensor([r["bbox"] for r in results], dtype=torch.float64, device=dev).reshape(-1, 4))
        self._img.append(torch.tensor([self._img_index.get(r["image_id"], -1) for r in results], dtype=torch.int64, device=dev))
        self._cat.append(torch.tensor([r["category_id"] for r in results], dtype=torch.int64, device=dev))
        self._score.append(torch.tensor([r["score"] for r in results], dtype=torch.float64, device=dev))
        self.num_added += len(results)

    # ---- ground truth, sorted category-major once, and the key tables of the federated rules (key = category index * images + image index)
    def _ground_truth(self):
        if self._gt is not None:
            return self._gt
        dev, I = self.device, len(self.img_ids)
        anns = self._anns
        key, order = sort_ground_truth(anns, self._cat_index, self._img_index, I)
        gt = {"key": key, "index": np.asarray([anns[o][0] for o in order], np.int64),
              "area": np.asarray([float(anns[o][1]["area"]) for o in order], np.float64),
              "flag": np.asarray([1 if anns[o][1].get("ignore", 0) else 0 for o in order], np.uint8),
              "no_crowd": np.zeros(len(anns), np.uint8)}                      # coco_iou's crowd array: LVIS never reads iscrowd
        gt["box"] = torch.from_numpy(np.asarray([anns[o][1]["bbox"] for o in order], np.float64).reshape(-1, 4)).to(dev)

        def keys_of(field):
            return [self._cat_index[c] * I + self._img_index[im["id"]] for im in self.dataset["images"] for c in im[field] if c in self._cat_index]
        table = lambda ks: torch.from_numpy(np.unique(np.asarray(ks, np.int64))).to(dev)
        gt["filter_keys"] = table(key.tolist() + keys_of("neg_category_ids"))             # positive keys and negative keys
        gt["nel_keys"] = table(keys_of("not_exhaustive_category_ids"))
        for k in ("key", "area", "flag", "no_crowd"):
            gt[k + "_dev"] = torch.from_numpy(gt[k]).to(dev)
        self._gt = gt
        return gt

    def _group(self):
        """The front end: cut, filter, group.  Leaves the slot layout (offsets, keys, flags, the detections' boxes, areas and scores) on the
        device and returns the size of the ragged IoU buffer."""
        dev, I, K = self.device, len(self.img_ids), len(self.cat_ids)
        gt = self._ground_truth()
        i64 = lambda xs: torch.cat(xs) if xs else torch.zeros(0, dtype=torch.int64, device=dev)
        img, cat_id = i64(self._img), i64(self._cat)
        score = torch.cat(self._score) if self._score else torch.zeros(0, dtype=torch.float64, device=dev)
        # the cut: descending score (stable), then by image (stable): each image's detections of all categories in score order; rank < 300
        src = torch.nonzero(img >= 0).reshape(-1)
        o1 = torch.sort(-score[src], stable=True).indices
        o2 = torch.sort(img[src][o1], stable=True).indices
        sel = src[o1[o2]]
        im = img[sel]
        rank = torch.arange(int(im.shape[0]), device=dev) - torch.searchsorted(im, im)      # im is sorted: its first position is the image's start
        sel = sel[rank < self.max_dets]
        # the federated filter, after the cut: known category, and (category, image) among the positive or negative keys
        cats = torch.tensor(self.cat_ids, dtype=torch.int64, device=dev)
        cat = torch.searchsorted(cats, cat_id[sel]).clamp_(max=max(K - 1, 0))
        key = cat * I + img[sel]
        keep = (_member(cats, cat_id[sel]) & _member(gt["filter_keys"], key)) if K else torch.zeros_like(key, dtype=torch.bool)
        sel, key = sel[keep], key[keep]
        # group: a stable sort by key keeps each group's detections in score order
        o3 = torch.sort(key, stable=True).indices
        self.dt_index, key = sel[o3], key[o3].contiguous()
        self.dt_score = score[self.dt_index].contiguous()
        self.dt_image, self.gt_image = (key % max(I, 1)).to(torch.int32), (gt["key_dev"] % max(I, 1)).to(torch.int32)       # bootstrap() weighs by them
        num_dt = int(key.shape[0])
        self.dt_rank = torch.zeros(num_dt, dtype=torch.int32, device=dev)                   # no per-group cut: nothing ranks past NO_CUT
        keys = torch.unique(torch.cat([key, gt["key_dev"]]))
        ng = int(keys.shape[0])
        dc, self.dt_offsets = group_offsets(keys, key)
        gc, self.gt_offsets = group_offsets(keys, gt["key_dev"])
        self.iou_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(dc * gc, 0)])
        iou_size = int(self.iou_offsets[-1])                      # the one host read: it sizes the IoU buffer
        self.group_keys, self.gt_index = keys, gt["index"]
        self.group_not_exhaustive = _member(gt["nel_keys"], keys).to(torch.uint8).contiguous()
        cat_edges = torch.arange(K + 1, device=dev) * I
        self.cat_dt_offsets = torch.searchsorted(key, cat_edges).contiguous()
        self.cat_gt_offsets = torch.searchsorted(gt["key_dev"], cat_edges).contiguous()
        dt_box = (torch.cat(self._box) if self._box else torch.zeros((0, 4), dtype=torch.float64, device=dev))[self.dt_index].contiguous()
        self.dt_boxes, self.dt_area = dt_box, (dt_box[:, 2] * dt_box[:, 3]).contiguous()
        self.num_dt, self.num_gt, self.num_groups = num_dt, int(gt["key"].shape[0]), ng
        return iou_size

    def _match(self, iou_size):
        """coco_iou with an all-zero crowd array (never the ignore flags), then lvis_match."""
        dev, gt = self.device, self._ground_truth()
        self.iou = ops.coco_iou(self.dt_offsets, self.gt_offsets, self.iou_offsets, iou_size, self.dt_boxes, gt["box"], gt["no_crowd_dev"])
        thr = torch.from_numpy(np.ascontiguousarray(self.iou_thrs, np.float64)).to(dev)
        rng = torch.from_numpy(np.ascontiguousarray(self.area_rng, np.float64)).to(dev)
        self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore = ops.lvis_match(
            self.dt_offsets, self.gt_offsets, self.iou_offsets, self.iou, self.dt_area, gt["area_dev"], gt["flag_dev"], self.group_not_exhaustive,
            thr, rng)

    def evaluate(self):
        """Cut, filter, group, IoU, match.  Leaves iou / iou_offsets / dt_offsets / gt_offsets / group_keys / group_not_exhaustive and the four
        match arrays dt_match, dt_ignore [4, 10, num_dt], gt_match [4, 10, num_gt], gt_ignore [4, num_gt] on the device."""
        self._match(self._group())
        return self

    def accumulate(self):
        """precision [10, 101, K, 4], recall [10, K, 4] as float64 numpy arrays."""
        if self.iou is None:
            raise RuntimeError("LVISEval.accumulate: call evaluate() first")
        self.order = category_order(self.cat_dt_offsets, self.dt_score)
        rec = torch.from_numpy(np.ascontiguousarray(self.rec_thrs, np.float64)).to(self.device)
        p, r, _scores = ops.coco_accumulate(self.cat_dt_offsets, self.cat_gt_offsets, self.order, self.dt_rank, self.dt_score, self.dt_match,
                                            self.dt_ignore, self.gt_ignore, [NO_CUT], rec)
        self.precision, self.recall = p[..., 0].cpu().numpy(), r[..., 0].cpu().numpy()
        return self

    def bootstrap(self, weights, return_cells=False, cell_budget_bytes=1 << 30):
        """The thirteen statistics of resampled data sets, float64 numpy [B, 13] in RESULT_KEYS order (APr / APc / APf over freq_groups):
        COCOEval.bootstrap under the LVIS rules, with the single maxDets that cuts nothing.  Needs evaluate() only and leaves .precision,
        .recall and .results as they are.  return_cells=True: -> (stats, (ap_sum, recall)), float64 [B, 10, K, 4, 1] on the device."""
        R = len(self.rec_thrs)

        def rows(ap_sum, recall):
            ap = lambda cells: cell_mean(cells, R)
            pick = lambda dim, idx: ap_sum.index_select(dim, torch.tensor([int(j) for j in idx], dtype=torch.int64, device=ap_sum.device))
            at = lambda thr: pick(1, np.flatnonzero(np.isclose(self.iou_thrs, thr)))
            return ([ap(ap_sum[:, :, :, 0]), ap(at(.5)[:, :, :, 0]), ap(at(.75)[:, :, :, 0])] + [ap(ap_sum[:, :, :, a]) for a in (1, 2, 3)] +
                    [ap(pick(2, c)[:, :, :, 0]) for c in self.freq_groups] + [cell_mean(recall[:, :, :, a], 1) for a in (0, 1, 2, 3)])
        return run_bootstrap(self, weights, [NO_CUT], rows, len(RESULT_KEYS), cell_budget_bytes, return_cells, "LVISEval.bootstrap")

    def _stat(self, ap, iou_thr=None, area=0, cats=None):
        s = self.precision if ap else self.recall
        if iou_thr is not None:
            s = s[np.isclose(self.iou_thrs, iou_thr)]
        if ap:
            s = s[:, :, :, area] if cats is None else s[:, :, np.asarray(cats, np.int64), area]
        else:
            s = s[:, :, area]
        s = s[s > -1]
        return np.float64(-1) if s.size == 0 else np.mean(s)

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
