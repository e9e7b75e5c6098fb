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

The 2021 protocol (Dave et al., "Evaluating Large-Vocabulary Object Detectors: The Devil is in the Details"; restated from memory of the paper
and of its fork of lvis-api, which is not installed): `max_dets=None` (or -1) drops the per-image cut, `max_dets_per_cat=K` keeps each
category id's K best detections of the whole data set and is applied first; `LVISEval.fixed(gt, dt)` is AP-fixed, `max_dets=None,
max_dets_per_cat=10000`.  The keys and printed rows then read `AR@-1` (lvis-api's f-string) and `stat_names` belongs to the instance.
AP-pool - one precision-recall curve over all categories' detections, and one each over the rare, common and frequent ones - is
`accumulate_pooled()` / `summarize_pooled()` / `print_pooled()` of evalcore.GroupedEval (csrc/pooled_kernels.hip), after evaluate().

LVISEval is `bbox`; `segm` (lvis-api's `LVISEval(gt, results, 'segm')`) is LVISSegmEval below: the same cut, filter, match, accumulate and
statistics over masks.  What differs, as in lvis-api: a result's area is its mask's set pixels and its box the mask's tight box
(LVISResults), the IoU is maskUtils.iou of the run lengths with an all-zero iscrowd, and the ground truth's polygons become run lengths
once (polygons.segmentations_to_rle = frPyObjects + merge); its area stays the annotation's `area` field."""
import json
import sys
from collections import OrderedDict

import numpy as np
import torch

from . import ops
from .cocoeval import _MaskStore
from .evalcore import (MASK_TYPES, NO_CUT, GroupedEval, cell_mean, image_indices, lookup, masked_mean, member, rank_in_run, score_then_key_order)
from .polygons import is_polygon_segmentation, segmentations_to_rle
from .rle import RLEBatch, boundary_dilation

MAX_DETS = 300
FIXED_DETS_PER_CAT = 10000                # AP-fixed (Dave et al. 2021): each category's best detections over the whole data set
RESULT_KEYS = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")


class LVISEval(GroupedEval):
    """LVISEval for `bbox` on the device.  `lvis_gt`: a path to an LVIS json, a dataset dict or an object with `.dataset`; `lvis_dt`: None, a
    path to a results json or a list of result dicts (more come in through add() / add_results()).  run() = evaluate(), accumulate(),
    summarize(); get_results() / print_results() as in lvis-api."""
    kind, flag_field, stat_names, cuts = "lvis", "ignore", RESULT_KEYS, [NO_CUT]

    def __init__(self, lvis_gt, lvis_dt=None, iou_type="bbox", device=None, max_dets=MAX_DETS, max_dets_per_cat=None):
        if iou_type != "bbox":
            raise NotImplementedError(f"LVISEval: iou_type {iou_type!r}: only bbox is evaluated here (for segm and boundary: LVISSegmEval(lvis_gt, lvis_dt, iou_type=...))")
        self._set_cuts(max_dets, max_dets_per_cat)
        self._setup(lvis_gt, lvis_dt, iou_type, device)

    @classmethod
    def fixed(cls, lvis_gt, lvis_dt=None, **kw):
        """The evaluator under the 2021 protocol (AP-fixed): no per-image cut, every category's 10 000 best detections of the data set."""
        return cls(lvis_gt, lvis_dt, max_dets=None, max_dets_per_cat=FIXED_DETS_PER_CAT, **kw)

    def _set_cuts(self, max_dets, max_dets_per_cat):
        """max_dets: the per-image cut, None or -1 for none (kept as -1, the number lvis-api's keys print); max_dets_per_cat: None or the
        per-category cut over the whole data set, applied first."""
        is_int = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))
        max_dets = -1 if max_dets is None else max_dets
        if not is_int(max_dets) or max_dets == 0 or max_dets < -1:
            raise ValueError(f"{type(self).__name__}: max_dets must be a positive integer, or None / -1 for no per-image cut, not {max_dets!r}")
        if max_dets_per_cat is not None and (not is_int(max_dets_per_cat) or max_dets_per_cat <= 0):
            raise ValueError(f"{type(self).__name__}: max_dets_per_cat must be None or a positive integer, not {max_dets_per_cat!r}")
        self.max_dets = int(max_dets)
        self.max_dets_per_cat = None if max_dets_per_cat is None else int(max_dets_per_cat)
        self.stat_names = tuple(k.replace("@300", f"@{self.max_dets}") for k in RESULT_KEYS)

    def _setup(self, lvis_gt, lvis_dt, iou_type, device):
        GroupedEval.__init__(self, lvis_gt, iou_type, device, self.max_dets)
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
            self._add_given(lvis_dt)

    def _add_given(self, lvis_dt):
        """The constructor's detections: a results json path or a list of result dicts."""
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
        masks = self._mask_tensors()                               # None for bbox; for segm a detection's box and area are its mask's
        area = None
        if masks is not None:
            box, area = masks[3], masks[2]
        # the cut: descending score (stable), then by image (stable): each image's detections of all categories in score order; rank < max_dets
        src = torch.nonzero(img >= 0).reshape(-1)
        if self.max_dets_per_cat is not None:
            # the category cut comes first: per category id (known or not) the best of the whole data set, back in the order added
            o = src[score_then_key_order(score[src], cat_id[src])]
            src = torch.sort(o[rank_in_run(cat_id[o]) < self.max_dets_per_cat]).values
        sel = src[score_then_key_order(score[src], img[src])]
        if self.max_dets >= 0:
            sel = sel[rank_in_run(img[sel]) < self.max_dets]
        # the federated filter, after the cut: known category, and (category, image) among the positive or negative keys
        cat, known = lookup(torch.tensor(self.cat_ids, dtype=torch.int64, device=self.device), cat_id[sel])
        key = cat * I + img[sel]
        keep = known & member(gt["filter_keys"], key)
        sel, key = sel[keep], key[keep]
        # group: a stable sort by key keeps each group's detections in score order
        o = torch.sort(key, stable=True).indices
        iou_size = self._layout(key[o].contiguous(), sel[o], score, box, area)
        self.group_not_exhaustive = member(gt["nel_keys"], self.group_keys).to(torch.uint8).contiguous()
        if masks is None:
            self._rle = None
        else:
            self._set_rle(masks, gt, src, img)
        return iou_size

    def _mask_tensors(self):
        """The detections' masks as _MaskStore.tensors() gives them; None where the evaluator works on boxes."""
        return None

    def _match(self, iou_size):
        """coco_iou with an all-zero crowd array (never the ignore flags), then lvis_match."""
        thr, rng, _rec = self._params()
        self.iou = self._iou(iou_size)
        self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore = ops.lvis_match(
            self.dt_offsets, self.gt_offsets, self.iou_offsets, self.iou, self.dt_area, self.gt_area, self.gt_flag, self.group_not_exhaustive,
            thr, rng)

    def default_pools(self):
        """AP-pool: all categories, then the rare, the common and the frequent ones."""
        return super().default_pools() + list(zip(("r", "c", "f"), self.freq_groups))

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
        for key, a in zip(self.stat_names[9:], (0, 1, 2, 3)):
            res[key] = self._stat(0, area=a)
        assert tuple(res) == self.stat_names
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
                self.stat_names[10]: (span, "s", "all"), self.stat_names[11]: (span, "m", "all"), self.stat_names[12]: (span, "l", "all")}
        for key, value in self.get_results().items():
            title, kind = ("Average Precision", "(AP)") if key.startswith("AP") else ("Average Recall", "(AR)")
            iou, area, cats = rows.get(key, (span, "all", "all"))
            print(template.format(title, kind, iou, area, self.max_dets, cats, value), file=sys.stdout if file is None else file)


class LVISSegmEval(LVISEval):
    """LVISEval for `segm` on the device: lvis-api's `LVISEval(lvis_gt, lvis_dt, 'segm')`.  The ground truth's `segmentation`s are polygons
    (LVIS's own form; converted once by polygons.segmentations_to_rle) or run lengths, and every image needs `height` and `width`.
    Detections are masks: add(image_id, category_ids, scores, masks=RLEBatch or dense probabilities) or result dicts with `segmentation`
    ({"size", "counts"}; on a GPU the counts strings of a whole list are decoded by csrc/rle_string_kernels.hip).  A detection's area is
    its mask's set pixels and its box the mask's tight box, whatever `bbox` a result dict carries; a mask must have its image's size.
    iou_type="boundary" is lvis-api's `LVISEval(lvis_gt, lvis_dt, 'boundary')`, Boundary AP: the same inputs and rules, matched on
    min(mask IoU, boundary IoU) with the boundaries eroded by rle.boundary_dilation(h, w, dilation_ratio)."""

    def __init__(self, lvis_gt, lvis_dt=None, device=None, iou_type="segm", dilation_ratio=0.02, max_dets=MAX_DETS, max_dets_per_cat=None):
        if iou_type not in MASK_TYPES:
            raise ValueError(f"LVISSegmEval: iou_type {iou_type!r} is not supported (segm, boundary; for bbox: LVISEval)")
        boundary_dilation(1, 1, dilation_ratio)                    # refuses a ratio <= 0
        self.dilation_ratio = float(dilation_ratio)
        self._set_cuts(max_dets, max_dets_per_cat)
        self._setup(lvis_gt, lvis_dt, iou_type, device)

    def _setup(self, lvis_gt, lvis_dt, iou_type, device):
        super()._setup(lvis_gt, None, iou_type, device)
        for im in self.dataset["images"]:
            if not all(isinstance(im.get(f), (int, np.integer)) and not isinstance(im.get(f), bool) and im[f] >= 1 for f in ("height", "width")):
                raise ValueError(f"LVISSegmEval: image {im.get('id')} of the ground truth has no height and width")
        self._image_hw = np.zeros((len(self.img_ids), 2), np.int64)
        for im in self.dataset["images"]:
            self._image_hw[self._img_index[im["id"]]] = (im["height"], im["width"])
        if lvis_dt is not None:
            self._add_given(lvis_dt)

    def reset(self):
        super().reset()
        self._masks = _MaskStore(self.device)

    def _check_sizes(self, img, sizes, what):
        """Every mask of a known image (img: image indices, -1 = unknown) has that image's size."""
        img, sizes = np.asarray(img, np.int64).reshape(-1), np.asarray(sizes, np.int64).reshape(-1, 2)
        known = img >= 0
        if not known.any():
            return
        wrong = np.flatnonzero(known & (sizes != self._image_hw[np.where(known, img, 0)]).any(1))
        if wrong.size:
            j = int(wrong[0])
            h, w = self._image_hw[img[j]]
            raise ValueError(f"LVISSegmEval: a {what} mask of image {self.img_ids[img[j]]} is {sizes[j][0]}x{sizes[j][1]}, the image {h}x{w}")

    # ---- detections
    def add(self, image_id, category_ids, scores, masks=None):
        """GroupedEval.add with masks in place of boxes: an RLEBatch (MaskRCNN(mask_format="rle")) or dense [n, H, W] / [n, 1, H, W]
        probabilities (`> 0.5` through ops.mask_rle_dense)."""
        if masks is not None:                                      # without masks DetectionStore.add refuses below
            if not isinstance(masks, RLEBatch):
                masks = ops.mask_rle_dense(torch.as_tensor(masks, device=self.device).to(torch.float32), 0.5)
            if torch.is_tensor(image_id) and image_id.dim() > 0:   # one id per detection: a host read of the ids
                img = image_indices(image_id, len(masks), self.img_ids, self._img_index, self.device, "LVISSegmEval.add").cpu().numpy()
            else:
                img = [self._img_index.get(image_id.item() if torch.is_tensor(image_id) else image_id, -1)]
            self._check_sizes(img, [masks.size] * len(img), "detection")
        self._dets.add("LVISSegmEval.add", image_id, category_ids, scores, None, masks)
        self._masks.add_batch(masks)

    def add_results(self, results):
        """LVIS result dicts (`image_id`, `category_id`, `score`, `segmentation`); a `bbox` is not read."""
        if not results:
            return
        for r in results:
            if "segmentation" not in r:
                raise ValueError("LVISSegmEval: a result without `segmentation`")
        store = _MaskStore(self.device)
        store.add_segmentations([r["segmentation"] for r in results])
        self._check_sizes([self._img_index.get(r["image_id"], -1) for r in results], store.tensors()[4], "detection")
        self._masks.extend(store)
        self._dets.add_results(results)

    # ---- ground truth
    def _build_ground_truth(self):
        """The annotations' masks in slot order: polygons through polygons.segmentations_to_rle (one conversion), run lengths as they are."""
        gt = super()._build_ground_truth()
        anns = [self._anns[o][1] for o in gt["order"]]
        for a in anns:
            if "segmentation" not in a:
                raise ValueError(f"LVISSegmEval: annotation {a.get('id')} of the ground truth has no segmentation")
        segs = [a["segmentation"] for a in anns]
        which = [j for j, s in enumerate(segs) if is_polygon_segmentation(s)]
        store = _MaskStore(self.device)
        if which:
            hw = [tuple(int(v) for v in self._image_hw[self._img_index[anns[j]["image_id"]]]) for j in which]
            r = segmentations_to_rle([segs[j] for j in which], hw, self.device)
        if which and len(which) == len(segs):                      # LVIS's own form: the run lengths stay on the device
            store.add_batch(r)
        else:
            if which:                                              # mixed forms: the polygons join the others as count lists
                host = np.ascontiguousarray(r.counts.detach().cpu().numpy(), dtype=np.int32)
                for n, j in enumerate(which):
                    segs[j] = {"size": [int(r.sizes[n][0]), int(r.sizes[n][1])], "counts": host[r.offsets[n]:r.offsets[n + 1]]}
            store.add_segmentations(segs)
        gt["counts"], gt["runs"], _area, gt["box"], gt["sizes"] = store.tensors()
        if self.iou_type == "boundary":
            gt["boundary"] = store.boundaries(self.dilation_ratio)
        self._check_sizes(gt["key"] % max(len(self.img_ids), 1), gt["sizes"], "ground-truth")
        return gt

    def _mask_tensors(self):
        return self._masks.tensors()
