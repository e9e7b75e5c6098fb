"""COCO evaluation on the device: the twelve COCO statistics for `bbox` and `segm` and the ten of `keypoints` without pycocotools.

What pycocotools' COCOeval computes with a Python loop over images x categories x area ranges is tens of thousands of small independent
(image, category) groups; here they are three kernel passes (csrc/cocoeval_kernels.hip, include/mi355det.h "COCO evaluation"):

    add(...)        detections stay device tensors (boxes, scores, labels; masks as RLEBatch)
    evaluate()      torch sorts group the detections (plumbing) -> coco_iou -> coco_match
    accumulate()    one stable sort per category -> coco_accumulate -> precision / recall / scores on the host
    summarize()     numpy on the small result arrays; prints pycocotools' twelve lines and sets .stats
    summarize_per_category()    the same twelve numbers for every category on its own, read out of precision / recall (compare.py)
    bootstrap(weights)          after evaluate(): the twelve numbers of resampled data sets, all replicates in one accumulate walk with integer
                                weights (csrc/bootstrap_kernels.hip); intervals and the paired test are compare.py

The slot layout evaluate() leaves behind, the detection lists and the accumulate and bootstrap passes are evalcore.py (GroupedEval); here are
COCO's cut (each group's detections in descending score order, stable, cut to 100), its match rule, the `segm` side and the summary.  The
LVIS rules (federated annotations, APr / APc / APf) are lviseval.py: another front end and match rule on the same base.
Polygon ground truth is converted first: COCOEval(polygons.dataset_to_rle(dataset), "segm").

`keypoints` (COCOEval(gt, "keypoints", sigmas=None)) is the same pipeline with another pair kernel and the two ground-truth
flags apart: coco_oks (csrc/oks_kernels.hip: the object keypoint similarity in coco_iou's ragged layout) -> keypoints_match -> the unchanged
coco_accumulate, at maxDets = 20 over the area ranges all / medium / large, summarised in pycocotools' ten lines.  Out of scope for
`keypoints`: tide.ErrorBreakdown and compare.Disagreement (boxes only), LVIS, and everything in the models and in ingest.

The masks of a `segm` evaluation live in a _MaskStore (also lviseval.LVISSegmEval's).  On a GPU a list of result dicts whose `counts` are
all strings - a results file - is decoded, checked and measured by csrc/rle_string_kernels.hip in one call (add_strings); every other form
is read on the host as before."""
import numpy as np
import torch

from . import ops
from .evalcore import (MASK_TYPES, REC_THRS, GroupedEval, bootstrap_cells, category_order, cell_mean, check_weights, group_offsets,  # noqa: F401 (re-exported)
                       image_indices, load_dataset, lookup, masked_mean, rank_in_run, rle_operands, score_then_key_order, sort_ground_truth)
from .polygons import PolygonRLE, is_polygon_segmentation
from .rle import RLEBatch, boundary_dilation, boundary_dilations, counts_stats, pack_strings, string_to_counts

MAX_DETS = [1, 10, 100]
AREA_LABELS = ["all", "small", "medium", "large"]
# the twelve statistics as (precision or recall, IoU threshold or all, area range, maxDets index), and the names the reference's notebooks use
STAT_ROWS = [(1, None, 0, 2), (1, .5, 0, 2), (1, .75, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
             (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2)]
STAT_NAMES = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]
# `keypoints`: one maxDets, no small range (pycocotools' Params.setKpParams), ten statistics in the same row form
KP_MAX_DETS = [20]
KP_AREA_RNG = [[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
KP_AREA_LABELS = ["all", "medium", "large"]
KP_STAT_ROWS = [(1, None, 0, 0), (1, .5, 0, 0), (1, .75, 0, 0), (1, None, 1, 0), (1, None, 2, 0),
                (0, None, 0, 0), (0, .5, 0, 0), (0, .75, 0, 0), (0, None, 1, 0), (0, None, 2, 0)]
KP_STAT_NAMES = ["AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl"]
# COCO's per-keypoint standard deviations of the 17 person keypoints (nose, eyes, ears, shoulders, elbows, wrists, hips, knees, ankles)
KP_SIGMAS = [v / 10 for v in (.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89)]
KP_MAX_K = 64                             # coco_oks' limit on the keypoints per instance


def _segmentation_counts(seg, bitmaps):
    """One annotation's or result's segmentation -> ((h, w), int32 counts), or a bitmap queued in `bitmaps` for the run-length kernels."""
    if isinstance(seg, RLEBatch):
        if len(seg) != 1:
            raise ValueError("COCOEval: an RLEBatch given as one segmentation must hold one mask")
        return seg.size, np.asarray(seg.counts_of(0), np.int32)
    if isinstance(seg, dict):
        size = (int(seg["size"][0]), int(seg["size"][1]))
        c = seg["counts"]
        return size, (string_to_counts(c) if isinstance(c, (str, bytes)) else np.asarray(c, np.int32))
    if torch.is_tensor(seg) or isinstance(seg, np.ndarray):
        m = torch.as_tensor(seg)
        if m.dim() != 2:
            raise ValueError("COCOEval: a bitmap segmentation must be [H, W]")
        bitmaps.append(m)
        return (int(m.shape[0]), int(m.shape[1])), None
    if is_polygon_segmentation(seg):
        raise NotImplementedError("COCOEval: polygon segmentations are not converted here; convert the data set first with "
                                  "polygons.dataset_to_rle, or give run lengths or bitmaps")
    raise ValueError(f"COCOEval: unsupported segmentation of type {type(seg).__name__}")


def _counts_strings(segs):
    """(sizes int32 [n, 2], the `counts` strings) where every segmentation is a dict whose counts are a str / bytes of a form the string
    kernels take (ASCII; 1 <= h, w and h*w < 2^31), else None: the host route reads - or refuses - everything else."""
    if not segs or not all(isinstance(s, dict) and isinstance(s.get("counts"), (str, bytes)) for s in segs):
        return None
    try:
        sizes = np.asarray([s["size"] for s in segs])
    except (KeyError, ValueError):
        return None
    if sizes.ndim != 2 or sizes.shape[1] != 2 or sizes.dtype.kind not in "iu":
        return None
    sizes = sizes.astype(np.int64)
    if (sizes < 1).any() or (sizes[:, 0] * sizes[:, 1] >= (1 << 31)).any() or (sizes >= (1 << 31)).any():
        return None
    strings = [s["counts"] for s in segs]
    if not all(c.isascii() for c in strings if isinstance(c, str)):
        return None
    return sizes.astype(np.int32), strings


class _MaskStore:
    """Run lengths of many masks in the concatenated counts / offsets form of RLEBatch, with each mask's size, area and tight box."""

    def __init__(self, dev):
        self.dev = torch.device(dev)
        self.counts, self.lens, self.area, self.bbox, self.sizes = [], [], [], [], []       # one entry per addition: tensors / host arrays

    def add_arrays(self, counts, lens, area, bbox, sizes):
        """Masks that are run lengths already: counts int32, area int64 [n], bbox int32 [n, 4] as tensors; lens [n], sizes [n, 2] on the
        host.  Every other way in ends here."""
        self.counts.append(counts.to(self.dev).to(torch.int32))
        self.lens.append(np.asarray(lens, np.int64).reshape(-1))
        self.area.append(area.to(self.dev))
        self.bbox.append(bbox.to(self.dev))
        self.sizes.append(np.asarray(sizes, np.int32).reshape(-1, 2))

    def extend(self, other):
        """The masks of another store of the same device, behind this one's."""
        for name in ("counts", "lens", "area", "bbox", "sizes"):
            getattr(self, name).extend(getattr(other, name))

    def add_strings(self, sizes, strings):
        """Masks given as `counts` strings, decoded, checked and measured by the string kernels (ops.rle_strings) in one call.  A refused
        mask goes through the host route once more, which raises what it raises for that string."""
        packed, offsets = pack_strings(strings)
        counts, runs, area, bbox, status = ops.rle_strings(packed, offsets, sizes, self.dev)
        if status is not None:
            bad = np.flatnonzero(status)
            parse = bad[(status[bad] & ops.RLESTR_PARSE) != 0]    # the host route decodes every string before it sums the first
            j = int(parse[0] if parse.size else bad[0])
            _MaskStore("cpu").add_segmentations([{"size": [int(sizes[j][0]), int(sizes[j][1])], "counts": strings[j]}])
            raise RuntimeError(f"COCOEval: the string kernels refuse mask {j} (status {int(status[j])}) and the host codec does not")
        self.add_arrays(counts, np.diff(runs), area, bbox, sizes)

    def add_batch(self, b):
        """An RLEBatch (one size for all its masks) or a polygons.PolygonRLE (a size per mask)."""
        one_size = isinstance(b, RLEBatch)
        if not one_size and not isinstance(b, PolygonRLE):
            raise TypeError(f"COCOEval: masks must be an RLEBatch or a PolygonRLE, not {type(b).__name__}")
        area, bbox = b.stats() if one_size else (b.area, b.bbox)
        self.add_arrays(b.counts, np.diff(np.asarray(b.offsets, np.int64)), area, bbox, [b.size] * len(b) if one_size else b.sizes)

    def add_segmentations(self, segs):
        """Segmentations in any accepted form, in order.  On a GPU, a list of nothing but `counts` strings goes through the string kernels
        (add_strings); everything else is read here on the host, bitmaps through ops.mask_rle_dense, one call per shape."""
        strings = _counts_strings(segs) if self.dev.type == "cuda" else None
        if strings is not None:
            return self.add_strings(*strings)
        bitmaps, parsed = [], []
        for s in segs:
            parsed.append(_segmentation_counts(s, bitmaps))
        by_shape, encoded = {}, {}
        for j, m in enumerate(bitmaps):
            by_shape.setdefault(tuple(m.shape), []).append(j)
        for shape, idx in by_shape.items():
            stack = torch.stack([bitmaps[j] for j in idx]).to(self.dev).to(torch.float32)
            b = ops.mask_rle_dense(stack, 0.5)
            for n, j in enumerate(idx):
                encoded[j] = np.asarray(b.counts_of(n), np.int32)
        nb, counts = 0, []
        for size, c in parsed:
            if c is None:
                c = encoded[nb]
                nb += 1
            if int(c.astype(np.int64).sum()) != size[0] * size[1] or (c < 0).any():
                raise ValueError(f"COCOEval: run lengths that do not add up to {size[0]}x{size[1]}")
            counts.append(c)
        flat = np.concatenate(counts) if counts else np.zeros(0, np.int32)
        lens = [len(c) for c in counts]
        sizes = [size for size, _c in parsed]
        area, bbox = counts_stats(flat, np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]), [size[0] for size in sizes])
        self.add_arrays(torch.from_numpy(np.ascontiguousarray(flat, np.int32)), lens, torch.from_numpy(area), torch.from_numpy(bbox), sizes)

    def _cat(self, area=True):
        """The five lists as one entry each: counts int32, area int64 [n] (None unless asked for), bbox int32 [n, 4] on the device; runs
        int64 [n + 1] and sizes int32 [n, 2] on the host."""
        cat = lambda xs, dt, shape: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt, device=self.dev)
        lens = np.concatenate(self.lens) if self.lens else np.zeros(0, np.int64)
        return (cat(self.counts, torch.int32, (0,)).contiguous(), np.concatenate([np.zeros(1, np.int64), np.cumsum(lens)]),
                cat(self.area, torch.int64, (0,)) if area else None, cat(self.bbox, torch.int32, (0, 4)),
                np.concatenate(self.sizes) if self.sizes else np.zeros((0, 2), np.int32))

    def _operands(self, counts, runs, area, bbox, sizes):
        return counts, torch.from_numpy(runs).to(self.dev), area.to(torch.float64), bbox.to(torch.float64).contiguous(), sizes

    def boundaries(self, dilation_ratio, budget_bytes=1 << 30):
        """tensors() of the masks' boundaries (ops.rle_boundary, each mask eroded by rle.boundary_dilation of its own size): one conversion
        of the whole store, one host read of the boxes and one of the run offsets."""
        counts, runs, _area, bbox, sizes = self._cat(area=False)
        return self._operands(*ops.rle_boundary(counts, runs, sizes, boundary_dilations(sizes, dilation_ratio), bbox, budget_bytes=budget_bytes),
                              sizes)

    def tensors(self):
        """counts int32, runs int64 [n + 1], area float64 [n], tight boxes float64 [n, 4] on the device; sizes int32 [n, 2] on the host."""
        return self._operands(*self._cat())


class COCOEval(GroupedEval):
    """COCOeval for `bbox`, `segm`, `boundary` or `keypoints` on the device.  `gt`: see load_dataset.  `boundary` (the COCO boundary-IoU
    API) takes exactly the inputs of `segm` and matches on min(mask IoU, boundary IoU), the boundaries eroded by rle.boundary_dilation(h,
    w, dilation_ratio); a detection's area and box stay its mask's.  Detections come in through add() (one image, device tensors) or
    add_results() (COCO result dicts); evaluate(), accumulate() and summarize() then follow pycocotools' protocol.

    `keypoints`: `sigmas` are the K per-keypoint standard deviations (None: COCO's 17 person values, KP_SIGMAS; another length serves
    another skeleton).  Every annotation that counts (a known image and category) must carry `keypoints`, 3K numbers x, y, v; a data set
    without any `keypoints` annotation is refused.  A ground truth is ignored when iscrowd or num_keypoints == 0, and only iscrowd lets it
    match again.  Where `num_keypoints` is missing, the number of keypoints with v > 0 stands in (pycocotools raises a KeyError there).  A
    detection's area and box are those of loadRes: over all K keypoints, box = [min x, min y, max x - min x, max y - min y], area = w * h."""
    kind, flag_field = "coco", "iscrowd"
    cuts = property(lambda self: self.max_dets)

    def __init__(self, gt, iou_type="bbox", device=None, dilation_ratio=0.02, sigmas=None):
        if iou_type not in ("bbox", "keypoints") + MASK_TYPES:
            raise ValueError(f"COCOEval: iou_type {iou_type!r} is not supported (bbox, segm, boundary, keypoints)")
        boundary_dilation(1, 1, dilation_ratio)                        # refuses a ratio <= 0
        self.dilation_ratio = float(dilation_ratio)
        self.on_keypoints = iou_type == "keypoints"
        self.stat_rows, self.stat_names, self.area_labels = (KP_STAT_ROWS, KP_STAT_NAMES, KP_AREA_LABELS) if self.on_keypoints else \
            (STAT_ROWS, STAT_NAMES, AREA_LABELS)
        if self.on_keypoints:
            self.sigmas = np.asarray(KP_SIGMAS if sigmas is None else sigmas, np.float64).reshape(-1)
            if not 1 <= self.sigmas.shape[0] <= KP_MAX_K or not (np.isfinite(self.sigmas).all() and (self.sigmas > 0).all()):
                raise ValueError(f"COCOEval: sigmas must be 1..{KP_MAX_K} positive numbers, one per keypoint")
        elif sigmas is not None:
            raise ValueError("COCOEval: sigmas belong to iou_type 'keypoints'")
        super().__init__(gt, iou_type, device, list(KP_MAX_DETS if self.on_keypoints else MAX_DETS))
        if self.on_keypoints:
            self.area_rng = np.asarray(KP_AREA_RNG, np.float64)
            if not any("keypoints" in a for a in self.dataset.get("annotations", [])):
                raise ValueError("COCOEval: keypoints evaluation needs a ground truth with `keypoints` annotations; this data set has none")
            for j, a in self._anns:
                kp = a.get("keypoints")
                if not isinstance(kp, (list, tuple)) or len(kp) != 3 * self.num_keypoints:
                    raise ValueError(f"COCOEval: annotation {a.get('id', j)!r} (position {j}) must have `keypoints`, a list of "
                                     f"{3 * self.num_keypoints} numbers (x, y, v of {self.num_keypoints} keypoints)")
        if self.on_masks:
            for _j, a in self._anns:
                if is_polygon_segmentation(a.get("segmentation")):
                    _segmentation_counts(a["segmentation"], [])            # raises NotImplementedError

    def reset(self):
        super().reset()
        self._masks = _MaskStore(self.device) if self.on_masks else None
        self._kp = []                                                  # `keypoints`: float64 [n, K, 2] per addition, on the device
        self.scores = self.stats = None

    num_keypoints = property(lambda self: int(self.sigmas.shape[0]))

    # ---- detections
    def _xy(self, keypoints, n, what):
        """[n, K, 3] or [n, K, 2] (also flat) -> x, y as float64 [n, K, 2] on the device; a detection's visibility is dropped."""
        K = self.num_keypoints
        kp = (keypoints.to(self.device) if torch.is_tensor(keypoints) else torch.tensor(keypoints, dtype=torch.float64, device=self.device))
        kp = kp.to(torch.float64)                                    # float32 model outputs are widened exactly; lists are read as float64
        if kp.numel() not in (n * K * 3, n * K * 2) or (kp.dim() == 3 and kp.shape[1] != K):
            raise ValueError(f"{what}: keypoints must be [n, {K}, 3] or [n, {K}, 2], one row per detection")
        return kp.reshape(n, K, 3 if kp.numel() == n * K * 3 else 2)[:, :, :2].contiguous()

    def add(self, image_id, category_ids, scores, boxes=None, masks=None, keypoints=None):
        """GroupedEval.add with, for `segm`, masks in place of boxes: an RLEBatch (MaskRCNN(mask_format="rle")) or dense [n, H, W] /
        [n, 1, H, W] probabilities (`> 0.5` through ops.mask_rle_dense); for `keypoints`, keypoints [n, K, 3] or [n, K, 2] (Keypoint
        R-CNN's output form; x and y are read, a third value is not)."""
        if self.on_keypoints:
            if keypoints is None:
                raise ValueError("COCOEval.add: keypoints evaluation needs keypoints")
            kp = self._xy(keypoints, int(torch.as_tensor(category_ids).numel()), "COCOEval.add")
        if self.on_masks and masks is not None and not isinstance(masks, RLEBatch):
            masks = ops.mask_rle_dense(torch.as_tensor(masks, device=self.device).to(torch.float32), 0.5)
        self._dets.add("COCOEval.add", image_id, category_ids, scores, boxes, masks)
        if self.on_masks:
            self._masks.add_batch(masks)
        if self.on_keypoints:
            self._kp.append(kp)

    def add_results(self, results):
        """COCO result dicts (`image_id`, `category_id`, `score` and `bbox`, `segmentation` or, flat x, y, v of the K keypoints,
        `keypoints`), e.g. the rows of to_coco_results."""
        if results and self.on_masks:
            self._masks.add_segmentations([r["segmentation"] for r in results])
        if results and self.on_keypoints:
            for j, r in enumerate(results):
                if len(r["keypoints"]) != 3 * self.num_keypoints:
                    raise ValueError(f"COCOEval.add_results: result {j} must have {3 * self.num_keypoints} keypoint numbers")
            self._kp.append(self._xy([r["keypoints"] for r in results], len(results), "COCOEval.add_results"))
        super().add_results(results)

    def _build_ground_truth(self):
        gt = super()._build_ground_truth()
        if self.on_masks:
            store = _MaskStore(self.device)
            store.add_segmentations([self._anns[o][1]["segmentation"] for o in gt["order"]])
            gt["counts"], gt["runs"], _area, gt["box"], gt["sizes"] = store.tensors()
            if self.iou_type == "boundary":
                gt["boundary"] = store.boundaries(self.dilation_ratio)
        if self.on_keypoints:
            anns = [self._anns[o][1] for o in gt["order"]]
            kp = np.asarray([a["keypoints"] for a in anns], np.float64).reshape(-1, self.num_keypoints, 3)
            labelled = np.asarray([int(a["num_keypoints"]) if "num_keypoints" in a else int((k[:, 2] > 0).sum()) for a, k in zip(anns, kp)],
                                  np.int64).reshape(-1)
            gt["flag"] = (gt["crowd"].astype(bool) | (labelled == 0)).astype(np.uint8)       # ignored; gt["crowd"] stays iscrowd alone
            gt["flag_dev"] = torch.from_numpy(gt["flag"]).to(self.device)
            gt["kp"] = torch.from_numpy(np.ascontiguousarray(kp)).to(self.device)
            gt["box"] = torch.from_numpy(np.asarray([a["bbox"] for a in anns], np.float64).reshape(-1, 4)).to(self.device)
            gt["vars"] = torch.from_numpy((self.sigmas * 2) ** 2).to(self.device)
        return gt

    def _group(self):
        """The front end: descending score (stable), then by group (stable), so each group's detections are in score order; cut to the
        largest maxDets.  For `segm` it also leaves coco_iou's run-length operands."""
        I = len(self.img_ids)
        img, cat_id, score, box = self._dets.tensors()
        cat, known = lookup(torch.tensor(self.cat_ids, dtype=torch.int64, device=self.device), cat_id)
        src = torch.nonzero(known & (img >= 0)).reshape(-1)
        key = cat[src] * I + img[src]
        perm = score_then_key_order(score[src], key)
        key = key[perm]
        rank = rank_in_run(key)
        top = rank < self.max_dets[-1]
        dt_index, key, rank = src[perm][top], key[top], rank[top].to(torch.int32)
        if self.iou_type == "bbox":
            self._rle = None
            return self._layout(key, dt_index, score, box, rank=rank)
        if self.on_keypoints:                                          # loadRes: area and box over all K keypoints
            kp = torch.cat(self._kp) if self._kp else torch.zeros((0, self.num_keypoints, 2), dtype=torch.float64, device=self.device)
            lo, hi = kp.min(1).values, kp.max(1).values
            wh = hi - lo
            iou_size = self._layout(key, dt_index, score, torch.cat([lo, wh], 1), wh[:, 0] * wh[:, 1], rank)
            self.dt_kp, self.gt_kp = kp[dt_index].contiguous(), self._ground_truth()["kp"]
            return iou_size
        gt = self._ground_truth()
        masks = self._masks.tensors()
        iou_size = self._layout(key, dt_index, score, masks[3], masks[2], rank)
        self._set_rle(masks, gt, src, img)
        return iou_size

    def _match(self, iou_size):
        """coco_iou (crowd pairs take the crowd union), then coco_match with iscrowd as the flag."""
        thr, rng, _rec = self._params()
        if self.on_keypoints:                                          # coco_oks (no crowd rule), then the match with the two flags apart
            self.iou = ops.coco_oks(self.dt_offsets, self.gt_offsets, self.iou_offsets, iou_size, self.dt_kp, self.gt_kp, self.gt_boxes,
                                    self.gt_area, self._ground_truth()["vars"])
            self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore = ops.keypoints_match(
                self.dt_offsets, self.gt_offsets, self.iou_offsets, self.iou, self.dt_area, self.gt_area, self.gt_flag, self.gt_crowd, thr, rng)
            return
        self.iou = self._iou(iou_size)
        self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore = ops.coco_match(
            self.dt_offsets, self.gt_offsets, self.iou_offsets, self.iou, self.dt_area, self.gt_area, self.gt_flag, thr, rng)

    def accumulate(self):
        """precision [10, 101, K, 4, 3], recall [10, K, 4, 3], scores [10, 101, K, 4, 3] as float64 numpy arrays (`keypoints`: 3 area
        ranges and 1 maxDets in place of 4 and 3)."""
        self.precision, self.recall, self.scores = (x.cpu().numpy() for x in self._accumulate())
        return self

    def _stat_rows(self, ap_sum, recall):
        """bootstrap(): the twelve (`keypoints`: ten) statistics in stat_rows order."""
        out = []
        for ap, thr, a, m in self.stat_rows:
            cells = ap_sum if ap else recall
            if thr is not None:
                cells = cells[:, [int(j) for j in np.flatnonzero(np.isclose(self.iou_thrs, thr))]]
            out.append(cell_mean(cells[:, :, :, a, m], len(self.rec_thrs) if ap else 1))
        return out

    def _stat(self, ap, iou_thr=None, area=0, max_det=2, cat=None):
        s = self.precision if ap else self.recall
        if iou_thr is not None:
            s = s[np.isclose(self.iou_thrs, iou_thr)]
        if cat is not None:                                        # one category's slice: pycocotools with params.catIds = [that category]
            s = s[:, :, cat:cat + 1] if ap else s[:, cat:cat + 1]
        return masked_mean(s[:, :, :, area, max_det] if ap else s[:, :, area, max_det])

    def summarize(self, file=None):
        """Prints pycocotools' twelve lines (`keypoints`: its ten, all at maxDets= 20) and sets .stats (float64 [12] or [10])."""
        if self.precision is None:
            raise RuntimeError("COCOEval.summarize: call accumulate() first")
        stats = np.zeros(len(self.stat_rows), np.float64)
        for n, (ap, thr, a, m) in enumerate(self.stat_rows):
            stats[n] = self._stat(ap, thr, a, m)
            title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
            span = f"{self.iou_thrs[0]:0.2f}:{self.iou_thrs[-1]:0.2f}" if thr is None else f"{thr:0.2f}"
            print(f" {title:<18} {kind} @[ IoU={span:<9} | area={self.area_labels[a]:>6s} | maxDets={self.max_dets[m]:>3d} ] = {stats[n]:0.3f}", file=file)
        self.stats = stats
        return stats

    def summarize_per_category(self):
        """The twelve (`keypoints`: ten) statistics of every category on its own, float64 [K, 12]: row k is what summarize() would give with only cat_ids[k]
        evaluated (pycocotools with params.catIds = [cat_ids[k]], which the reference's notebooks/get_map.py:54-60 runs once per category).
        Read out of precision / recall by category: no new pass, nothing printed, .stats untouched."""
        if self.precision is None:
            raise RuntimeError("COCOEval.summarize_per_category: call accumulate() first")
        out = np.zeros((len(self.cat_ids), len(self.stat_rows)), np.float64)
        for k in range(len(self.cat_ids)):
            for n, (ap, thr, a, m) in enumerate(self.stat_rows):
                out[k, n] = self._stat(ap, thr, a, m, cat=k)
        return out
