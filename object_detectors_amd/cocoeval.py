"""COCO evaluation on the device: the twelve COCO statistics for `bbox` and `segm` without pycocotools.

What pycocotools' COCOeval computes with a Python loop over images x categories x area ranges is tens of thousands of small independent
(image, category) groups; here they are three kernel passes (csrc/cocoeval_kernels.hip, include/mi355det.h "COCO evaluation"):

    add(...)        detections stay device tensors (boxes, scores, labels; masks as RLEBatch)
    evaluate()      torch sorts group the detections (plumbing) -> coco_iou -> coco_match
    accumulate()    one stable sort per category -> coco_accumulate -> precision / recall / scores on the host
    summarize()     numpy on the small result arrays; prints pycocotools' twelve lines and sets .stats
    summarize_per_category()    the same twelve numbers for every category on its own, read out of precision / recall (compare.py)
    bootstrap(weights)          after evaluate(): the twelve numbers of resampled data sets, all replicates in one accumulate walk with integer
                                weights (csrc/bootstrap_kernels.hip); intervals and the paired test are compare.py

Slot layout after evaluate(): detections and ground truths are each sorted category-major, image second (the order of `cat_ids`, `img_ids`);
within a group the detections are in descending score order (stable, cut to 100) and the ground truths in annotation order.
`group_keys[j] = category index * len(img_ids) + image index`; group j owns the slots `dt_offsets[j]:dt_offsets[j + 1]`,
`gt_offsets[j]:gt_offsets[j + 1]` and the row-major [D, G] matrix at `iou[iou_offsets[j]]`.  `dt_index` / `gt_index` map a slot back to the
detection's position in the order it was added and to the annotation's position in the dataset.

The LVIS rules (federated annotations, APr / APc / APf) are lviseval.py: another front end and match rule on the same layout and kernels.
Out of scope: keypoints / OKS, and polygon ground truth (no polygon-to-mask conversion here: DESIGN.md)."""
import json

import numpy as np
import torch

from . import ops
from .rle import RLEBatch, counts_stats, string_to_counts

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
MAX_DETS = [1, 10, 100]
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
AREA_LABELS = ["all", "small", "medium", "large"]
# the twelve statistics as (precision or recall, IoU threshold or all, area range, maxDets index), and the names the reference's notebooks use
STAT_ROWS = [(1, None, 0, 2), (1, .5, 0, 2), (1, .75, 0, 2), (1, None, 1, 2), (1, None, 2, 2), (1, None, 3, 2),
             (0, None, 0, 0), (0, None, 0, 1), (0, None, 0, 2), (0, None, 1, 2), (0, None, 2, 2), (0, None, 3, 2)]
STAT_NAMES = ["AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl"]


def load_dataset(gt):
    """A path to a COCO json, a dataset dict, or any object whose `.dataset` is one (a pycocotools COCO, never imported here)."""
    if isinstance(gt, (str, bytes)) or hasattr(gt, "__fspath__"):
        with open(gt) as f:
            gt = json.load(f)
    elif not isinstance(gt, dict):
        gt = getattr(gt, "dataset", None)
    if not isinstance(gt, dict) or "images" not in gt or "categories" not in gt:
        raise ValueError("COCOEval: the ground truth must be a COCO json path, a dataset dict or an object with a .dataset dict")
    return gt


def _is_polygon(seg):
    return isinstance(seg, (list, tuple)) and (len(seg) == 0 or isinstance(seg[0], (list, tuple, int, float)))


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
    if _is_polygon(seg):
        raise NotImplementedError("COCOEval: polygon segmentations need the polygon-to-mask conversion (pycocotools frPyObjects), which is out "
                                  "of scope here (DESIGN.md); give run lengths or bitmaps")
    raise ValueError(f"COCOEval: unsupported segmentation of type {type(seg).__name__}")


class _MaskStore:
    """Run lengths of many masks in the concatenated counts / offsets form of RLEBatch, with each mask's size, area and tight box."""

    def __init__(self, dev):
        self.dev = dev
        self.counts, self.lens, self.area, self.bbox, self.sizes = [], [], [], [], []

    def add_batch(self, b):
        area, bbox = b.stats()
        self.counts.append(b.counts.to(self.dev).to(torch.int32))
        self.lens.extend(b.offsets[k + 1] - b.offsets[k] for k in range(len(b)))
        self.area.append(area.to(self.dev))
        self.bbox.append(bbox.to(self.dev))
        self.sizes.extend([b.size] * len(b))

    def add_segmentations(self, segs):
        """Segmentations in any accepted form, in order.  Bitmaps go through ops.mask_rle_dense, one call per shape."""
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
        groups = {}
        for j, (size, _c) in enumerate(parsed):
            groups.setdefault(size, []).append(j)
        flat = np.concatenate(counts) if counts else np.zeros(0, np.int32)
        area, bbox = np.zeros(len(parsed), np.int64), np.zeros((len(parsed), 4), np.int32)
        for size, idx in groups.items():                       # the tight boxes need the column height
            sub_off = [0]
            for j in idx:
                sub_off.append(sub_off[-1] + len(counts[j]))
            sub = np.concatenate([counts[j] for j in idx])
            area[idx], bbox[idx] = counts_stats(sub, sub_off, size[0])
        self.counts.append(torch.from_numpy(np.ascontiguousarray(flat, np.int32)).to(self.dev))
        self.lens.extend(len(c) for c in counts)
        self.area.append(torch.from_numpy(area).to(self.dev))
        self.bbox.append(torch.from_numpy(bbox).to(self.dev))
        self.sizes.extend(size for size, _c in parsed)

    def tensors(self):
        """counts int32, runs int64 [n + 1], area float64 [n], tight boxes float64 [n, 4] on the device; sizes int32 [n, 2] on the host."""
        cat = lambda xs, dt, shape: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt, device=self.dev)
        runs = torch.from_numpy(np.concatenate([[0], np.cumsum(np.asarray(self.lens, np.int64))]).astype(np.int64)).to(self.dev)
        return (cat(self.counts, torch.int32, (0,)).contiguous(), runs, cat(self.area, torch.int64, (0,)).to(torch.float64),
                cat(self.bbox, torch.int32, (0, 4)).to(torch.float64).contiguous(), np.asarray(self.sizes, np.int32).reshape(-1, 2))


def _image_sizes(sizes, img, num_images, what):
    """Per-image [h, w] of one side's masks ([0, 0]: none); masks of one image must agree."""
    out = np.zeros((num_images, 2), np.int32)
    for s, i in zip(sizes, img):
        if out[i].any() and (out[i] != s).any():
            raise ValueError(f"COCOEval: the {what} masks of one image differ in size")
        out[i] = s
    return out


# ---- plain helpers of the slot layout, shared with lviseval.py
def sort_ground_truth(anns, cat_index, img_index, num_images):
    """[(position, annotation)] -> (their group keys category index * num_images + image index, sorted; the stable order that sorts them)."""
    key = np.asarray([cat_index[a["category_id"]] * num_images + img_index[a["image_id"]] for _j, a in anns], np.int64)
    order = np.argsort(key, kind="mergesort")
    return key[order], order


def group_offsets(keys, k):
    """Sorted unique group keys [ng] and the (sorted) keys of one side's slots -> slots per group [ng], offsets [ng + 1]."""
    ng, dev = int(keys.shape[0]), keys.device
    c = torch.bincount(torch.searchsorted(keys, k), minlength=ng) if ng else torch.zeros(0, dtype=torch.int64, device=dev)
    return c, torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(c, 0)])


def image_indices(image_id, n, img_ids, img_index, dev, what):
    """The image of n detections - one id for all, or a tensor [n] of ids - as int64 [n] positions in the sorted `img_ids` on the device
    (`img_index`: id -> position); -1 for an image the ground truth does not know."""
    if torch.is_tensor(image_id) and image_id.dim() > 0:
        ids = image_id.to(dev).to(torch.int64).reshape(-1)
        if ids.shape[0] != n:
            raise ValueError(f"{what}: one image id per detection, or one for all")
        table = torch.tensor(img_ids, dtype=torch.int64, device=dev)
        i = torch.searchsorted(table, ids).clamp_(max=max(len(img_ids) - 1, 0))
        return torch.where(table[i] == ids, i, torch.full_like(i, -1)) if len(img_ids) else torch.full_like(ids, -1)
    i = img_index.get(image_id.item() if torch.is_tensor(image_id) else image_id, -1)
    return torch.full((n,), i, dtype=torch.int64, device=dev)


def category_order(cat_dt_offsets, dt_score):
    """Per category its detection slots in descending score order (stable over the image order the slots are in): coco_accumulate's `order`."""
    cat_of = torch.searchsorted(cat_dt_offsets, torch.arange(int(dt_score.shape[0]), device=dt_score.device), right=True) - 1
    o1 = torch.sort(-dt_score, stable=True).indices
    o2 = torch.sort(cat_of[o1], stable=True).indices
    return o1[o2].contiguous()


# ---- bootstrap replicates (csrc/bootstrap_kernels.hip), shared with lviseval.py
def check_weights(weights, num_images, what):
    """Bootstrap weights, an integer numpy array or tensor [B, num_images] without negative entries -> an int32 tensor (on the device it
    came from); anything else is a ValueError."""
    if not torch.is_tensor(weights):
        arr = np.asarray(weights)
        if arr.dtype.kind not in "iu":
            raise ValueError(f"{what}: the weights must be integers, not {arr.dtype}")
        weights = torch.from_numpy(np.ascontiguousarray(arr.astype(np.int64) if arr.dtype.kind == "u" else arr))
    if weights.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        raise ValueError(f"{what}: the weights must be integers, not {weights.dtype}")
    if weights.dim() != 2 or int(weights.shape[1]) != num_images:
        raise ValueError(f"{what}: the weights must be [replicates, {num_images}] (one column per entry of img_ids), not {list(weights.shape)}")
    if weights.numel() and (int(weights.min()) < 0 or int(weights.max()) > 2 ** 31 - 1):
        raise ValueError(f"{what}: the weights must lie in 0 .. 2^31 - 1")
    return weights.to(torch.int32)


def bootstrap_cells(ev, weights, max_dets, cell_budget_bytes):
    """The replicate cells of an evaluated COCOEval / LVISEval, a chunk of replicates at a time: yields (ap_sum, recall), float64
    [chunk, T, K, A, M] on the device (mi355det_coco_bootstrap).  `weights`: int32 [B, images]; a chunk's two buffers stay within
    `cell_budget_bytes` (one replicate at least).  A replicate's cells do not depend on the chunk it falls into."""
    dev, I, K = ev.device, len(ev.img_ids), len(ev.cat_ids)
    T, A, M = len(ev.iou_thrs), int(ev.area_rng.shape[0]), len(max_dets)
    B = int(weights.shape[0])
    chunk = max(1, int(cell_budget_bytes) // max(2 * 8 * T * K * A * M, 1))
    if K == 0 or I == 0:                                          # nothing to evaluate: every cell is -1, no launch
        for b0 in range(0, B, chunk):
            none = torch.full((min(chunk, B - b0), T, K, A, M), -1.0, dtype=torch.float64, device=dev)
            yield none, none.clone()
        return
    order = category_order(ev.cat_dt_offsets, ev.dt_score)
    rec = torch.from_numpy(np.ascontiguousarray(ev.rec_thrs, np.float64)).to(dev)
    for b0 in range(0, B, chunk):
        w = weights[b0:b0 + chunk].to(dev).t().contiguous()                              # [images, chunk]: replicate-minor
        yield ops.coco_bootstrap(ev.cat_dt_offsets, ev.cat_gt_offsets, order, ev.dt_rank, ev.dt_match, ev.dt_ignore, ev.gt_ignore, max_dets, rec,
                                 ev.dt_image, ev.gt_image, w)


def _row_sums(v):
    """[B, n] -> [B], each row summed by halving (zero-padded to a power of two): elementwise additions only, so a row's sum has one fixed
    order whatever the number of rows it is computed with - a replicate's statistics do not depend on the chunk it falls into."""
    size = 1 << max(int(v.shape[1]) - 1, 0).bit_length()
    v = torch.nn.functional.pad(v, (0, size - int(v.shape[1])))
    while size > 1:
        size >>= 1
        v = v[:, :size] + v[:, size:]
    return v[:, 0]


def cell_mean(cells, per_cell):
    """pycocotools' mean(s[s > -1]) of each replicate, regrouped: cells [B, ...] (-1: not valid) -> sum of the valid cells / (per_cell *
    their number), -1 where none is valid; float64 [B] on the device.  `per_cell`: 101 for ap_sum (a cell is a sum of 101 values), 1 for
    recall."""
    v = cells.reshape(cells.shape[0], -1)
    valid = v > -1
    n = valid.sum(1)
    total = _row_sums(torch.where(valid, v, torch.zeros_like(v)))
    return torch.where(n > 0, total / (per_cell * n.clamp(min=1)).to(torch.float64), torch.full_like(total, -1.0))


def run_bootstrap(ev, weights, max_dets, stat_rows, num_stats, cell_budget_bytes, return_cells, what):
    """bootstrap() of both evaluators: `stat_rows(ap_sum, recall)` -> the `num_stats` statistics of a chunk as a list of [chunk] tensors."""
    w = check_weights(weights, len(ev.img_ids), what)
    if ev.iou is None:
        raise RuntimeError(f"{what}: call evaluate() first")
    none = torch.zeros((0, len(ev.iou_thrs), len(ev.cat_ids), int(ev.area_rng.shape[0]), len(max_dets)), dtype=torch.float64, device=ev.device)
    stats, aps, rcs = [torch.zeros((0, num_stats), dtype=torch.float64, device=ev.device)], [none], [none]          # no replicate: empty results
    for ap_sum, recall in bootstrap_cells(ev, w, max_dets, cell_budget_bytes):
        stats.append(torch.stack(stat_rows(ap_sum, recall), 1))
        if return_cells:
            aps.append(ap_sum)
            rcs.append(recall)
    out = torch.cat(stats).cpu().numpy()
    return (out, (torch.cat(aps), torch.cat(rcs))) if return_cells else out


class COCOEval:
    """COCOeval for `bbox` or `segm` on the device.  `gt`: see load_dataset.  Detections come in through add() (one image, device tensors) or
    add_results() (COCO result dicts); evaluate(), accumulate() and summarize() then follow pycocotools' protocol."""

    def __init__(self, gt, iou_type="bbox", device=None):
        if iou_type not in ("bbox", "segm"):
            raise ValueError(f"COCOEval: iou_type {iou_type!r} is not supported (bbox, segm; keypoints / OKS are out of scope)")
        self.iou_type = iou_type
        self.dataset = load_dataset(gt)
        self.device = torch.device("cuda:0" if device is None else device)
        self.img_ids = sorted(set(im["id"] for im in self.dataset["images"]))
        self.cat_ids = sorted(c["id"] for c in self.dataset["categories"])
        self._img_index = {v: i for i, v in enumerate(self.img_ids)}
        self._cat_index = {v: i for i, v in enumerate(self.cat_ids)}
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rng = IOU_THRS, REC_THRS, list(MAX_DETS), np.asarray(AREA_RNG, np.float64)
        anns = [(j, a) for j, a in enumerate(self.dataset.get("annotations", []))
                if a["image_id"] in self._img_index and a["category_id"] in self._cat_index]
        if iou_type == "segm":
            for _j, a in anns:
                if _is_polygon(a.get("segmentation")):
                    _segmentation_counts(a["segmentation"], [])            # raises NotImplementedError
        self._anns = anns
        self._gt = None
        self.reset()

    def reset(self):
        """Forget the detections (the ground truth stays)."""
        self._img, self._cat, self._score, self._box = [], [], [], []
        self._masks = _MaskStore(self.device) if self.iou_type == "segm" else None
        self.num_added = 0
        self.precision = self.recall = self.scores = self.stats = None
        self.iou = None

    # ---- detections
    def add(self, image_id, category_ids, scores, boxes=None, masks=None):
        """The detections of one image (or, with image_id a tensor [n], of many): category_ids [n], scores [n] and, for `bbox`, boxes
        [n, 4] as [x, y, w, h]; for `segm`, masks as an RLEBatch (MaskRCNN(mask_format="rle")) or dense [n, H, W] / [n, 1, H, W] probabilities (`> 0.5` through ops.mask_rle_dense).
        Tensors stay on the device; float32 is widened exactly."""
        dev = self.device
        cat = torch.as_tensor(category_ids, device=dev).to(torch.int64).reshape(-1)
        n = int(cat.shape[0])
        score = torch.as_tensor(scores, device=dev).to(torch.float64).reshape(-1)
        if score.shape[0] != n:
            raise ValueError("COCOEval.add: one score per detection")
        if self.iou_type == "bbox":
            if boxes is None:
                raise ValueError("COCOEval.add: bbox evaluation needs boxes")
            box = torch.as_tensor(boxes, device=dev).to(torch.float64).reshape(-1, 4)
            if box.shape[0] != n:
                raise ValueError("COCOEval.add: one box per detection")
            self._box.append(box)
        else:
            if masks is None:
                raise ValueError("COCOEval.add: segm evaluation needs masks")
            batch = masks if isinstance(masks, RLEBatch) else ops.mask_rle_dense(torch.as_tensor(masks, device=dev).to(torch.float32), 0.5)
            if len(batch) != n:
                raise ValueError("COCOEval.add: one mask per detection")
            self._masks.add_batch(batch)
        self._img.append(image_indices(image_id, n, self.img_ids, self._img_index, dev, "COCOEval.add"))
        self._cat.append(cat)
        self._score.append(score)
        self.num_added += n

    def add_results(self, results):
        """COCO result dicts (`image_id`, `category_id`, `score` and `bbox` or `segmentation`), e.g. the rows of to_coco_results."""
        if not results:
            return
        dev = self.device
        if self.iou_type == "bbox":
            self._box.append(torch.tensor([r["bbox"] for r in results], dtype=torch.float64, device=dev).reshape(-1, 4))
        else:
            self._masks.add_segmentations([r["segmentation"] for r in results])
        self._img.append(torch.tensor([self._img_index.get(r["image_id"], -1) for r in results], dtype=torch.int64, device=dev))
        self._cat.append(torch.tensor([r["category_id"] for r in results], dtype=torch.int64, device=dev))
        self._score.append(torch.tensor([r["score"] for r in results], dtype=torch.float64, device=dev))
        self.num_added += len(results)

    # ---- ground truth, sorted category-major once
    def _ground_truth(self):
        if self._gt is not None:
            return self._gt
        dev, I = self.device, len(self.img_ids)
        anns = self._anns
        key, order = sort_ground_truth(anns, self._cat_index, self._img_index, I)
        gt = {"key": key, "index": np.asarray([anns[o][0] for o in order], np.int64),
              "area": np.asarray([float(anns[o][1]["area"]) for o in order], np.float64),
              "crowd": np.asarray([1 if anns[o][1].get("iscrowd", 0) else 0 for o in order], np.uint8)}
        if self.iou_type == "bbox":
            gt["box"] = torch.from_numpy(np.asarray([anns[o][1]["bbox"] for o in order], np.float64).reshape(-1, 4)).to(dev)
        else:
            store = _MaskStore(dev)
            store.add_segmentations([anns[o][1]["segmentation"] for o in order])
            gt["counts"], gt["runs"], _area, gt["box"], gt["sizes"] = store.tensors()
        for k in ("key", "area", "crowd"):
            gt[k + "_dev"] = torch.from_numpy(gt[k]).to(dev)
        self._gt = gt
        return gt

    def evaluate(self):
        """Group, IoU, match.  Leaves iou / iou_offsets / dt_offsets / gt_offsets / group_keys and the four match arrays dt_match, dt_ignore
        [4, 10, num_dt], gt_match [4, 10, num_gt], gt_ignore [4, num_gt] on the device (module docstring: slot layout)."""
        dev, I, K = self.device, len(self.img_ids), len(self.cat_ids)
        gt = self._ground_truth()
        i64 = lambda xs: torch.cat(xs) if xs else torch.zeros(0, dtype=torch.int64, device=dev)
        img, cat_id = i64(self._img), i64(self._cat)
        score = torch.cat(self._score) if self._score else torch.zeros(0, dtype=torch.float64, device=dev)
        cats = torch.tensor(self.cat_ids, dtype=torch.int64, device=dev)
        if K:
            cat = torch.searchsorted(cats, cat_id).clamp_(max=K - 1)
            known = (cats[cat] == cat_id) & (img >= 0)
        else:
            cat, known = torch.zeros_like(cat_id), torch.zeros_like(cat_id, dtype=torch.bool)
        # descending score (stable), then by group (stable): each group's detections in score order; cut to the largest maxDets
        src = torch.nonzero(known).reshape(-1)
        key = cat[src] * I + img[src]
        o1 = torch.sort(-score[src], stable=True).indices
        o2 = torch.sort(key[o1], stable=True).indices
        perm = o1[o2]
        key = key[perm]
        n = int(key.shape[0])
        _u, per = torch.unique_consecutive(key, return_counts=True)
        rank = torch.arange(n, device=dev) - torch.repeat_interleave(torch.cumsum(per, 0) - per, per)
        top = rank < self.max_dets[-1]
        self.dt_index = src[perm][top]
        key, self.dt_rank = key[top], rank[top].to(torch.int32)
        self.dt_score = score[self.dt_index].contiguous()
        self.dt_image, self.gt_image = (key % max(I, 1)).to(torch.int32), (gt["key_dev"] % max(I, 1)).to(torch.int32)       # bootstrap() weighs by them
        num_dt = int(key.shape[0])
        # the groups: every (category, image) with a detection or a ground truth
        keys = torch.unique(torch.cat([key, gt["key_dev"]]))
        ng = int(keys.shape[0])
        dc, self.dt_offsets = group_offsets(keys, key)
        gc, self.gt_offsets = group_offsets(keys, gt["key_dev"])
        self.iou_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(dc * gc, 0)])
        iou_size = int(self.iou_offsets[-1])                      # the one host read: it sizes the IoU buffer
        self.group_keys, self.gt_index = keys, gt["index"]
        cat_edges = torch.arange(K + 1, device=dev) * I
        self.cat_dt_offsets = torch.searchsorted(key, cat_edges).contiguous()
        self.cat_gt_offsets = torch.searchsorted(gt["key_dev"], cat_edges).contiguous()
        if self.iou_type == "bbox":
            dt_box = (torch.cat(self._box) if self._box else torch.zeros((0, 4), dtype=torch.float64, device=dev))[self.dt_index].contiguous()
            self.dt_area = (dt_box[:, 2] * dt_box[:, 3]).contiguous()
            rle = None
        else:
            counts, runs, area, box, sizes = self._masks.tensors()
            dt_box, self.dt_area = box[self.dt_index].contiguous(), area[self.dt_index].contiguous()
            host_keys = keys.cpu().numpy() % max(I, 1)            # the groups' image indices
            dt_img = _image_sizes(sizes[src.cpu().numpy()], img[src].cpu().numpy(), I, "detection")
            gt_img = _image_sizes(gt["sizes"], gt["key"] % max(I, 1), I, "ground-truth")
            has = lambda c: (c > 0).cpu().numpy()[:, None]
            rle = {"dt": (counts, runs, self.dt_index.contiguous()), "gt": (gt["counts"], gt["runs"], None),
                   "dt_sizes": dt_img[host_keys] * has(dc), "gt_sizes": gt_img[host_keys] * has(gc)}
        self.dt_boxes = dt_box
        self.iou = ops.coco_iou(self.dt_offsets, self.gt_offsets, self.iou_offsets, iou_size, dt_box, gt["box"], gt["crowd_dev"], rle)
        thr = torch.from_numpy(np.ascontiguousarray(self.iou_thrs, np.float64)).to(dev)
        rng = torch.from_numpy(np.ascontiguousarray(self.area_rng, np.float64)).to(dev)
        self.dt_match, self.dt_ignore, self.gt_match, self.gt_ignore = ops.coco_match(
            self.dt_offsets, self.gt_offsets, self.iou_offsets, self.iou, self.dt_area, gt["area_dev"], gt["crowd_dev"], thr, rng)
        self.num_dt, self.num_gt, self.num_groups = num_dt, int(gt["key"].shape[0]), ng
        return self

    def accumulate(self):
        """precision [10, 101, K, 4, 3], recall [10, K, 4, 3], scores [10, 101, K, 4, 3] as float64 numpy arrays."""
        if self.iou is None:
            raise RuntimeError("COCOEval.accumulate: call evaluate() first")
        dev = self.device
        self.order = category_order(self.cat_dt_offsets, self.dt_score)
        rec = torch.from_numpy(np.ascontiguousarray(self.rec_thrs, np.float64)).to(dev)
        p, r, s = ops.coco_accumulate(self.cat_dt_offsets, self.cat_gt_offsets, self.order, self.dt_rank, self.dt_score, self.dt_match,
                                      self.dt_ignore, self.gt_ignore, self.max_dets, rec)
        self.precision, self.recall, self.scores = p.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()
        return self

    def bootstrap(self, weights, return_cells=False, cell_budget_bytes=1 << 30):
        """The twelve statistics of resampled data sets, float64 numpy [B, 12] in STAT_ROWS order.  `weights`: integers [B, len(img_ids)]
        (numpy or tensor, e.g. compare.bootstrap_weights); replicate b is the evaluation of the data set in which image i occurs
        weights[b, i] times (include/mi355det.h, "Bootstrap replicates").  Needs evaluate() only; the match arrays are read, and .precision,
        .recall and .stats stay as they are.  The replicates go through mi355det_coco_bootstrap in chunks whose two cell buffers stay within
        `cell_budget_bytes`; a replicate's cells and statistics are the same bits whatever the chunking.
        return_cells=True: -> (stats, (ap_sum, recall)), the cells float64 [B, 10, K, 4, 3] on the device: ap_sum = the sum of a cell's 101
        precision values, so the AP of category k alone is a mean over ap_sum[:, :, k] / 101; -1 marks a cell without ground truth."""
        R = len(self.rec_thrs)

        def rows(ap_sum, recall):
            out = []
            for ap, thr, a, m in STAT_ROWS:
                cells = ap_sum if ap else recall
                if thr is not None:
                    cells = cells[:, [int(j) for j in np.flatnonzero(np.isclose(self.iou_thrs, thr))]]
                out.append(cell_mean(cells[:, :, :, a, m], R if ap else 1))
            return out
        return run_bootstrap(self, weights, self.max_dets, rows, len(STAT_ROWS), cell_budget_bytes, return_cells, "COCOEval.bootstrap")

    def _stat(self, ap, iou_thr=None, area=0, max_det=2, cat=None):
        s = self.precision if ap else self.recall
        if iou_thr is not None:
            s = s[np.isclose(self.iou_thrs, iou_thr)]
        if cat is not None:                                        # one category's slice: pycocotools with params.catIds = [that category]
            s = s[:, :, cat:cat + 1] if ap else s[:, cat:cat + 1]
        s = s[:, :, :, area, max_det] if ap else s[:, :, area, max_det]
        s = s[s > -1]
        return np.float64(-1) if s.size == 0 else np.mean(s)

    def summarize(self, file=None):
        """Prints pycocotools' twelve lines and sets .stats (float64 [12])."""
        if self.precision is None:
            raise RuntimeError("COCOEval.summarize: call accumulate() first")
        stats = np.zeros(12, np.float64)
        for n, (ap, thr, a, m) in enumerate(STAT_ROWS):
            stats[n] = self._stat(ap, thr, a, m)
            title, kind = ("Average Precision", "(AP)") if ap else ("Average Recall", "(AR)")
            span = f"{self.iou_thrs[0]:0.2f}:{self.iou_thrs[-1]:0.2f}" if thr is None else f"{thr:0.2f}"
            print(f" {title:<18} {kind} @[ IoU={span:<9} | area={AREA_LABELS[a]:>6s} | maxDets={self.max_dets[m]:>3d} ] = {stats[n]:0.3f}", file=file)
        self.stats = stats
        return stats

    def summarize_per_category(self):
        """The twelve statistics of every category on its own, float64 [K, 12]: row k is what summarize() would give with only cat_ids[k]
        evaluated (pycocotools with params.catIds = [cat_ids[k]], which the reference's notebooks/get_map.py:54-60 runs once per category).
        Read out of precision / recall by category: no new pass, nothing printed, .stats untouched."""
        if self.precision is None:
            raise RuntimeError("COCOEval.summarize_per_category: call accumulate() first")
        out = np.zeros((len(self.cat_ids), 12), np.float64)
        for k in range(len(self.cat_ids)):
            for n, (ap, thr, a, m) in enumerate(STAT_ROWS):
                out[k, n] = self._stat(ap, thr, a, m, cat=k)
        return out
