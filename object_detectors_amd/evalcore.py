"""The evaluator core: the slot layout that the evaluation kernels read (csrc/cocoeval_kernels.hip, csrc/bootstrap_kernels.hip,
csrc/tide_kernels.hip) and everything the front ends on top of them share.  cocoeval.py and lviseval.py are GroupedEval with their own cut,
filter and match rule; compare.py and tide.py use the helpers and read an evaluator's public attributes.  DESIGN.md 7a states the contract.

Slot layout after evaluate(): detections and ground truths are each sorted category-major, image second (the order of `cat_ids`, `img_ids`);
within a group the detections are in descending score order (stable) and the ground truths in annotation order.
`group_keys[j] = category index * len(img_ids) + image index`; group j owns the slots `dt_offsets[j]:dt_offsets[j + 1]`,
`gt_offsets[j]:gt_offsets[j + 1]` and the row-major [D, G] matrix at `iou[iou_offsets[j]]`; category k owns the slots
`cat_dt_offsets[k]:cat_dt_offsets[k + 1]` and `cat_gt_offsets[k]:cat_gt_offsets[k + 1]`.  `dt_index` / `gt_index` map a slot back to the
detection's position in the order it was added and to the annotation's position in the dataset.  Per detection slot: `dt_score`,
`dt_boxes` [x, y, w, h], `dt_area`, `dt_image` (image index, int32) and `dt_rank` (rank within the group, int32; all zero where the
evaluator has no per-group cut).  Per ground-truth slot: `gt_boxes`, `gt_area`, `gt_flag` (uint8: the flag the match rule reads, iscrowd
or ignore), `gt_crowd` (uint8: what the IoU pass takes as crowd) and `gt_image`.  COCOEval with `keypoints` adds `dt_kp` [num_dt, K, 2] and
`gt_kp` [num_gt, K, 3] (float64), and its `gt_flag` is the ignore flag while `gt_crowd` alone lets a ground truth match again.  The match leaves `iou`, `dt_match`, `dt_ignore`
[4, 10, num_dt], `gt_match` [4, 10, num_gt] and `gt_ignore` [4, num_gt].  All of them are device tensors but `gt_index` (numpy)."""
import json

import numpy as np
import torch

from . import ops

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
MASK_TYPES = ("segm", "boundary")     # the evaluations over masks; "boundary" matches on min(mask IoU, boundary IoU)
NO_CUT = 2 ** 31 - 1                      # as the single "maxDets" of an accumulate pass: every rank passes


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


# ---- plain helpers of the slot layout
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


def lookup(table, keys):
    """keys in the sorted table, elementwise (both int64 on the device) -> (position, clamped into the table; whether the key is there)."""
    n = int(table.shape[0])
    if n == 0:
        return torch.zeros_like(keys), torch.zeros_like(keys, dtype=torch.bool)
    pos = torch.searchsorted(table, keys).clamp_(max=n - 1)
    return pos, table[pos] == keys


def member(table, keys):
    """keys in the sorted table, elementwise (both int64 on the device)."""
    return lookup(table, keys)[1]


def image_indices(image_id, n, img_ids, img_index, dev, what):
    """The image of n detections - one id for all, or a tensor [n] of ids - as int64 [n] positions in the sorted `img_ids` on the device
    (`img_index`: id -> position); -1 for an image the ground truth does not know."""
    if torch.is_tensor(image_id) and image_id.dim() > 0:
        ids = image_id.to(dev).to(torch.int64).reshape(-1)
        if ids.shape[0] != n:
            raise ValueError(f"{what}: one image id per detection, or one for all")
        i, found = lookup(torch.tensor(img_ids, dtype=torch.int64, device=dev), ids)
        return torch.where(found, i, torch.full_like(i, -1))
    i = img_index.get(image_id.item() if torch.is_tensor(image_id) else image_id, -1)
    return torch.full((n,), i, dtype=torch.int64, device=dev)


def rank_in_run(sorted_keys):
    """Position of each element within its run of equal keys, int64.  The keys are sorted, so a key's first position is its run's start;
    exact on integers and no host read."""
    return torch.arange(int(sorted_keys.shape[0]), device=sorted_keys.device) - torch.searchsorted(sorted_keys, sorted_keys)


def score_then_key_order(score, key):
    """The order that sorts by key and, within a key, by descending score; both sorts stable, so ties stay in input order."""
    o1 = torch.sort(-score, stable=True).indices
    return o1[torch.sort(key[o1], stable=True).indices]


def zero_rank(n, dev):
    """`dt_rank` of n slots without a per-group cut: nothing ranks past NO_CUT."""
    return torch.zeros(n, dtype=torch.int32, device=dev)


def category_order(cat_dt_offsets, dt_score):
    """Per category its detection slots in descending score order (stable over the image order the slots are in): coco_accumulate's `order`."""
    cat_of = torch.searchsorted(cat_dt_offsets, torch.arange(int(dt_score.shape[0]), device=dt_score.device), right=True) - 1
    return score_then_key_order(dt_score, cat_of).contiguous()


def masked_mean(s):
    """pycocotools' mean(s[s > -1]): the mean of the valid cells, -1 where none is valid."""
    s = s[s > -1]
    return np.float64(-1) if s.size == 0 else np.mean(s)


# ---- the run-length operands of coco_iou (`segm`)
def image_sizes(sizes, img, num_images, what, name):
    """Per-image [h, w] of one side's masks ([0, 0]: none): sizes [n, 2] and image indices [n] on the host; masks of one image must agree."""
    out = np.zeros((num_images, 2), np.int32)
    sizes, img = np.asarray(sizes, np.int32).reshape(-1, 2), np.asarray(img, np.int64).reshape(-1)
    out[img] = sizes                                           # one of an image's sizes; it is every mask's unless they differ
    if (out[img] != sizes).any():
        raise ValueError(f"{name}: the {what} masks of one image differ in size")
    return out


def rle_operands(ev, masks, gt, src, img):
    """coco_iou's run-length mode for an evaluator whose _layout() has run: `masks` = the detections' (counts, runs, area, box, sizes) as
    the mask store gives them, `gt` the ground truth with counts / runs / sizes, `src` the positions (device int64) of the detections
    that count for the per-image sizes and `img` every detection's image index -> the `rle` dict of ops.coco_iou."""
    I = len(ev.img_ids)
    counts, runs, _area, _box, sizes = masks
    host_keys = ev.group_keys.cpu().numpy() % max(I, 1)       # the groups' image indices
    dt_img = image_sizes(sizes[src.cpu().numpy()], img[src].cpu().numpy(), I, "detection", ev.name)
    gt_img = image_sizes(gt["sizes"], gt["key"] % max(I, 1), I, "ground-truth", ev.name)
    has = lambda off: (off[1:] > off[:-1]).cpu().numpy()[:, None]
    return {"dt": (counts, runs, ev.dt_index.contiguous()), "gt": (gt["counts"], gt["runs"], None),
            "dt_sizes": dt_img[host_keys] * has(ev.dt_offsets), "gt_sizes": gt_img[host_keys] * has(ev.gt_offsets)}


# ---- bootstrap replicates (csrc/bootstrap_kernels.hip)
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
    """The replicate cells of an evaluated GroupedEval, a chunk of replicates at a time: yields (ap_sum, recall), float64
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
    """masked_mean of each replicate, regrouped: cells [B, ...] (-1: not valid) -> sum of the valid cells / (per_cell * their number), -1
    where none is valid; float64 [B] on the device.  `per_cell`: 101 for ap_sum (a cell is a sum of 101 values), 1 for recall."""
    v = cells.reshape(cells.shape[0], -1)
    valid = v > -1
    n = valid.sum(1)
    total = _row_sums(torch.where(valid, v, torch.zeros_like(v)))
    return torch.where(n > 0, total / (per_cell * n.clamp(min=1)).to(torch.float64), torch.full_like(total, -1.0))


def run_bootstrap(ev, weights, max_dets, stat_rows, num_stats, cell_budget_bytes, return_cells, what):
    """GroupedEval.bootstrap(): `stat_rows(ap_sum, recall)` -> the `num_stats` statistics of a chunk as a list of [chunk] tensors."""
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


class DetectionStore:
    """The detections of one result set as they were added: per detection its image index (-1: an image the ground truth does not know),
    category id, score and, `with_boxes`, box [x, y, w, h].  `with_masks`: every detection has a mask that its owner keeps; add() only
    checks their number.  `img_ids` / `img_index`: the ground truth's sorted image ids and id -> position."""

    def __init__(self, device, img_ids, img_index, with_boxes=True, with_masks=False):
        self.device, self.img_ids, self.img_index, self.with_boxes, self.with_masks = device, img_ids, img_index, with_boxes, with_masks
        self._img, self._cat, self._score, self._box = [], [], [], []
        self.num_added = 0

    def add(self, what, image_id, category_ids, scores, boxes=None, masks=None):
        """Detections of one image (or, with image_id a tensor [n], of many) as tensors, which stay on the device; float32 is widened
        exactly.  `what` names the caller in the messages."""
        dev = self.device
        cat = torch.as_tensor(category_ids, device=dev).to(torch.int64).reshape(-1)
        n = int(cat.shape[0])
        score = torch.as_tensor(scores, device=dev).to(torch.float64).reshape(-1)
        if score.shape[0] != n:
            raise ValueError(f"{what}: one score per detection")
        if self.with_boxes:
            if boxes is None:
                raise ValueError(f"{what}: bbox evaluation needs boxes")
            box = torch.as_tensor(boxes, device=dev).to(torch.float64).reshape(-1, 4)
            if box.shape[0] != n:
                raise ValueError(f"{what}: one box per detection")
        if self.with_masks:
            if masks is None:
                raise ValueError(f"{what}: segm evaluation needs masks")
            if len(masks) != n:
                raise ValueError(f"{what}: one mask per detection")
        self._img.append(image_indices(image_id, n, self.img_ids, self.img_index, dev, what))
        self._cat.append(cat)
        self._score.append(score)
        if self.with_boxes:
            self._box.append(box)
        self.num_added += n

    def add_results(self, results):
        """COCO / LVIS result dicts (`image_id`, `category_id`, `score` and, `with_boxes`, `bbox`)."""
        if not results:
            return
        dev = self.device
        if self.with_boxes:
            self._box.append(torch.tensor([r["bbox"] for r in results], dtype=torch.float64, device=dev).reshape(-1, 4))
        self._img.append(torch.tensor([self.img_index.get(r["image_id"], -1) for r in results], dtype=torch.int64, device=dev))
        self._cat.append(torch.tensor([r["category_id"] for r in results], dtype=torch.int64, device=dev))
        self._score.append(torch.tensor([r["score"] for r in results], dtype=torch.float64, device=dev))
        self.num_added += len(results)

    def tensors(self):
        """-> image index int64 [n], category id int64 [n], score float64 [n], box float64 [n, 4] (None without boxes), in the order added."""
        cat = lambda xs, dt, shape: torch.cat(xs) if xs else torch.zeros(shape, dtype=dt, device=self.device)
        return (cat(self._img, torch.int64, (0,)), cat(self._cat, torch.int64, (0,)), cat(self._score, torch.float64, (0,)),
                cat(self._box, torch.float64, (0, 4)) if self.with_boxes else None)


class GroupedEval:
    """What COCOEval and LVISEval share: the ground truth sorted into the slot layout once, the detections, the tail of the front end, and
    the accumulate and bootstrap passes.  A subclass sets `kind` ("coco" / "lvis"), `flag_field` (the annotation field `gt_flag` is read
    from), `stat_names` and `cuts` (the maxDets list of its accumulate pass) and supplies
        _group()            its cut and filter, ending in _layout(); -> the size of the ragged IoU buffer
        _match(iou_size)    the IoU pass and its match entry
        _stat_rows(ap_sum, recall)      its statistics of a chunk of bootstrap replicates, a list of [chunk] tensors
        accumulate(), summarize() and printing."""
    kind = flag_field = stat_names = None

    def __init__(self, gt, iou_type, device, max_dets):
        self.iou_type = iou_type
        self.dataset = load_dataset(gt)
        self.device = torch.device("cuda:0" if device is None else device)
        self.img_ids = sorted(set(im["id"] for im in self.dataset["images"]))
        self.cat_ids = sorted(c["id"] for c in self.dataset["categories"])
        self._img_index = {v: i for i, v in enumerate(self.img_ids)}
        self._cat_index = {v: i for i, v in enumerate(self.cat_ids)}
        self.iou_thrs, self.rec_thrs, self.max_dets, self.area_rng = IOU_THRS, REC_THRS, max_dets, np.asarray(AREA_RNG, np.float64)
        self._anns = [(j, a) for j, a in enumerate(self.dataset.get("annotations", []))
                      if a["image_id"] in self._img_index and a["category_id"] in self._cat_index]
        self._gt = self._dev_params = None
        self.reset()

    @property
    def name(self):
        return type(self).__name__

    def reset(self):
        """Forget the detections (the ground truth stays)."""
        self._dets = DetectionStore(self.device, self.img_ids, self._img_index, self.iou_type == "bbox", self.on_masks)
        self.precision = self.recall = self.iou = self.precision_pool = None

    num_added = property(lambda self: self._dets.num_added)
    on_masks = property(lambda self: self.iou_type in MASK_TYPES)

    # ---- detections
    def add(self, image_id, category_ids, scores, boxes=None):
        """The detections of one image (or, with image_id a tensor [n], of many): category_ids [n], scores [n], boxes [n, 4] as [x, y, w, h].
        Tensors stay on the device; float32 is widened exactly."""
        self._dets.add(f"{self.name}.add", image_id, category_ids, scores, boxes)

    def add_results(self, results):
        """Result dicts (`image_id`, `category_id`, `score`, `bbox`), e.g. the rows of to_coco_results."""
        self._dets.add_results(results)

    # ---- ground truth, sorted category-major once
    def _build_ground_truth(self):
        dev, anns = self.device, self._anns
        key, order = sort_ground_truth(anns, self._cat_index, self._img_index, len(self.img_ids))
        gt = {"key": key, "order": order, "index": np.asarray([anns[o][0] for o in order], np.int64),
              "area": np.asarray([float(anns[o][1]["area"]) for o in order], np.float64),
              "flag": np.asarray([1 if anns[o][1].get(self.flag_field, 0) else 0 for o in order], np.uint8)}
        # coco_iou's crowd array: only the iscrowd flag switches a pair to the crowd union
        gt["crowd"] = gt["flag"] if self.flag_field == "iscrowd" else np.zeros_like(gt["flag"])
        if self.iou_type == "bbox":
            gt["box"] = torch.from_numpy(np.asarray([anns[o][1]["bbox"] for o in order], np.float64).reshape(-1, 4)).to(dev)
        for k in ("key", "area", "flag", "crowd"):
            gt[k + "_dev"] = torch.from_numpy(gt[k]).to(dev)
        return gt

    def _ground_truth(self):
        if self._gt is None:
            self._gt = self._build_ground_truth()
        return self._gt

    def _params(self):
        """iou_thrs, area_rng and rec_thrs as float64 on the device, uploaded once per evaluator."""
        if self._dev_params is None:
            self._dev_params = tuple(torch.from_numpy(np.ascontiguousarray(v, np.float64)).to(self.device)
                                     for v in (self.iou_thrs, self.area_rng, self.rec_thrs))
        return self._dev_params

    def _layout(self, key, dt_index, score, box, area=None, rank=None):
        """The tail of the front end.  `key`: the kept detections' group keys, sorted, each group in score order; `dt_index`: their positions
        in the order added; `score`, `box`, `area` (None: w * h of the box): per added detection; `rank`: per kept detection (None: no
        per-group cut).  Sets every slot attribute of the module docstring but the match arrays; -> the size of the ragged IoU buffer."""
        dev, I, K = self.device, len(self.img_ids), len(self.cat_ids)
        gt = self._ground_truth()
        num_dt = int(key.shape[0])
        self.dt_index, self.dt_rank = dt_index, zero_rank(num_dt, dev) if rank is None else rank
        self.dt_score = score[dt_index].contiguous()
        self.dt_image, self.gt_image = (key % max(I, 1)).to(torch.int32), (gt["key_dev"] % max(I, 1)).to(torch.int32)       # bootstrap() weighs by them
        # the groups: every (category, image) with a detection or a ground truth
        keys = torch.unique(torch.cat([key, gt["key_dev"]]))
        dc, self.dt_offsets = group_offsets(keys, key)
        gc, self.gt_offsets = group_offsets(keys, gt["key_dev"])
        self.iou_offsets = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(dc * gc, 0)])
        iou_size = int(self.iou_offsets[-1])                      # the one host read: it sizes the IoU buffer
        self.group_keys, self.gt_index = keys, gt["index"]
        cat_edges = torch.arange(K + 1, device=dev) * I
        self.cat_dt_offsets = torch.searchsorted(key, cat_edges).contiguous()
        self.cat_gt_offsets = torch.searchsorted(gt["key_dev"], cat_edges).contiguous()
        self.dt_boxes = box[dt_index].contiguous()
        self.dt_area = ((self.dt_boxes[:, 2] * self.dt_boxes[:, 3]) if area is None else area[dt_index]).contiguous()
        self.gt_boxes, self.gt_area, self.gt_flag, self.gt_crowd = gt["box"], gt["area_dev"], gt["flag_dev"], gt["crowd_dev"]
        self.num_dt, self.num_gt, self.num_groups = num_dt, int(gt["key"].shape[0]), int(keys.shape[0])
        return iou_size

    def _set_rle(self, masks, gt, src, img):
        """After _layout(), for an evaluation over masks: coco_iou's run-length operands (rle_operands) and, for `boundary`, the same
        operands over the boundaries of the same slots with the boundaries' tight boxes.  The detections' boundaries are made here, once
        per evaluate(); the ground truth's were made with the ground truth."""
        self._rle, self._boundary = rle_operands(self, masks, gt, src, img), None
        if self.iou_type == "boundary":
            counts, runs, _area, box, _sizes = self._masks.boundaries(self.dilation_ratio)
            g = gt["boundary"]
            self._boundary = {"rle": dict(self._rle, dt=(counts, runs, self.dt_index.contiguous()), gt=(g[0], g[1], None)),
                              "dt_boxes": box[self.dt_index].contiguous(), "gt_boxes": g[3]}

    def _iou(self, iou_size):
        """The ragged IoU buffer: coco_iou on boxes or masks; for `boundary` the element-wise minimum (float64) of the mask IoU and the
        IoU of the boundaries, both with the same crowd flags."""
        iou = ops.coco_iou(self.dt_offsets, self.gt_offsets, self.iou_offsets, iou_size, self.dt_boxes, self.gt_boxes, self.gt_crowd, self._rle)
        if self.iou_type == "boundary":
            b = self._boundary
            iou = torch.minimum(iou, ops.coco_iou(self.dt_offsets, self.gt_offsets, self.iou_offsets, iou_size, b["dt_boxes"], b["gt_boxes"],
                                                  self.gt_crowd, b["rle"]))
        return iou

    def evaluate(self):
        """Group, IoU, match: leaves the slot layout and the match arrays of the module docstring on the device."""
        self._match(self._group())
        return self

    def _accumulate(self):
        """-> precision [T, R, K, A, M], recall [T, K, A, M], scores [T, R, K, A, M] on the device, M = len(cuts)."""
        if self.iou is None:
            raise RuntimeError(f"{self.name}.accumulate: call evaluate() first")
        self.order = category_order(self.cat_dt_offsets, self.dt_score)
        return ops.coco_accumulate(self.cat_dt_offsets, self.cat_gt_offsets, self.order, self.dt_rank, self.dt_score, self.dt_match,
                                   self.dt_ignore, self.gt_ignore, self.cuts, self._params()[2])

    # ---- AP-pool (csrc/pooled_kernels.hip; include/mi355det.h, "Pooled precision-recall")
    area_labels = ("all", "small", "medium", "large")

    def default_pools(self):
        """[(name, category indices)]: the pools accumulate_pooled() draws without arguments; a name is the suffix of the pool's key."""
        return [("", list(range(len(self.cat_ids))))]

    def pool_lists(self, pools):
        """The operands of ops.pooled_accumulate for `pools` (lists of category indices): pool_order int64 [P], pool_offsets int64 [S + 1]
        and pool_npig int64 [S, A] on the device.  A pool's list: the slots of its categories with dt_rank below the largest cut, in
        descending score, stable over the slot index (torch masks and sorts: plumbing)."""
        dev, K = self.device, len(self.cat_ids)
        cat_of_dt = torch.searchsorted(self.cat_dt_offsets, torch.arange(self.num_dt, device=dev), right=True) - 1
        cat_of_gt = torch.searchsorted(self.cat_gt_offsets, torch.arange(self.num_gt, device=dev), right=True) - 1
        kept = self.dt_rank < max(self.cuts)
        by_score = torch.sort(-self.dt_score, stable=True).indices            # one sort serves every pool: a subsequence of it stays sorted
        orders, npig = [], []
        for cats in pools:
            cats = np.asarray(cats, np.int64).reshape(-1)
            if cats.size and (cats.min() < 0 or cats.max() >= K):
                raise ValueError(f"{self.name}.accumulate_pooled: a pool holds category indices 0..{K - 1}")
            inside = torch.zeros(K + 1, dtype=torch.bool, device=dev)
            inside[torch.from_numpy(cats).to(dev)] = True
            orders.append(by_score[(inside[cat_of_dt] & kept)[by_score]])
            npig.append(((self.gt_ignore == 0) & inside[cat_of_gt][None, :]).sum(1))
        host_offsets = np.cumsum([0] + [int(o.shape[0]) for o in orders]).astype(np.int64)       # the masks above sized the lists on the host
        return torch.cat(orders).contiguous(), torch.from_numpy(host_offsets).to(dev), torch.stack(npig).contiguous(), host_offsets

    def accumulate_pooled(self, pools=None):
        """AP-pool: one precision-recall curve per pool of categories, every category's detections ranked in one list.  `pools`: lists of
        category indices (None: default_pools()).  Sets precision_pool and scores_pool [T, R, S, A] and recall_pool [T, S, A], float64 numpy.
        Needs evaluate() only, and leaves precision, recall and the results of accumulate() as they are."""
        if self.iou is None:
            raise RuntimeError(f"{self.name}.accumulate_pooled: call evaluate() first")
        named = self.default_pools() if pools is None else [(f"[{j}]", p) for j, p in enumerate(pools)]
        if not named:
            raise ValueError(f"{self.name}.accumulate_pooled: no pools")
        self.pool_names = [n for n, _p in named]
        order, offsets, npig, host_offsets = self.pool_lists([p for _n, p in named])
        p, r, s = ops.pooled_accumulate(order, offsets, npig, self.dt_score, self.dt_match, self.dt_ignore, self._params()[2], host_offsets)
        self.precision_pool, self.recall_pool, self.scores_pool = p.cpu().numpy(), r.cpu().numpy(), s.cpu().numpy()
        return self

    def summarize_pooled(self):
        """-> an ordered dict: APpool, APpool50, APpool75, one APpool<s|m|l> per area range after the first and ARpool over the first pool,
        then APpool<name> for every further pool; each the masked_mean of its cells."""
        from collections import OrderedDict
        if getattr(self, "precision_pool", None) is None:
            raise RuntimeError(f"{self.name}.summarize_pooled: call accumulate_pooled() first")
        pr, rc = self.precision_pool, self.recall_pool
        at = lambda thr: np.isclose(self.iou_thrs, thr)
        res = OrderedDict()
        res["APpool"], res["APpool50"], res["APpool75"] = masked_mean(pr[:, :, 0, 0]), masked_mean(pr[at(.5)][:, :, 0, 0]), masked_mean(pr[at(.75)][:, :, 0, 0])
        for a in range(1, pr.shape[3]):
            res["APpool" + self.area_labels[a][0]] = masked_mean(pr[:, :, 0, a])
        for s in range(1, pr.shape[2]):
            res["APpool" + self.pool_names[s]] = masked_mean(pr[:, :, s, 0])
        res["ARpool"] = masked_mean(rc[:, 0, 0])
        self.results_pool = res
        return res

    def print_pooled(self, file=None):
        """One line per key of summarize_pooled()."""
        import sys
        for key, value in self.summarize_pooled().items():
            print(f" {key:<10} = {value:0.3f}", file=sys.stdout if file is None else file)

    def bootstrap(self, weights, return_cells=False, cell_budget_bytes=1 << 30):
        """The statistics of resampled data sets, float64 numpy [B, len(stat_names)].  `weights`: integers [B, len(img_ids)] (numpy or tensor,
        e.g. compare.bootstrap_weights); replicate b is the evaluation of the data set in which image i occurs weights[b, i] times
        (include/mi355det.h, "Bootstrap replicates").  Needs evaluate() only; the match arrays are read, and the accumulated results stay as
        they are.  The replicates go through mi355det_coco_bootstrap in chunks whose two cell buffers stay within `cell_budget_bytes`; a
        replicate's cells and statistics are the same bits whatever the chunking.
        return_cells=True: -> (stats, (ap_sum, recall)), the cells float64 [B, 10, K, 4, len(cuts)] on the device: ap_sum = the sum of a
        cell's 101 precision values, so the AP of category k alone is a mean over ap_sum[:, :, k] / 101; -1 marks a cell without ground
        truth."""
        return run_bootstrap(self, weights, self.cuts, self._stat_rows, len(self.stat_names), cell_budget_bytes, return_cells,
                             f"{self.name}.bootstrap")
