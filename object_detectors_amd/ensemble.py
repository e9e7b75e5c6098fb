"""Weighted boxes fusion on the device: two or more result sets - or several passes of one model - merged into one (Solovyev, Wang,
Gabruseva 2021).  The rule is stated in include/mi355det.h, "Weighted boxes fusion", from the paper and from memory of the authors' package
`ensemble-boxes`, which this module was NOT run against; three deviations are deliberate: a candidate whose weighted score is not positive
is dropped, the fusion order is a stable sort (ties by model, then by the order added), and of the package's conf_types only avg and max
exist.

    f = WeightedBoxesFusion(gt_or_image_ids, weights=[2, 1])
    f.add(model, image_id, category_ids, scores, boxes) / f.add_results(model, results)
    f.run()                   torch filters and sorts (plumbing) -> mi355det_wbf_fuse (csrc/fusion_kernels.hip), one wavefront per
                              (image, category) group -> the founders compacted and put in output order; one host read
    f.to_results()            COCO result dicts
    f.feed(evaluator)         the fused detections into a COCOEval / LVISEval, as device tensors, in one add()

Boxes are [x, y, w, h] in image coordinates; un-flipping and rescaling the boxes of a test-time augmentation is the caller's job.  One model
(M = 1) is allowed: it merges that model's overlapping detections; passes that deserve weights of their own are added as separate models."""
import os

import numpy as np
import torch

from . import ops
from .cocoeval import STAT_NAMES, COCOEval
from .evalcore import DetectionStore, load_dataset, score_then_key_order
from .lviseval import RESULT_KEYS, LVISEval

DROP_REASONS = ("unknown_image", "below_skip_box_thr", "score_not_positive", "box_not_finite", "box_empty")


def _image_ids(images):
    """A ground truth as evalcore.load_dataset takes it, or a list / array / tensor of image ids -> the sorted ids."""
    if torch.is_tensor(images):
        images = images.cpu().tolist()
    if isinstance(images, (list, tuple, set, frozenset, range, np.ndarray)):
        return sorted(set(int(i) for i in images))
    return sorted(set(im["id"] for im in load_dataset(images)["images"]))


class WeightedBoxesFusion:
    """`images`: the ground truth (only its image list is read) or the image ids; a detection on another image is dropped.  `weights`: one
    positive number per model, which fixes the number of models; None: every model weighs 1 and there are as many models as were added
    to (at least one).  iou_thr in [0, 1), skip_box_thr and conf_type ("avg" / "max") as in the rule."""

    def __init__(self, images, weights=None, iou_thr=0.55, skip_box_thr=0.0, conf_type="avg", device=None):
        if weights is not None:
            weights = [float(w) for w in np.asarray(weights, np.float64).reshape(-1)]
            if not weights:
                raise ValueError("WeightedBoxesFusion: at least one model, so at least one weight")
            if not all(np.isfinite(w) and w > 0 for w in weights):
                raise ValueError("WeightedBoxesFusion: every weight must be positive and finite")
        if not 0 <= float(iou_thr) < 1:
            raise ValueError("WeightedBoxesFusion: iou_thr must lie in [0, 1)")
        if np.isnan(float(skip_box_thr)):
            raise ValueError("WeightedBoxesFusion: skip_box_thr must be a number")
        if conf_type not in ops.WBF_CONF_TYPES:
            raise ValueError(f"WeightedBoxesFusion: conf_type must be one of {sorted(ops.WBF_CONF_TYPES)}, not {conf_type!r}")
        self._given, self.iou_thr, self.skip_box_thr, self.conf_type = weights, float(iou_thr), float(skip_box_thr), conf_type
        self.device = torch.device("cuda:0" if device is None else device)
        self.img_ids = _image_ids(images)
        self._img_index = {v: i for i, v in enumerate(self.img_ids)}
        self._ids_dev = None
        self.reset()

    weights = property(lambda self: [1.0] * len(self._det) if self._given is None else self._given)
    weight_sum = property(lambda self: float(np.cumsum(np.asarray(self.weights, np.float64))[-1]))     # w_0 + w_1 + .. in that order
    weight_max = property(lambda self: max(self.weights))
    num_models = property(lambda self: len(self._det))
    num_added = property(lambda self: [side.num_added for side in self._det])

    def _store(self):
        return DetectionStore(self.device, self.img_ids, self._img_index)

    def reset(self):
        """Forget the detections of every model."""
        self._det = [self._store() for _ in (self._given or [1.0])]
        self.result = None

    # ---- detections
    def _side(self, model):
        if isinstance(model, bool) or not isinstance(model, (int, np.integer)) or model < 0 or (self._given is not None and model >= len(self._given)):
            raise ValueError(f"WeightedBoxesFusion: model must be an index in 0 .. {len(self._det) - 1} (one weight per model), not {model!r}")
        while len(self._det) <= model:                             # without weights the models are counted as they come
            self._det.append(self._store())
        return self._det[int(model)]

    def add(self, model, image_id, category_ids, scores, boxes):
        """The detections of `model` on one image (or, with image_id a tensor [n], on many): category_ids [n], scores [n], boxes [n, 4] as
        [x, y, w, h].  Tensors stay on the device; float32 is widened exactly."""
        self._side(model).add("WeightedBoxesFusion.add", image_id, category_ids, scores, boxes)
        self.result = None

    def add_results(self, model, results):
        """COCO result dicts (`image_id`, `category_id`, `score`, `bbox`) of `model`, e.g. a loaded results json."""
        self._side(model).add_results(results)
        self.result = None

    # ---- the three parts of run()
    def _front(self):
        """Filter, weigh, sort -> the kernel's operands and what the tail needs, or None when nothing was added.  No host read: a dropped
        detection is not removed but sorted behind the last group, where no group owns it."""
        dev, I = self.device, len(self.img_ids)
        n = sum(self.num_added)
        if n == 0:
            return None
        sides = [side.tensors() for side in self._det]
        img, cat, score, box = (torch.cat([s[k] for s in sides]) for k in range(4))                    # model-major
        weight = torch.cat([torch.full((int(s[0].shape[0]),), w, dtype=torch.float64, device=dev) for s, w in zip(sides, self.weights)])
        weighted = score * weight
        corners = torch.stack([box[:, 0], box[:, 1], box[:, 0] + box[:, 2], box[:, 1] + box[:, 3]], 1)
        reasons = [img < 0, score < self.skip_box_thr, ~(torch.isfinite(weighted) & (weighted > 0)),
                   ~(torch.isfinite(box).all(1) & torch.isfinite(corners).all(1)), (box[:, 2] <= 0) | (box[:, 3] <= 0)]
        keep = torch.ones(n, dtype=torch.bool, device=dev)
        dropped = []
        for r in reasons:                                                                              # the first reason that holds counts
            dropped.append((keep & r).sum())
            keep &= ~r
        # fusion order: image, then category, then descending weighted score, then the model-major order (three stable sorts)
        order = torch.sort(-torch.where(keep, weighted, torch.zeros_like(weighted)), stable=True).indices
        order = order[torch.sort(cat[order], stable=True).indices]
        key_img = torch.where(keep, img, torch.full_like(img, I))
        order = order[torch.sort(key_img[order], stable=True).indices]
        ki, kc = key_img[order], cat[order]
        first = torch.ones(n, dtype=torch.bool, device=dev)
        first[1:] = (ki[1:] != ki[:-1]) | (kc[1:] != kc[:-1])
        # group j = the j-th run of one (image, category); there are at most n, the ones past the last are empty, the dropped belong to none
        group = torch.where(ki < I, torch.cumsum(first, 0) - 1, torch.full_like(ki, n))
        offsets = torch.searchsorted(group, torch.arange(n + 1, device=dev)).contiguous()
        return {"n": n, "order": order, "offsets": offsets, "boxes": corners[order].contiguous(), "scores": weighted[order].contiguous(),
                "image": ki, "category": kc, "dropped": torch.stack(dropped)}

    def _ids_on_device(self):
        """`img_ids` as an int64 tensor on the device, uploaded once."""
        if self._ids_dev is None:
            self._ids_dev = torch.tensor(self.img_ids, dtype=torch.int64, device=self.device)
        return self._ids_dev

    def _kernel(self, fr):
        return ops.wbf_fuse(fr["offsets"], fr["boxes"], fr["scores"], self.iou_thr, self.conf_type, self.weight_sum, self.weight_max)

    def _finish(self, fr, out):
        """Compact the founders, apply the output order, number the clusters: the one host read is the founder count with the dropped counts."""
        dev, n = self.device, fr["n"]
        leader, fused, score, members, _sums = out
        founder = leader == torch.arange(n, device=dev)
        host = torch.cat([founder.sum().reshape(1), fr["dropped"]]).cpu().tolist()                     # the one host read
        slots = torch.nonzero_static(founder, size=int(host[0])).reshape(-1)                           # fusion order: image, category, creation
        slots = slots[score_then_key_order(score[slots], fr["image"][slots])]                          # image-major, descending score, stable
        position = torch.full((n,), -1, dtype=torch.int64, device=dev)                                 # founder slot -> output position
        position[slots] = torch.arange(int(slots.shape[0]), device=dev)
        # no boolean-mask indexing here: it would size its result with a host read of its own
        cluster_of = torch.empty(n, dtype=torch.int64, device=dev)
        cluster_of[fr["order"]] = torch.where(leader >= 0, position[leader.clamp(min=0)], torch.full_like(leader, -1))
        f = fused[slots]
        image_index = fr["image"][slots]
        return {"image_index": image_index, "image_id": self._ids_on_device()[image_index],
                "category_id": fr["category"][slots], "score": score[slots],
                "box": torch.stack([f[:, 0], f[:, 1], f[:, 2] - f[:, 0], f[:, 3] - f[:, 1]], 1), "members": members[slots],
                "cluster_of": cluster_of, "dropped": dict(zip(DROP_REASONS, (int(v) for v in host[1:])))}

    def _empty(self):
        dev = self.device
        z = lambda dt, *shape: torch.zeros(shape or (0,), dtype=dt, device=dev)
        return {"image_index": z(torch.int64), "image_id": z(torch.int64), "category_id": z(torch.int64), "score": z(torch.float64),
                "box": z(torch.float64, 0, 4), "members": z(torch.int32), "cluster_of": z(torch.int64), "dropped": dict.fromkeys(DROP_REASONS, 0)}

    def run(self):
        """-> {"image_index", "image_id", "category_id" int64 [K], "score" float64 [K], "box" float64 [K, 4] as [x, y, w, h], "members" int32
        [K]} on the device, one row per fused detection, image-major and within an image in descending score order (ties: ascending category
        id, then the order the clusters were made); "cluster_of" int64 [detections added, model-major]: the row each detection was fused into,
        -1 for a dropped one; "dropped": {reason: count} (ints).  May be called again; the same bits come out."""
        fr = self._front()
        self.result = self._empty() if fr is None else self._finish(fr, self._kernel(fr))
        return self.result

    # ---- the fused detections
    def _result(self):
        return self.run() if self.result is None else self.result

    def to_results(self):
        """The fused detections as COCO result dicts: `image_id`, `category_id`, `score`, `bbox`."""
        r = self._result()
        ids, cats, scores, boxes = (r[k].cpu().tolist() for k in ("image_id", "category_id", "score", "box"))
        return [{"image_id": i, "category_id": c, "score": s, "bbox": b} for i, c, s, b in zip(ids, cats, scores, boxes)]

    def feed(self, evaluator):
        """The fused detections into `evaluator` (COCOEval, LVISEval: anything whose add() takes image ids, category ids, scores and boxes
        as tensors) in one call; an LVISEval then applies its own 300-per-image cut.  -> the evaluator."""
        r = self._result()
        evaluator.add(r["image_id"], r["category_id"], r["score"], r["box"])
        return evaluator


def fuse_results(result_lists, images, **kw):
    """The one-call form: a list of COCO result lists (one per model) and the images -> the fused COCO result dicts.  Keywords as
    WeightedBoxesFusion takes them."""
    f = WeightedBoxesFusion(images, **kw)
    if kw.get("weights") is not None and f.num_models != len(result_lists):
        raise ValueError(f"fuse_results: {f.num_models} weights for {len(result_lists)} result lists: one weight per model")
    for m, rows in enumerate(result_lists):
        f.add_results(m, rows)
    return f.to_results()


def evaluate_with_fusion(gt, result_lists, names, lvis=False, device=None, **kw):
    """The statistics of every result list and of their fusion over one ground truth -> (statistic names, {name: float64 array}, the
    WeightedBoxesFusion after run()).  COCO: the twelve numbers of COCOEval.summarize; `lvis`: the thirteen of LVISEval.  The fused
    detections go into their evaluator as device tensors (feed).  Keywords as WeightedBoxesFusion takes them."""
    dataset = load_dataset(gt)
    fusion = WeightedBoxesFusion(dataset, device=device, **kw)
    for m, rows in enumerate(result_lists):
        fusion.add_results(m, rows)
    fusion.run()

    def stats(fill):
        if lvis:
            ev = LVISEval(dataset, device=device)
            fill(ev)
            return np.asarray(list(ev.run().get_results().values()), np.float64)
        ev = COCOEval(dataset, "bbox", device=device)
        fill(ev)
        with open(os.devnull, "w") as quiet:
            return ev.evaluate().accumulate().summarize(file=quiet)
    table = {name: stats(lambda ev, rows=rows: ev.add_results(rows)) for name, rows in zip(names, result_lists)}
    table["fusion"] = stats(fusion.feed)
    return list(RESULT_KEYS if lvis else STAT_NAMES), table, fusion


def print_stats_table(stat_names, table, file=None):
    """One line per statistic, one column per entry of `table` ({name: values}, in its order)."""
    names = list(table)
    width = [max(8, len(n)) for n in names]
    print(" " * 8 + " ".join(f"{n:>{w}s}" for n, w in zip(names, width)), file=file)
    for k, stat in enumerate(stat_names):
        print(f"{stat:>8s} " + " ".join(f"{table[n][k]:{w}.4f}" for n, w in zip(names, width)), file=file)
