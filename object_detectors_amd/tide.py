"""Error breakdown of AP50 on the device: why an evaluated COCOEval / LVISEval (`bbox`) loses AP, after TIDE (Bolya et al., ECCV 2020).

Every false positive at IoU 0.5 is one of five kinds - Cls (right place, wrong label), Loc (right label, loose box), Both, Dupe (a second
detection of a ground truth that is taken) or Bkg - the ground truths no Loc or Cls detection explains are Miss, and each kind is priced by
the AP50 gained when that kind alone is fixed.  The rules are spelled out in include/mi355det.h, "Error breakdown"; they are close to tidecv's
order of tests, not a port of it.

    ErrorBreakdown(ev)      ev: a COCOEval or LVISEval after evaluate(); only its public slot attributes (evalcore.py) are read
    .run(fg=0.5, bg=0.1)    torch sorts build the image-major view of the category-major slots (plumbing) -> tide_classify -> tide_fixes ->
                            coco_accumulate twice (seven fixes as eight "area ranges", then the Cls fix with its detections moved) -> dict
    .report(file=None)      the table

What the evaluator never computes is the overlap of a detection with the ground truth of the other categories of its image; that is the hot
part (csrc/tide_kernels.hip).  The eight deltas do not add up to 1 - AP50: each fix is priced alone."""
import sys

import numpy as np
import torch

from . import ops
from .evalcore import NO_CUT, category_order, masked_mean, zero_rank

KINDS = ("Cls", "Loc", "Both", "Dupe", "Bkg", "Miss")            # kind codes 1..5 on the detections; Miss lives on the ground truths
FIXES = KINDS + ("FP", "FN")
_ROW_OF_FIX = {"Loc": 1, "Both": 2, "Dupe": 3, "Bkg": 4, "Miss": 5, "FP": 6, "FN": 7}     # rows of tide_fixes' arrays; row 0 is the base state


def _ap(p, cats=None):
    """precision [R, K] of one state -> the mean of the valid cells the way the evaluators' summarize() takes it (-1: no category counts)."""
    return masked_mean(p if cats is None else p[:, np.asarray(cats, np.int64)])


def _delta(fixed, base):
    return np.float64(np.nan) if (fixed == -1 or base == -1) else fixed - base


class ErrorBreakdown:
    """The error breakdown of one evaluated COCOEval / LVISEval.  After run(): .kind uint8 [num_dt] (0: not a false positive, 1..5 = Cls,
    Loc, Both, Dupe, Bkg), .partner int64 [num_dt] (ground-truth slot or -1), .best_same / .best_other float64 [num_dt], .missed uint8
    [num_gt] on the device in the evaluator's slot layout, and .result, the dict run() returned."""

    def __init__(self, ev):
        if getattr(ev, "iou_type", None) != "bbox":
            raise NotImplementedError(f"ErrorBreakdown: iou_type {getattr(ev, 'iou_type', None)!r}: only bbox is broken down here")
        if getattr(ev, "iou", None) is None:
            raise RuntimeError("ErrorBreakdown: call evaluate() on the evaluator first")
        self.ev = ev
        self.kind = self.partner = self.best_same = self.best_other = self.missed = self.result = None

    def _view(self):
        """The image-major view: each image's detection slots in claim order (descending score, then ascending dt_index), its ground-truth
        slots ascending; three stable sorts, least significant key first."""
        ev, dev, I = self.ev, self.ev.device, len(self.ev.img_ids)
        edges = torch.arange(I + 1, device=dev)
        dt_img = ev.dt_image.to(torch.int64)
        o = torch.sort(ev.dt_index, stable=True).indices
        o = o[torch.sort(-ev.dt_score[o], stable=True).indices]
        o = o[torch.sort(dt_img[o], stable=True).indices].contiguous()
        gt_img = ev.gt_image.to(torch.int64)
        g = torch.sort(gt_img, stable=True).indices.contiguous()
        return (torch.searchsorted(dt_img[o].contiguous(), edges).contiguous(), o, torch.searchsorted(gt_img[g].contiguous(), edges).contiguous(), g)

    def _front_end(self, t):
        """The per-slot inputs of the kernels from the evaluator's arrays at threshold index t: the image-major view, the categories, the
        base match rows and the three flags."""
        ev, dev = self.ev, self.ev.device
        nd, ng = int(ev.num_dt), int(ev.num_gt)
        slot_cat = lambda off, n: (torch.searchsorted(off, torch.arange(n, device=dev), right=True) - 1).to(torch.int32)
        f = {"view": self._view(), "dt_cat": slot_cat(ev.cat_dt_offsets, nd), "gt_cat": slot_cat(ev.cat_gt_offsets, ng),
             "dt_match": ev.dt_match[0, t].contiguous(), "dt_ignore": ev.dt_ignore[0, t].contiguous(), "gt_box": ev.gt_boxes}
        f["dt_fp"] = ((f["dt_match"] == 0) & (f["dt_ignore"] == 0)).to(torch.uint8)
        counted = ev.gt_ignore[0] == 0
        f["gt_free"] = (counted & (ev.gt_match[0, t] == 0)).to(torch.uint8)
        f["gt_counted"] = counted.to(torch.uint8)
        return f

    def _classify(self, f, fg, bg):
        self.kind, self.partner, self.best_same, self.best_other, self.missed = ops.tide_classify(
            f["view"], self.ev.dt_boxes, f["dt_cat"], f["dt_fp"], f["gt_box"], f["gt_cat"], f["gt_counted"], f["gt_free"], fg, bg)

    def _fixes(self, f):
        self.fix_dt_match, self.fix_dt_ignore, self.fix_gt_ignore, self.cls_cat, self.cls_match, self.cls_ignore = ops.tide_fixes(
            f["view"], f["dt_match"], f["dt_ignore"], f["dt_cat"], f["gt_cat"], f["gt_counted"], f["gt_free"], self.kind, self.partner, self.missed)

    def _price_in_place(self, rec):
        """The base state and the seven in-place fixes in one accumulate call, the fix in the place of the area range -> [R, K, 8] on the device."""
        ev = self.ev
        rows, _r, _s = ops.coco_accumulate(ev.cat_dt_offsets, ev.cat_gt_offsets, category_order(ev.cat_dt_offsets, ev.dt_score),
                                           zero_rank(int(ev.num_dt), ev.device), ev.dt_score, self.fix_dt_match, self.fix_dt_ignore, self.fix_gt_ignore, [NO_CUT], rec)
        return rows[0, :, :, :, 0]

    def _price_cls(self, f, rec):
        """The Cls fix: the slots category-major again under their new categories, each group still in claim order -> [R, K] on the device."""
        ev, dev, K, nd = self.ev, self.ev.device, len(self.ev.cat_ids), int(self.ev.num_dt)
        claim = f["view"][1]
        perm = claim[torch.sort(self.cls_cat[claim], stable=True).indices].contiguous()
        cat_off = torch.searchsorted(self.cls_cat[perm].to(torch.int64).contiguous(), torch.arange(K + 1, device=dev)).contiguous()
        score = ev.dt_score[perm].contiguous()
        cls, _r, _s = ops.coco_accumulate(cat_off, ev.cat_gt_offsets, category_order(cat_off, score), zero_rank(nd, dev), score,
                                          self.cls_match[perm].reshape(1, 1, nd).contiguous(), self.cls_ignore[perm].reshape(1, 1, nd).contiguous(),
                                          self.fix_gt_ignore[:1].contiguous(), [NO_CUT], rec)
        return cls[0, :, :, 0, 0]

    def run(self, fg=0.5, bg=0.1):
        ev, dev = self.ev, self.ev.device
        hit = np.flatnonzero(np.isclose(ev.iou_thrs, fg))
        if hit.size == 0:
            raise ValueError(f"ErrorBreakdown: fg = {fg} is not one of the evaluator's IoU thresholds")
        I, K = len(ev.img_ids), len(ev.cat_ids)
        f = self._front_end(int(hit[0]))
        self._classify(f, fg, bg)
        self._fixes(f)
        dt_cat, gt_cat, dt_fp = f["dt_cat"], f["gt_cat"], f["dt_fp"]
        p = -np.ones((len(ev.rec_thrs), K, 9), np.float64)         # [:, :, 0] the base state, then FIXES
        if K and I:
            rec = torch.from_numpy(np.ascontiguousarray(ev.rec_thrs, np.float64)).to(dev)
            rows, cls = self._price_in_place(rec).cpu().numpy(), self._price_cls(f, rec).cpu().numpy()
            p[:, :, 0], p[:, :, 1] = rows[:, :, 0], cls
            for j, fix in enumerate(FIXES[1:]):
                p[:, :, 2 + j] = rows[:, :, _ROW_OF_FIX[fix]]
        self.precision = p
        kind64 = self.kind.to(torch.int64)
        per_kind = torch.bincount(kind64, minlength=6)[1:6]
        counts = torch.cat([per_kind, self.missed.sum(dtype=torch.int64).reshape(1), dt_fp.sum(dtype=torch.int64).reshape(1)]).cpu().numpy()
        per_cat = torch.zeros((K, 6), dtype=torch.int64, device=dev)
        if K:
            per_cat[:, :5] = torch.bincount(dt_cat.to(torch.int64) * 6 + kind64, minlength=6 * K).reshape(K, 6)[:, 1:]
            per_cat[:, 5] = torch.bincount(gt_cat.to(torch.int64)[self.missed != 0], minlength=K)
        # a category's curve is valid as a whole or not at all, so its AP is the mean along a contiguous row: the pairwise sum np.mean takes
        # of the same 101 values one category at a time
        curves = np.ascontiguousarray(p.transpose(1, 2, 0))        # [K, 9, R]
        ap = np.where(curves[:, :, 0] > -1, curves.mean(axis=-1), -1.0).reshape(K, 9)
        total = [_ap(p[:, :, j]) for j in range(9)]
        off = (ap[:, 1:] == -1) | (ap[:, :1] == -1)
        res = {"fg": float(fg), "bg": float(bg), "counts": counts.astype(np.int64), "counts_per_category": per_cat.cpu().numpy(),
               "ap_base": total[0], "ap_fixed": np.asarray(total[1:], np.float64),
               "dap": np.asarray([_delta(a, total[0]) for a in total[1:]], np.float64),
               "ap_per_category": ap,
               "dap_per_category": np.where(off, np.nan, ap[:, 1:] - ap[:, :1]).reshape(K, 8)}
        if ev.kind == "lvis":
            groups = [[_ap(p[:, :, j], cats) if len(cats) else np.float64(-1) for j in range(9)] for cats in ev.freq_groups]
            res["dap_per_frequency"] = np.asarray([[_delta(g[j], g[0]) for j in range(1, 9)] for g in groups], np.float64)
        self.result = res
        return res

    def report(self, file=None, per_category=False):
        """The table: one row per kind with its count and dAP, then the FP / FN rows."""
        if self.result is None:
            raise RuntimeError("ErrorBreakdown.report: call run() first")
        out, res = sys.stdout if file is None else file, self.result
        print(f"Error breakdown at IoU {res['fg']:0.2f} (background below {res['bg']:0.2f}): AP50 = {100 * res['ap_base']:0.2f}", file=out)
        print(f"{'kind':<6}{'count':>10}{'dAP50':>9}", file=out)
        n = list(res["counts"][:6]) + [res["counts"][6], None]
        for name, count, d in zip(FIXES, n, res["dap"]):
            print(f"{name:<6}{'' if count is None else int(count):>10}{100 * d:>9.2f}", file=out)
        print("Each dAP50 is the gain from fixing that kind alone; the rows do not add up to 100 - AP50.", file=out)
        if per_category:
            print(f"{'category':<10}" + "".join(f"{name:>8}" for name in FIXES), file=out)
            for cat, row in zip(self.ev.cat_ids, res["dap_per_category"]):
                print(f"{cat!s:<10}" + "".join(f"{100 * d:>8.2f}" for d in row), file=out)
        if "dap_per_frequency" in res:
            print(f"{'frequency':<10}" + "".join(f"{name:>8}" for name in FIXES), file=out)
            for f, row in zip("rcf", res["dap_per_frequency"]):
                print(f"{f:<10}" + "".join(f"{100 * d:>8.2f}" for d in row), file=out)
