#!/usr/bin/env python3
"""One LVIS result file under the three protocols, on the device:
    python tools/lvis_protocols.py --gt lvis_v1_val.json --results A.json [--segm | --boundary] [--per-cat K]
prints the standard table (300 detections per image: LVISEval(...).run()), the AP-fixed table (no per-image cut, each category's K = 10 000
best detections of the data set: LVISEval.fixed) and the AP-pool table of the AP-fixed evaluation (all categories' detections ranked in one
list: accumulate_pooled).  AP-fixed and AP-pool are those of Dave et al., "Evaluating Large-Vocabulary Object Detectors: The Devil is in the
Details" (2021), restated from memory of the paper and of its fork of lvis-api (include/mi355det.h, "Pooled precision-recall")."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gt", required=True, help="the LVIS ground truth json")
    ap.add_argument("--results", required=True, help="a results json (a list of result dicts)")
    kind = ap.add_mutually_exclusive_group()
    kind.add_argument("--segm", action="store_true", help="mask AP (results carry `segmentation`)")
    kind.add_argument("--boundary", action="store_true", help="Boundary AP")
    ap.add_argument("--per-cat", type=int, default=None, metavar="K", help="the category cut of AP-fixed (default 10000)")
    args = ap.parse_args(argv)
    from object_detectors_amd.lviseval import FIXED_DETS_PER_CAT, LVISEval, LVISSegmEval
    with open(args.gt) as f:
        gt = json.load(f)
    with open(args.results) as f:
        results = json.load(f)
    if args.segm or args.boundary:
        cls, kw = LVISSegmEval, {"iou_type": "boundary" if args.boundary else "segm"}
    else:
        cls, kw = LVISEval, {}
    per_cat = FIXED_DETS_PER_CAT if args.per_cat is None else args.per_cat
    standard = cls(gt, results, **kw).run()
    print(f"standard: {standard.max_dets} detections per image")
    standard.print_results()
    fixed = cls(gt, results, max_dets=None, max_dets_per_cat=per_cat, **kw).run()
    print(f"AP-fixed: no per-image cut, {per_cat} detections per category")
    fixed.print_results()
    print("AP-pool, on the AP-fixed detections")
    fixed.accumulate_pooled().print_pooled()
    return standard, fixed


if __name__ == "__main__":
    main()
