#!/usr/bin/env python3
"""Why does a model lose AP50?  The error breakdown of one or two result files on the device (object_detectors_amd/tide.py, after TIDE):
every false positive at IoU 0.5 is Cls, Loc, Both, Dupe or Bkg, the ground truths nothing explains are Miss, and each kind is priced by the
AP50 gained when that kind alone is fixed.
    python tools/error_breakdown.py --gt instances_val2017.json --results baseline.json [other.json] [--lvis] [--per-category]
One table per model and, with two models, the difference of the dAP rows (second minus first).  Each fix is priced alone, so a table's rows
do not add up to 100 - AP50.  No plots."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="COCO (with --lvis: LVIS) ground-truth json")
    ap.add_argument("--results", nargs="+", required=True, metavar="A.json", help="one or two result files (lists of result dicts)")
    ap.add_argument("--lvis", action="store_true", help="evaluate under the LVIS rules; adds the rows per frequency group")
    ap.add_argument("--per-category", action="store_true", help="print the dAP rows of every category as well")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if len(args.results) > 2:
        ap.error("--results takes one or two files")

    import torch
    from object_detectors_amd.cocoeval import COCOEval, load_dataset
    from object_detectors_amd.lviseval import LVISEval
    from object_detectors_amd.tide import FIXES, ErrorBreakdown
    dev = torch.device(args.device)
    dataset = load_dataset(args.gt)
    names = [os.path.splitext(os.path.basename(p))[0] for p in args.results]
    found = []
    for name, path in zip(names, args.results):
        with open(path) as f:
            rows = json.load(f)
        print(f"== {name}: {len(rows)} detections")
        if args.lvis:
            ev = LVISEval(dataset, rows, device=dev)
        else:
            ev = COCOEval(dataset, "bbox", device=dev)
            ev.add_results(rows)
        b = ErrorBreakdown(ev.evaluate())
        found.append(b.run())
        b.report(per_category=args.per_category)
    if len(found) == 2:
        print(f"== dAP50 of {names[1]} minus dAP50 of {names[0]} (AP50 {100 * found[0]['ap_base']:0.2f} -> {100 * found[1]['ap_base']:0.2f})")
        for name, a, b in zip(FIXES, found[0]["dap"], found[1]["dap"]):
            print(f"{name:<6}{100 * (b - a):>+9.2f}")


if __name__ == "__main__":
    main()
