#!/usr/bin/env python3
"""Fuse two or more COCO result files - or several passes of one model - by weighted boxes fusion on the device and evaluate the inputs and
the fusion side by side: the twelve COCO statistics of each, or with --lvis the thirteen LVIS statistics.
    python tools/fuse_models.py --gt instances_val2017.json --results a.json b.json c.json --weights 2 1 1 \\
        --iou_thr 0.55 --skip_box_thr 0.0 --conf_type avg --out fused.json
The rule is the one of include/mi355det.h, "Weighted boxes fusion" (DESIGN.md 7i); it was not run against the ensemble-boxes package."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="COCO (or, with --lvis, LVIS) ground-truth json")
    ap.add_argument("--results", nargs="+", required=True, metavar="A.json", help="result files (lists of result dicts), one per model")
    ap.add_argument("--names", nargs="+", default=None, help="column names (default: the file names)")
    ap.add_argument("--weights", type=float, nargs="+", default=None, help="one positive weight per result file (default: 1 each)")
    ap.add_argument("--iou_thr", type=float, default=0.55, help="a candidate joins a cluster whose fused box it overlaps by more than this")
    ap.add_argument("--skip_box_thr", type=float, default=0.0, help="drop detections with a score below this")
    ap.add_argument("--conf_type", default="avg", choices=["avg", "max"])
    ap.add_argument("--out", default=None, help="write the fused detections to this json file")
    ap.add_argument("--lvis", action="store_true", help="evaluate under the LVIS rules (an LVIS ground truth)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.weights is not None and len(args.weights) != len(args.results):
        ap.error("--weights: one weight per result file")
    if args.names is not None and len(args.names) != len(args.results):
        ap.error("--names: one name per result file")

    import torch
    from object_detectors_amd import ensemble
    names = args.names or [os.path.splitext(os.path.basename(p))[0] for p in args.results]
    if len(set(names)) != len(names) or "fusion" in names:
        names = [f"{n}_{k}" for k, n in enumerate(names)]
    results = []
    for path in args.results:
        with open(path) as f:
            results.append(json.load(f))
    stat_names, table, fusion = ensemble.evaluate_with_fusion(args.gt, results, names, lvis=args.lvis, device=torch.device(args.device),
                                                              weights=args.weights, iou_thr=args.iou_thr, skip_box_thr=args.skip_box_thr,
                                                              conf_type=args.conf_type)
    r = fusion.result
    print(f"== fusion of {len(results)} result sets ({', '.join(f'{n}: {len(rows)}' for n, rows in zip(names, results))} detections): "
          f"{int(r['score'].shape[0])} fused detections, weights {fusion.weights}, iou_thr {fusion.iou_thr}, skip_box_thr {fusion.skip_box_thr}, "
          f"conf_type {fusion.conf_type}{' (LVIS rules)' if args.lvis else ''}")
    print("dropped: " + ", ".join(f"{k} {v}" for k, v in r["dropped"].items()))
    ensemble.print_stats_table(stat_names, table)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(fusion.to_results(), f)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
