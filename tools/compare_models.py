#!/usr/bin/env python3
"""Compare two COCO result files on the device: the per-category COCO statistics of each (the reference's notebooks/get_map.py) and the
2 x 2 table of ground-truth instances each gets right with McNemar's test (its notebooks/get_disagreement.py).
    python tools/compare_models.py --gt instances_val2017.json --results baseline.json other.json \\
        --iou_threshold 0.5 --confidence 0.0 --alpha 0.05 --metric_columns 0 1 --table per_category.json
The first result file is the baseline (model 0, "Correct1" in the table).  No plots.
--bootstrap B [--seed S] [--lvis] adds a last block: is the difference in AP more than noise?  Percentile intervals of AP, AP50
and AP75 per model over B resamples of the images (all replicates in one kernel: COCOEval.bootstrap) and the paired difference with its p.
--fuse adds a last block: what the two models score together - the statistics of A, B and their weighted boxes fusion at default parameters
side by side (under --lvis the LVIS statistics; tools/fuse_models.py takes more than two files, weights and the other parameters)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--gt", required=True, help="COCO ground-truth json")
    ap.add_argument("--results", nargs=2, required=True, metavar=("A.json", "B.json"), help="two COCO result files (lists of result dicts)")
    ap.add_argument("--names", nargs=2, default=None, help="experiment names for the table (default: the file names)")
    ap.add_argument("--iou_threshold", type=float, default=0.5, help="IoU at which an instance counts as found")
    ap.add_argument("--confidence", type=float, default=0.0, help="keep detections with score > confidence")
    ap.add_argument("--alpha", type=float, default=0.05, help="significance level of McNemar's test")
    ap.add_argument("--max_dets", type=int, default=None, help="keep each image's best-scored detections (300 for LVIS-style results)")
    ap.add_argument("--metric_columns", type=int, nargs="+", default=[0],
                    help="which of AP AP50 AP75 APs APm APl AR1 AR10 AR100 ARs ARm ARl (0..11) go into the per-category table")
    ap.add_argument("--table", default=None, help="write the per-category table to this json file")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--bootstrap", type=int, default=0, metavar="B",
                    help="add a block with bootstrap intervals of AP / AP50 / AP75 per model and their paired difference over B resamples of the images")
    ap.add_argument("--seed", type=int, default=0, help="seed of the resamples")
    ap.add_argument("--lvis", action="store_true", help="the bootstrap block under the LVIS rules (an LVIS ground truth; adds APr / APc / APf)")
    ap.add_argument("--fuse", action="store_true", help="add a block with the statistics of A, B and their weighted boxes fusion side by side")
    args = ap.parse_args(argv)

    import torch
    from object_detectors_amd import compare
    from object_detectors_amd.cocoeval import COCOEval, load_dataset
    dev = torch.device(args.device)
    dataset = load_dataset(args.gt)
    names = args.names or [os.path.splitext(os.path.basename(p))[0] for p in args.results]
    if names[0] == names[1]:
        names = [names[0] + "_0", names[1] + "_1"]
    results = []
    for path in args.results:
        with open(path) as f:
            results.append(json.load(f))

    evaluators = {}
    for name, rows in zip(names, results):
        print(f"== {name}: {len(rows)} detections")
        e = COCOEval(dataset, "bbox", device=dev)
        e.add_results(rows)
        e.evaluate().accumulate().summarize()
        evaluators[name] = e
    table = compare.per_category_table(evaluators, args.metric_columns)
    cats = {c["id"]: c.get("name", str(c["id"])) for c in dataset["categories"]}
    cat_ids = evaluators[names[0]].cat_ids
    for col in table["columns"]:
        print(f"== {col} per category ({names[0]} | {names[1]} | difference)")
        for k, cat in enumerate(cat_ids):
            a, b = table[names[0]][col][k], table[names[1]][col][k]
            print(f"{cats[cat]:>24s} {a:8.4f} {b:8.4f} {b - a:+8.4f}")
    if args.table:
        with open(args.table, "w") as f:
            json.dump(dict(table, category_ids=cat_ids), f)
        print("wrote", args.table)

    d = compare.Disagreement(dataset, device=dev, max_dets=args.max_dets)
    d.add_results(0, results[0])
    d.add_results(1, results[1])
    r = d.run(args.iou_threshold, args.confidence)
    print(f"== disagreement: {names}, {r['total']} instances on {len(d.img_ids) - r['missed']} images ({r['missed']} images not counted)")
    d.report(alpha=args.alpha)
    if args.bootstrap:
        bootstrap_block(args, dataset, results, names, evaluators, dev)
    if args.fuse:
        fuse_block(args, dataset, results, names, dev)


def fuse_block(args, dataset, results, names, dev):
    """The statistics of both models and of their weighted boxes fusion (default parameters, equal weights) side by side."""
    from object_detectors_amd import ensemble
    columns = [n + "_" + str(k) for k, n in enumerate(names)] if "fusion" in names else names
    stat_names, table, fusion = ensemble.evaluate_with_fusion(dataset, results, columns, lvis=args.lvis, device=dev)
    print(f"== fusion: weighted boxes fusion of {names}, iou_thr {fusion.iou_thr}, conf_type {fusion.conf_type}, equal weights: "
          f"{int(fusion.result['score'].shape[0])} fused detections{' (LVIS rules)' if args.lvis else ''}")
    ensemble.print_stats_table(stat_names, table)


def bootstrap_block(args, dataset, results, names, evaluators, dev):
    """Percentile intervals of AP, AP50, AP75 (under --lvis also APr, APc, APf) per model over resampled images, and the paired difference:
    both models see the same resamples."""
    from object_detectors_amd import compare
    if args.lvis:
        from object_detectors_amd.lviseval import RESULT_KEYS, LVISEval
        evs = [LVISEval(dataset, rows, device=dev).evaluate() for rows in results]
        columns = [(RESULT_KEYS.index(k), k) for k in ("AP", "AP50", "AP75", "APr", "APc", "APf")]
    else:
        evs = [evaluators[n] for n in names]
        columns = [(0, "AP"), (1, "AP50"), (2, "AP75")]
    weights = compare.bootstrap_weights(len(evs[0].img_ids), args.bootstrap, args.seed)
    a, b = (e.bootstrap(weights) for e in evs)
    paired = compare.paired_bootstrap(a, b)
    print(f"== bootstrap: {args.bootstrap} resamples of {len(evs[0].img_ids)} images, seed {args.seed}, 95% percentile intervals"
          f"{' (LVIS rules)' if args.lvis else ''}")
    for c, key in columns:
        for name, v in zip(names, (a, b)):
            i = compare.interval(v[:, c])
            print(f"{key:>6s} {name:>24s} {i['mean']:8.4f} [{i['lo']:.4f}, {i['hi']:.4f}] ({i['n_used']} used)")
        print(f"{key:>6s} {'difference':>24s} {paired['delta_mean'][c]:+8.4f} [{paired['lo'][c]:+.4f}, {paired['hi'][c]:+.4f}] "
              f"p={paired['p'][c]:.4f} ({paired['n_used'][c]} used)")


if __name__ == "__main__":
    main()
