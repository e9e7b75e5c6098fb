#!/usr/bin/env python3
"""Bootstrap replicates of the accumulate pass at COCO-val and LVIS-v1-val size (the synthetic sets of tools/bench_cocoeval.py and
tools/bench_lviseval.py), `bbox`.
    python tools/bench_bootstrap.py --sets coco lvis --replicates 256 1024 --rounds 3 --out profiles/r18_bootstrap.md
Two routes to B replicates of one evaluated set, timed in one process with HIP events around whole routes, alternated round by round after
a warm-up of each:
    (a) evaluator.bootstrap(weights): mi355det_coco_bootstrap for all replicates and the torch reductions to the statistics, results on the
        host; its kernel part (weights to the device and transposed, the launches) is timed on its own as well;
    (b) what it replaces: B calls of ops.coco_accumulate one after the other on the same evaluator, nothing copied to the host.  (Route (b)
        computes one and the same replicate B times: the kernel it calls has no weights.  Its time does not depend on them.)
Before the timing the unit-weight replicate is compared with the evaluator's own accumulate() + summarize() at this size.  Prints the
markdown report and, with --out, writes it."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import bench_cocoeval, bench_lviseval  # noqa: E402

SIZES = {"coco": dict(images=5000, categories=80, ground_truths=36000, detections=100),
         "lvis": dict(images=19809, categories=1203, ground_truths=244707, detections=300)}


def once_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def evaluator(kind, size, dev):
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISEval
    synth = bench_cocoeval.synth if kind == "coco" else bench_lviseval.synth
    dataset, (d_img, d_cat, d_score, d_box) = synth(size["images"], size["categories"], size["ground_truths"], size["detections"], 0)
    e = COCOEval(dataset, "bbox", device=dev) if kind == "coco" else LVISEval(dataset, device=dev)
    e.add(torch.from_numpy(d_img).to(dev), torch.from_numpy(d_cat).to(dev), torch.from_numpy(d_score).to(dev), boxes=torch.from_numpy(d_box).to(dev))
    e.evaluate().accumulate()
    return e, list(e.cuts)


def bench(kind, size, replicates, rounds, dev):
    from object_detectors_amd import compare, ops
    from object_detectors_amd.cocoeval import bootstrap_cells, check_weights
    e, max_dets = evaluator(kind, size, dev)
    own = e.summarize(file=open(os.devnull, "w")) if kind == "coco" else np.asarray(list(e.summarize().values()))
    unit = e.bootstrap(np.ones((1, len(e.img_ids)), np.int32))[0]
    rec = torch.from_numpy(np.ascontiguousarray(e.rec_thrs)).to(dev)
    lines = [f"## {kind.upper()} size: {size['images']} images, {size['categories']} categories, {size['ground_truths']} ground truths, "
             f"{size['detections']} detections per image; {e.num_dt} detection slots, {e.num_gt} ground-truth slots after evaluate()", "",
             f"Unit weights against accumulate() + summarize() at this size: largest difference of a statistic {np.abs(unit - own).max():.2e}.", "",
             "| B | (a) bootstrap() ms | of which kernel route ms | reductions + host copy ms | (b) B x coco_accumulate ms | (b) / (a) | cells MB |",
             "|---:|---:|---:|---:|---:|---:|---:|"]
    routes = {}
    for B in replicates:
        w = compare.bootstrap_weights(len(e.img_ids), B, 0)
        wt = check_weights(w, len(e.img_ids), "bench")

        def kernel_route(wt=wt):
            for _cells in bootstrap_cells(e, wt, max_dets, 1 << 30):
                pass

        def sequential(B=B):
            for _ in range(B):
                ops.coco_accumulate(e.cat_dt_offsets, e.cat_gt_offsets, e.order, e.dt_rank, e.dt_score, e.dt_match, e.dt_ignore, e.gt_ignore, max_dets, rec)
        routes[B] = {"a": lambda w=w: e.bootstrap(w), "k": kernel_route, "b": sequential}
        e.bootstrap(w[:64])                                          # warm-up: code objects, allocator
        kernel_route(wt[:64])
        sequential(8)
    times = {B: {r: [] for r in "akb"} for B in replicates}
    for _ in range(rounds):
        for B in replicates:
            for r in "akb":
                times[B][r].append(once_ms(routes[B][r]))
    med = lambda xs: float(np.median(xs))
    span = lambda xs: f"{med(xs):.1f} ({min(xs):.1f} .. {max(xs):.1f})"
    for B in replicates:
        t = times[B]
        cells = 2 * 8 * B * len(e.iou_thrs) * len(e.cat_ids) * 4 * len(max_dets) / 1e6
        lines.append(f"| {B} | **{span(t['a'])}** | {span(t['k'])} | {med(t['a']) - med(t['k']):.1f} | **{span(t['b'])}** | "
                     f"**{med(t['b']) / med(t['a']):.1f}x** | {cells:.0f} |")
    return lines + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["coco", "lvis"], choices=sorted(SIZES))
    ap.add_argument("--replicates", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# Bootstrap replicates of the accumulate pass on the device", "",
             f"tools/bench_bootstrap.py on one MI355X, one process.  Per set and B, {args.rounds} rounds; in each round the routes run one after the "
             "other ((a), the kernel route of (a) alone, (b)), each once, HIP events around the whole route; median (min .. max) over the rounds.",
             ""]
    for kind in args.sets:
        lines += bench(kind, SIZES[kind], args.replicates, args.rounds, dev)
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
