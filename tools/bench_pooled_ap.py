#!/usr/bin/env python3
"""AP-pool on the device at LVIS-v1-val size: the synthetic set of tools/bench_lviseval.py (19 809 images, 1203 categories, 300 detections per
image), evaluate() once, then the pooled precision-recall curve of the pool "all" by three routes on the same list:
    (a) mi355det_pooled_accumulate (csrc/pooled_kernels.hip), the new entry;
    (b) mi355det_coco_accumulate with the pool as its single category - the only way to this curve without the new entry;
    (c) the same arithmetic as torch ops on the device: cumsum, flipped cummax, searchsorted over all cells at once.
    python tools/bench_pooled_ap.py --reps 10 --warmup 5 --out profiles/r30_pooled_ap.md
Before any timing the three routes must agree bit for bit.  Each repetition times every route once, one after the other (HIP events round
each call), so the routes alternate within one process; the table gives the median and the range.  The pooled sort (torch: plumbing) is timed
apart, (a) is also timed on the four default pools all / r / c / f, and the AP-fixed front end stands next to the 300-per-image one.
--only-new runs route (a) alone, for a kernel trace taken in a run of its own."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_cocoeval import device_ms  # noqa: E402
from tools.bench_lviseval import SIZES, synth  # noqa: E402


def torch_route(order, npig, dt_score, dt_match, dt_ignore, rec):
    """One pool: precision [T, R, A], recall [T, A], scores [T, R, A] with torch ops (float64, the expressions of the rules)."""
    A, T, _nd = dt_match.shape
    n, R = int(order.shape[0]), int(rec.shape[0])
    matched, ignored = dt_match[:, :, order] != 0, dt_ignore[:, :, order] != 0
    tp = torch.cumsum(matched & ~ignored, -1).to(torch.float64)
    fp = torch.cumsum(~matched & ~ignored, -1).to(torch.float64)
    dn = npig.to(torch.float64).clamp(min=1).reshape(A, 1, 1)
    rc = tp / dn
    pr = tp / (fp + tp + float(np.spacing(1)))
    pr = torch.flip(torch.cummax(torch.flip(pr, [-1]), -1).values, [-1])
    first = torch.searchsorted(rc, rec.reshape(1, 1, R).expand(A, T, R).contiguous())
    inside, at = first < n, first.clamp(max=max(n - 1, 0))
    zero = torch.zeros((), dtype=torch.float64, device=rec.device)
    precision = torch.where(inside, pr.gather(-1, at), zero)
    scores = torch.where(inside, dt_score[order][at], zero)
    recall = rc[:, :, -1]
    none = (npig == 0).reshape(A, 1, 1)
    minus = torch.full((), -1.0, dtype=torch.float64, device=rec.device)
    return (torch.where(none, minus, precision).permute(1, 2, 0), torch.where(none[:, :, 0], minus, recall).permute(1, 0),
            torch.where(none, minus, scores).permute(1, 2, 0))


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=SIZES["images"])
    ap.add_argument("--categories", type=int, default=SIZES["categories"])
    ap.add_argument("--ground-truths", type=int, default=SIZES["ground_truths"])
    ap.add_argument("--detections", type=int, default=SIZES["detections"], help="per image")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only-new", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops
    from object_detectors_amd.lviseval import NO_CUT, LVISEval
    dev = torch.device("cuda:0")
    dataset, (d_img, d_cat, d_score, d_box) = synth(args.images, args.categories, args.ground_truths, args.detections, 0)
    dets = [torch.from_numpy(x).to(dev) for x in (d_img, d_cat, d_score, d_box)]
    e = LVISEval(dataset, device=dev)
    e.add(*dets)
    e.evaluate()
    rec = e._params()[2]
    pools = [c for _n, c in e.default_pools()]
    order4, off4, npig4, host4 = e.pool_lists(pools)
    order1, off1, npig1, host1 = e.pool_lists(pools[:1])
    new = lambda o, f, n, h: ops.pooled_accumulate(o, f, n, e.dt_score, e.dt_match, e.dt_ignore, rec, h)
    route_a = lambda: new(order1, off1, npig1, host1)
    route_a4 = lambda: new(order4, off4, npig4, host4)
    if args.only_new:
        for _ in range(args.warmup + args.reps):
            route_a4()
        torch.cuda.synchronize()
        return
    # (b): one category holding the pool; its ground truths are all of them, in slot order
    one_dt = torch.tensor([0, int(order1.shape[0])], dtype=torch.int64, device=dev)
    one_gt = torch.tensor([0, e.num_gt], dtype=torch.int64, device=dev)
    route_b = lambda: ops.coco_accumulate(one_dt, one_gt, order1, e.dt_rank, e.dt_score, e.dt_match, e.dt_ignore, e.gt_ignore, [NO_CUT], rec)
    route_c = lambda: torch_route(order1, npig1[0], e.dt_score, e.dt_match, e.dt_ignore, rec)
    pa, ra, sa = route_a()
    pb, rb, sb = route_b()
    pc, rc_, sc = route_c()
    assert torch.equal(pa[:, :, 0], pb[:, :, 0, :, 0]) and torch.equal(ra[:, 0], rb[:, 0, :, 0]) and torch.equal(sa[:, :, 0], sb[:, :, 0, :, 0]), \
        "mi355det_pooled_accumulate and mi355det_coco_accumulate disagree"
    assert torch.equal(pa[:, :, 0], pc) and torch.equal(ra[:, 0], rc_) and torch.equal(sa[:, :, 0], sc), "the torch route disagrees"
    p4 = route_a4()[0]
    assert torch.equal(p4[:, :, 0], pa[:, :, 0])
    routes = [("a", route_a), ("b", route_b), ("c", route_c), ("a4", route_a4), ("sort", lambda: e.pool_lists(pools))]
    times = {k: [] for k, _f in routes}
    for rep in range(args.warmup + args.reps):
        for k, fn in routes:
            t = timed(fn)
            if rep >= args.warmup:
                times[k].append(t)
    stat = lambda k, b="": f"{b}{np.median(times[k]):.3f}{b} | {min(times[k]):.3f} .. {max(times[k]):.3f}"
    # the front ends: 300 per image against AP-fixed (no per-image cut, 10 000 per category)
    t_front = device_ms(e._group, args.reps, args.warmup)
    kept_300 = e.num_dt
    f = LVISEval.fixed(dataset, device=dev)
    f.add(*dets)
    t_front_fixed = device_ms(f._group, args.reps, args.warmup)
    e.accumulate_pooled()
    res = e.summarize_pooled()
    P1, P4 = int(order1.shape[0]), int(order4.shape[0])
    lines = [
        "# AP-pool on the device at LVIS-v1-val size",
        "",
        f"tools/bench_pooled_ap.py, `bbox`: {args.images} images, {args.categories} categories, {args.ground_truths} ground truths, "
        f"{args.detections} detections per image ({e.num_added} in all, {kept_300} after the cut to 300 per image and the federated filter).  "
        f"The pool `all` is one list of {P1} slots, 40 cells (4 area ranges x 10 thresholds), 101 recall thresholds; the four default pools "
        f"all / r / c / f hold {P4} positions.  The three routes agreed bit for bit on precision, recall and scores before timing.  "
        f"{args.reps} repetitions after {args.warmup} warm-up rounds; every repetition runs each route once, in the order of the table, with HIP "
        "events round the call (output and workspace allocation included); median and range.",
        "",
        "| route | median ms | min .. max ms |",
        "|---|---:|---:|",
        f"| **(a) mi355det_pooled_accumulate**, pool `all` | {stat('a', '**')} |",
        f"| (b) mi355det_coco_accumulate, the pool as its single category | {stat('b')} |",
        f"| (c) torch ops: gather, cumsum, flipped cummax, searchsorted, all 40 cells at once | {stat('c')} |",
        f"| (a) on the four default pools all / r / c / f | {stat('a4')} |",
        f"| the pooled lists (torch mask and stable sort: plumbing), four pools | {stat('sort')} |",
        "",
        f"(b) / (a) = {np.median(times['b']) / np.median(times['a']):.1f}, (c) / (a) = {np.median(times['c']) / np.median(times['a']):.2f}.",
        "",
        "| front end (`_group`: cuts, federated filter, grouping) | device ms | slots kept |",
        "|---|---:|---:|",
        f"| 300 per image | {t_front:.3f} | {kept_300} |",
        f"| AP-fixed: no per-image cut, 10 000 per category | {t_front_fixed:.3f} | {f.num_dt} |",
        "",
        "Pooled statistics of this synthetic set (they say nothing about a model): " + ", ".join(f"{k} = {v:.4f}" for k, v in res.items()) + ".",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
