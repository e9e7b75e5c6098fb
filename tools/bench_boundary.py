#!/usr/bin/env python3
"""Boundary IoU on the device: (a) mask boundaries as run lengths (ops.rle_boundary, csrc/boundary_kernels.hip) against the dense route a
user has without it - ops.mask_rle_decode, 1 - max_pool2d(1 - m, 2d + 1, stride 1) with the image border as 0, ops.mask_rle_dense - at
COCO-val size (500 000 masks) and LVIS-v1-val size (5.9 million); (b) LVISSegmEval.evaluate() for `boundary` beside `segm` at LVIS-v1-val
size.
    python tools/bench_boundary.py --reps 3 --warmup 1 --out profiles/r24_boundary.md
Synthetic and seeded: the elliptical masks of tools/bench_lvissegm.py in a 480 x 640 image (d = 16), drawn from a pool with repetition and
gathered on the device (every mask is converted on its own on both routes).  The two routes are alternated in one process, twice, and both
rounds are printed: their difference is the spread.  Both work in chunks under the same byte budget; the dense route (one image size per
chunk, float32 bitmaps) is timed on --dense-sample masks and scaled above that, after its result has been compared with the device route's.
Device figures are HIP events around the calls after a warm-up; wall figures are the wall clock around synchronised calls, host planning
and the host read included."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import bench_lviseval, bench_lvissegm  # noqa: E402
from tools.bench_cocoeval import device_ms, wall_ms  # noqa: E402

H, W = bench_lvissegm.H, bench_lvissegm.W


def mask_pool(n, seed, dev):
    """n elliptical masks: (counts int32 on the device, runs int64 [n + 1] host, tight boxes int32 [n, 4] host)."""
    from object_detectors_amd.rle import counts_stats
    rng = np.random.RandomState(seed)
    cs = [bench_lvissegm.ellipse_counts(rng) for _ in range(n)]
    runs = np.concatenate([[0], np.cumsum([c.size for c in cs])]).astype(np.int64)
    flat = np.concatenate(cs).astype(np.int32)
    _area, bbox = counts_stats(flat, runs, H)
    return torch.from_numpy(flat).to(dev), runs, bbox


def draw(pool, n, dev):
    """n masks of the pool with repetition, gathered on the device -> (counts, runs host, boxes host)."""
    counts, runs, bbox = pool
    pick = np.random.RandomState(n % 1000).randint(0, len(runs) - 1, n)
    lens = np.diff(runs)[pick]
    out_runs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    d_lens = torch.from_numpy(lens).to(dev)
    owner = torch.repeat_interleave(torch.arange(n, device=dev), d_lens)
    src = torch.from_numpy(runs[:-1][pick]).to(dev)[owner] + (torch.arange(int(out_runs[-1]), device=dev) - torch.from_numpy(out_runs[:-1]).to(dev)[owner])
    return counts[src].contiguous(), out_runs, np.ascontiguousarray(bbox[pick])


def dense_route(counts, runs, d, budget_bytes):
    """The same boundaries through bitmaps: decode, erode by max-pooling the complement (the image border counts as 0), subtract, encode;
    chunks of masks whose float32 bitmaps (four live at the peak) stay within the budget.  -> [(counts, offsets)] per chunk."""
    from object_detectors_amd import ops
    n = len(runs) - 1
    per = max(1, int(budget_bytes) // (4 * 4 * H * W))
    out = []
    for j0 in range(0, n, per):
        j1 = min(n, j0 + per)
        m = ops.mask_rle_decode(counts[runs[j0]:runs[j1]], (runs[j0:j1 + 1] - runs[j0]).tolist(), (H, W)).to(torch.float32)
        inv = torch.nn.functional.pad(1 - m, (d, d, d, d), value=1.0)
        eroded = 1 - torch.nn.functional.max_pool2d(inv[:, None], 2 * d + 1, stride=1)[:, 0]
        b = ops.mask_rle_dense(m * (1 - eroded), 0.5)
        out.append((b.counts, b.offsets))
    return out


def bench_convert(n, pool, args, dev):
    from object_detectors_amd import ops
    from object_detectors_amd.rle import boundary_dilation
    d = boundary_dilation(H, W)
    counts, runs, boxes = draw(pool, n, dev)
    sizes = np.tile(np.asarray([[H, W]], np.int32), (n, 1))
    ns = min(n, args.dense_sample)
    s_counts, s_runs = counts[:runs[ns]], runs[:ns + 1]
    device = lambda: ops.rle_boundary(counts, runs, sizes, d, boxes, budget_bytes=args.budget)
    dense = lambda: dense_route(s_counts, s_runs, d, args.budget)
    # the two routes agree on the sample
    got = ops.rle_boundary(s_counts, s_runs, sizes[:ns], d, boxes[:ns], budget_bytes=args.budget)
    ref = dense()
    assert torch.equal(got[0], torch.cat([c for c, _o in ref])) and int(got[1][-1]) == sum(o[-1] for _c, o in ref)
    rounds = []
    for _ in range(2):
        t_dev = wall_ms(device, args.convert_reps, 1 if not rounds else 0)
        t_dense = wall_ms(dense, 1, 0) * (n / ns)
        rounds.append((t_dev, t_dense))
    plan = ops.BoundaryPlan(counts, runs, sizes, d, boxes, None, args.budget)
    t = time.perf_counter()
    ops.BoundaryPlan(counts, runs, sizes, d, boxes, None, args.budget)
    torch.cuda.synchronize()
    t_plan = (time.perf_counter() - t) * 1e3
    t_cnt = device_ms(plan.count, args.reps, args.warmup)
    run_offsets = plan.count()
    total = int(run_offsets[-1])
    t_emit = device_ms(lambda: plan.emit(run_offsets, total), args.reps, args.warmup)
    scaled = "" if ns == n else f" (timed on {ns} masks, scaled)"
    return (f"| {n} | {int(runs[-1]) / 1e6:.1f} M in, {total / 1e6:.1f} M out | {len(plan.chunks)} x <= {plan.nbytes / 2 ** 20:.0f} MiB | {t_plan:.1f} | "
            f"{t_cnt:.3f} | {t_emit:.3f} | {rounds[0][0]:.1f} / {rounds[1][0]:.1f} | {rounds[0][1]:.0f} / {rounds[1][1]:.0f}{scaled} | "
            f"{min(r[1] for r in rounds) / max(r[0] for r in rounds):.1f}x |")


def bench_eval(args, dev):
    """LVISSegmEval at LVIS-v1-val size on the rectangles of tools/bench_lvissegm.py, `segm` and `boundary` alternated."""
    from object_detectors_amd.lviseval import LVISSegmEval
    from object_detectors_amd.rle import RLEBatch, boundary_dilation
    SH, SW = bench_lvissegm.SH, bench_lvissegm.SW
    dataset, (d_img, d_cat, d_score, d_box) = bench_lviseval.synth(args.images, args.categories, args.ground_truths, args.detections, 0)
    g = bench_lvissegm.rect_of([a["bbox"] for a in dataset["annotations"]])
    for a, (x, y, w, h) in zip(dataset["annotations"], g.tolist()):
        a["bbox"], a["area"] = [float(x), float(y), float(w), float(h)], float(w * h)
        a["segmentation"] = [[x, y, x + w, y, x + w, y + h, x, y + h]]
    for im in dataset["images"]:
        im["height"], im["width"] = SH, SW
    d = bench_lvissegm.rect_of(d_box)
    ids, cats, scores = (torch.from_numpy(v).to(dev) for v in (d_img, d_cat, d_score))
    counts, runs = bench_lvissegm.rect_runs(d, dev)
    dd = torch.from_numpy(d).to(dev)
    evs, t_gt = {}, {}
    for kind in ("segm", "boundary"):
        e = LVISSegmEval(dataset, device=dev, iou_type=kind)
        e.add(ids, cats, scores, masks=RLEBatch((SH, SW), counts, runs.tolist(), dd[:, 2] * dd[:, 3], dd.to(torch.int32)))
        t = time.perf_counter()
        e._ground_truth()
        torch.cuda.synchronize()
        t_gt[kind] = time.perf_counter() - t
        evs[kind] = e
    rounds = []
    for _ in range(2):
        rounds.append(tuple(wall_ms(evs[kind].evaluate, args.reps, 1 if not rounds else 0) for kind in ("segm", "boundary")))
    t_conv = wall_ms(lambda: evs["boundary"]._masks.boundaries(0.02), args.reps, 0)
    res = {kind: e.accumulate().summarize() for kind, e in evs.items()}
    s = evs["segm"]
    return [
        f"{args.images} images of {SH} x {SW} (d = {boundary_dilation(SH, SW)}), {args.categories} categories, {args.ground_truths} ground truths, "
        f"{args.detections} detections per image ({s.num_added} in all, {s.num_dt} after the cut and the federated filter; "
        f"{int(counts.shape[0]) / 1e6:.0f} M counts of detection masks on the device).  The ground truth (polygons to run lengths, once per "
        f"evaluator) takes {t_gt['segm']:.1f} s for `segm` and {t_gt['boundary']:.1f} s for `boundary`, which also makes its boundaries.",
        "",
        "| evaluate(), wall ms, first round / second round | `segm` | `boundary` |",
        "|---|---:|---:|",
        f"| front end + IoU + match | {rounds[0][0]:.1f} / {rounds[1][0]:.1f} | {rounds[0][1]:.1f} / {rounds[1][1]:.1f} |",
        f"| of which the detections' boundaries (`_MaskStore.boundaries`, all {s.num_added} masks) | | {t_conv:.1f} |",
        "",
        f"`segm`: AP = {res['segm']['AP']:.4f}, APr = {res['segm']['APr']:.4f}; `boundary`: AP = {res['boundary']['AP']:.4f}, APr = "
        f"{res['boundary']['APr']:.4f} (filled rectangles against rleFrPoly's rasterisation of the same rectangles; they say nothing about a model).",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", type=int, nargs="+", default=[500000, 5900000])
    ap.add_argument("--pool", type=int, default=20000)
    ap.add_argument("--dense-sample", type=int, default=2000, help="the dense route is timed on at most this many masks")
    ap.add_argument("--budget", type=int, default=1 << 30, help="bytes of scratch (device route) or of bitmaps (dense route) per chunk")
    ap.add_argument("--convert-reps", type=int, default=2)
    ap.add_argument("--images", type=int, default=bench_lviseval.SIZES["images"])
    ap.add_argument("--categories", type=int, default=bench_lviseval.SIZES["categories"])
    ap.add_argument("--ground-truths", type=int, default=bench_lviseval.SIZES["ground_truths"])
    ap.add_argument("--detections", type=int, default=bench_lviseval.SIZES["detections"], help="per image")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-eval", action="store_true")
    ap.add_argument("--skip-convert", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pool = mask_pool(args.pool, 0, dev)
    lines = ["# Boundary IoU on the device: mask boundaries as run lengths, LVISSegmEval with `boundary`", "",
             "## (a) run lengths to the run lengths, area and tight box of the boundary", "",
             f"tools/bench_boundary.py: elliptical masks in a {H} x {W} image (d = 16), {np.diff(pool[1]).mean():.0f} counts per mask on average, "
             f"drawn from a pool of {len(pool[1]) - 1}.  plan = the host checks, the scratch layout and the table uploads (wall); count / emit = "
             "the two kernel passes over all chunks with their output allocation, HIP events; device route = ops.rle_boundary end to end with the "
             "host read; dense route = ops.mask_rle_decode, max_pool2d of the complement, ops.mask_rle_dense under the same byte budget; both "
             "wall clock, first round / second round.", "",
             "| masks | counts | chunks | plan ms | count ms | emit ms | device route ms | dense route ms | dense / device |",
             "|---:|---|---|---:|---:|---:|---:|---:|---:|"]
    for n in ([] if args.skip_convert else args.masks):
        lines.append(bench_convert(n, pool, args, dev))
        print(lines[-1], file=sys.stderr, flush=True)
    if not args.skip_eval:
        lines += ["", "## (b) LVISSegmEval: `boundary` beside `segm` at LVIS-v1-val size", ""] + bench_eval(args, dev)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
