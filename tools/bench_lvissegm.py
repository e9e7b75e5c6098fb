#!/usr/bin/env python3
"""LVIS `segm` on the device: (a) result masks from their `counts` strings, the string kernels against the host codec, at COCO-val size
(500 000 masks) and LVIS-v1-val size (5.9 million); (b) LVISSegmEval.evaluate() / accumulate() at LVIS-v1-val size beside LVISEval (`bbox`)
on the same rectangles, by section.
    python tools/bench_lvissegm.py --reps 5 --warmup 1 --out profiles/r23_lvissegm.md
Synthetic and seeded.  (a): a pool of elliptical masks in a 480 x 640 image, encoded by the host codec; the N strings of a run are drawn from
the pool with repetition (every string is decoded on its own on both routes, so repetition does not help either).  The two routes are
alternated in one process, twice, and both rounds are printed: their difference is the spread.  The host route is what
`_MaskStore.add_segmentations` does for anything but a list of strings on a GPU (and did for strings before the string kernels); above
--host-sample masks it is timed on that many and scaled.  (b): the boxes of tools/bench_lviseval.py at a quarter of their scale in 180 x 180
images; ground truth as 4-point polygons (converted once, in the warm-up), detections as filled rectangles built on the device.  Device
figures are HIP events around the calls after a warm-up; wall figures are the wall clock around synchronised calls."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import bench_lviseval  # noqa: E402
from tools.bench_cocoeval import device_ms, wall_ms  # noqa: E402

H, W = 480, 640                                          # (a)
SH, SW, SCALE = 180, 180, 4                              # (b)


def ellipse_counts(rng):
    """The run lengths of a filled ellipse in an H x W image: one run of ones per column it covers."""
    a, b = np.exp(rng.uniform(np.log(4), np.log(150), 2))
    cx, cy = rng.uniform(0, W), rng.uniform(0, H)
    xs = np.arange(max(0, int(np.ceil(cx - a))), min(W, int(np.floor(cx + a)) + 1))
    if xs.size == 0:
        return np.asarray([H * W], np.int64)
    hh = b * np.sqrt(np.maximum(0.0, 1.0 - ((xs - cx) / a) ** 2))
    ya = np.clip(np.round(cy - hh), 0, H - 2).astype(np.int64)
    yb = np.clip(np.round(cy + hh) + 1, ya + 1, H - 1).astype(np.int64)
    edges = np.stack([xs * H + ya, xs * H + yb], 1).reshape(-1)
    return np.diff(np.concatenate([[0], edges, [H * W]]))


def string_pool(n, seed):
    from object_detectors_amd.rle import counts_to_string
    rng = np.random.RandomState(seed)
    return [counts_to_string(ellipse_counts(rng)) for _ in range(n)]


def bench_strings(n, pool, args, dev):
    """-> the markdown rows of one size."""
    from object_detectors_amd import cocoeval, ops
    from object_detectors_amd.rle import pack_strings
    rng = np.random.RandomState(n % 1000)
    strings = [pool[i] for i in rng.randint(0, len(pool), n)]
    segs = [{"size": [H, W], "counts": s} for s in strings]
    sizes = np.tile(np.asarray([[H, W]], np.int32), (n, 1))
    sample = segs[:min(n, args.host_sample)]
    chooser = cocoeval._counts_strings

    def host_route():
        cocoeval._counts_strings = lambda segs_: None      # the form test says "not strings": the host route, as before the string kernels
        try:
            cocoeval._MaskStore(dev).add_segmentations(sample)
        finally:
            cocoeval._counts_strings = chooser
    rounds = []
    for _ in range(2):                                      # the two routes alternated, twice
        t_dev = wall_ms(lambda: cocoeval._MaskStore(dev).add_segmentations(segs), args.string_reps, 1 if not rounds else 0)
        t_host = wall_ms(host_route, 1, 0) * (n / len(sample))
        rounds.append((t_dev, t_host))
    t_pack = wall_ms(lambda: pack_strings(strings), args.string_reps, 0)
    packed, offsets = pack_strings(strings)
    stamps = {}

    def mark(name):
        torch.cuda.synchronize()
        stamps[name] = time.perf_counter()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    counts, runs, _area, _bbox, status = ops.rle_strings(packed, offsets, sizes, dev, mark=mark)
    assert status is None
    t_up, t_cnt_w, t_emit_w = ((stamps[b] - a) * 1e3 for a, b in ((t0, "upload"), (stamps["upload"], "count"), (stamps["count"], "emit")))
    d_bytes, d_off, d_sz = torch.from_numpy(packed).to(dev), torch.from_numpy(offsets).to(dev), torch.from_numpy(sizes).to(dev)
    t_cnt = device_ms(lambda: ops.rle_strings_count(d_bytes, offsets, d_off, d_sz), args.reps, args.warmup)
    table, _st = ops.rle_strings_count(d_bytes, offsets, d_off, d_sz)
    total = int(runs[-1])
    t_emit = device_ms(lambda: ops.rle_strings_emit(d_bytes, d_off, d_sz, table, total), args.reps, args.warmup)
    scaled = "" if len(sample) == n else f" (timed on {len(sample)} masks, scaled)"
    return [f"| {n} | {packed.size / 1e6:.1f} MB, {total / 1e6:.1f} M counts | {t_pack:.1f} | {t_up:.1f} | {t_cnt:.3f} ({t_cnt_w:.1f}) | "
            f"{t_emit:.3f} ({t_emit_w:.1f}) | {rounds[0][0]:.1f} / {rounds[1][0]:.1f} | {rounds[0][1]:.0f} / {rounds[1][1]:.0f}{scaled} | "
            f"{min(r[1] for r in rounds) / max(r[0] for r in rounds):.1f}x |"]


def rect_of(box):
    """float boxes [n, 4] of tools/bench_lviseval.py -> integer rectangles inside the SH x SW image, below the full column height."""
    b = np.asarray(box, np.float64) / SCALE
    x = np.clip(b[:, 0].astype(np.int64), 0, SW - 2)
    y = np.clip(b[:, 1].astype(np.int64), 0, SH - 2)
    w = np.clip(b[:, 2].astype(np.int64), 1, SW - x)
    h = np.clip(b[:, 3].astype(np.int64), 1, SH - 1 - y)
    return np.stack([x, y, w, h], 1)


def rect_runs(rects, dev):
    """The run lengths of filled rectangles (h < SH) on the device: mask j has 2 w + 1 counts: x*SH + y, then h, SH - h, ..., h, the rest."""
    r = torch.from_numpy(rects).to(dev)
    x, y, w, h = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    lens = 2 * w + 1
    runs = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(lens, 0)])
    owner = torch.repeat_interleave(torch.arange(r.shape[0], device=dev), lens)
    pos = torch.arange(int(runs[-1]), device=dev) - runs[owner]
    first = x * SH + y
    tail = SH * SW - (first + (w - 1) * SH + h)
    counts = torch.where(pos == 0, first[owner], torch.where(pos % 2 == 1, h[owner], torch.where(pos == lens[owner] - 1, tail[owner], SH - h[owner])))
    return counts.to(torch.int32), runs


def sections(e, reps, warmup):
    from object_detectors_amd import ops
    t_front = device_ms(e._group, reps, warmup), wall_ms(e._group, reps, 0)
    iou_size = e._group()
    thr, rng, _rec = e._params()
    t_iou = device_ms(lambda: ops.coco_iou(e.dt_offsets, e.gt_offsets, e.iou_offsets, iou_size, e.dt_boxes, e.gt_boxes, e.gt_crowd, e._rle),
                      reps, warmup)
    e._match(iou_size)
    t_match = device_ms(lambda: ops.lvis_match(e.dt_offsets, e.gt_offsets, e.iou_offsets, e.iou, e.dt_area, e.gt_area, e.gt_flag,
                                               e.group_not_exhaustive, thr, rng), reps, warmup)
    t_acc = device_ms(e.accumulate, reps, warmup), wall_ms(e.accumulate, reps, 0)
    t_eval = wall_ms(e.evaluate, reps, 0)
    return {"front": t_front, "iou": t_iou, "match": t_match, "acc": t_acc, "eval": t_eval, "iou_size": iou_size, "res": e.summarize()}


def bench_eval(args, dev):
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    from object_detectors_amd.rle import RLEBatch
    dataset, (d_img, d_cat, d_score, d_box) = bench_lviseval.synth(args.images, args.categories, args.ground_truths, args.detections, 0)
    g = rect_of([a["bbox"] for a in dataset["annotations"]])
    for a, (x, y, w, h) in zip(dataset["annotations"], g.tolist()):
        a["bbox"], a["area"] = [float(x), float(y), float(w), float(h)], float(w * h)
        a["segmentation"] = [[x, y, x + w, y, x + w, y + h, x, y + h]]
    for im in dataset["images"]:
        im["height"], im["width"] = SH, SW
    d = rect_of(d_box)
    ids, cats, scores = (torch.from_numpy(v).to(dev) for v in (d_img, d_cat, d_score))
    box = LVISEval(dataset, device=dev)
    box.add(ids, cats, scores, torch.from_numpy(d.astype(np.float32)).to(dev))
    segm = LVISSegmEval(dataset, device=dev)
    counts, runs = rect_runs(d, dev)
    dd = torch.from_numpy(d).to(dev)
    segm.add(ids, cats, scores, masks=RLEBatch((SH, SW), counts, runs.tolist(), dd[:, 2] * dd[:, 3], dd.to(torch.int32)))
    t = time.perf_counter()
    segm._ground_truth()
    t_gt = time.perf_counter() - t
    out = {"bbox": sections(box, args.reps, args.warmup), "segm": sections(segm, args.reps, args.warmup)}
    b, s = out["bbox"], out["segm"]
    return [
        f"{args.images} images of {SH} x {SW}, {args.categories} categories, {args.ground_truths} ground truths, {args.detections} detections "
        f"per image ({segm.num_added} in all, {segm.num_dt} after the cut and the federated filter; {int(counts.shape[0]) / 1e6:.0f} M counts of "
        f"detection masks on the device), {s['iou_size']} IoU pairs.  The polygon ground truth takes {t_gt:.1f} s once (host flattening, "
        "polygons.segmentations_to_rle), outside the sections.",
        "",
        "| section | `bbox` device ms | `bbox` wall ms | `segm` device ms | `segm` wall ms |",
        "|---|---:|---:|---:|---:|",
        f"| front end (cut, federated filter, grouping; `segm`: the masks' tensors and the per-group sizes too) | {b['front'][0]:.3f} | "
        f"{b['front'][1]:.3f} | {s['front'][0]:.3f} | {s['front'][1]:.3f} |",
        f"| IoU: mi355det_coco_iou (`segm`: run-length mode) | {b['iou']:.3f} | | {s['iou']:.3f} | |",
        f"| match: mi355det_lvis_match | {b['match']:.3f} | | {s['match']:.3f} | |",
        f"| accumulate() | {b['acc'][0]:.3f} | {b['acc'][1]:.3f} | {s['acc'][0]:.3f} | {s['acc'][1]:.3f} |",
        f"| evaluate() = front end + IoU + match | | {b['eval']:.3f} | | {s['eval']:.3f} |",
        "",
        f"`bbox`: AP = {b['res']['AP']:.4f}, APr = {b['res']['APr']:.4f}; `segm`: AP = {s['res']['AP']:.4f}, APr = {s['res']['APr']:.4f} "
        "(the ground-truth masks are rleFrPoly's rasterisation of the rectangles, so the two differ slightly; they say nothing about a model).",
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--masks", type=int, nargs="+", default=[500000, 5900000])
    ap.add_argument("--pool", type=int, default=20000)
    ap.add_argument("--host-sample", type=int, default=50000, help="the host route is timed on at most this many masks above COCO-val size")
    ap.add_argument("--string-reps", type=int, default=2)
    ap.add_argument("--images", type=int, default=bench_lviseval.SIZES["images"])
    ap.add_argument("--categories", type=int, default=bench_lviseval.SIZES["categories"])
    ap.add_argument("--ground-truths", type=int, default=bench_lviseval.SIZES["ground_truths"])
    ap.add_argument("--detections", type=int, default=bench_lviseval.SIZES["detections"], help="per image")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--skip-eval", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    pool = string_pool(args.pool, 0)
    lines = ["# LVIS `segm` on the device: result masks from strings, LVISSegmEval", "",
             "## (a) `counts` strings to run lengths, area and tight box", "",
             f"tools/bench_lvissegm.py: elliptical masks in a {H} x {W} image, {np.mean([len(s) for s in pool]):.0f} characters per string on "
             f"average, drawn from a pool of {len(pool)}.  pack = rle.pack_strings on the host; upload = the bytes and the table; count / emit = "
             "ops.rle_strings_count / _emit with their output allocation, HIP events (in brackets: wall clock inside ops.rle_strings, the count "
             "figure with the one host read); device route / host route = `_MaskStore(cuda).add_segmentations(list of dicts)` end to end, wall "
             "clock, first round / second round.", "",
             "| masks | bytes, counts | pack ms | upload ms | count ms | emit ms | device route ms | host route ms | host / device |",
             "|---:|---|---:|---:|---:|---:|---:|---:|---:|"]
    for n in args.masks:
        args_n = argparse.Namespace(**vars(args))
        if n <= 500000:
            args_n.host_sample = n                          # COCO-val size: the host route in full
        lines += bench_strings(n, pool, args_n, dev)
        print(lines[-1], file=sys.stderr, flush=True)
    if not args.skip_eval:
        lines += ["", "## (b) LVISSegmEval beside LVISEval at LVIS-v1-val size", ""] + bench_eval(args, dev)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
