#!/usr/bin/env python3
"""Polygon ground truth to run lengths on the device, at COCO-val size: 5000 images of 480 x 640 and 36 000 annotations of star-shaped
polygons with 8 to 60 vertices, about one annotation in eight with 2 or 3 parts (synthetic: no dataset is read).
    python tools/bench_poly_rle.py --reps 5 --out profiles/r15_poly_rle.md
The stages of ops.poly_rle are timed with HIP events recorded between them (the host reads that size the buffers fall into the stage that
waits for them); dataset_to_rle end to end with the wall clock around a synchronised call (host flattening and the count lists included).
Prints the markdown table and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def star(rng, h, w):
    k = int(rng.integers(8, 61))
    cx, cy = rng.uniform(0, w), rng.uniform(0, h)
    r = rng.uniform(6, 110)
    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
    rad = r * rng.uniform(0.45, 1.0, k)
    return np.round(np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], 1), 2).reshape(-1).tolist()


def synth(images, annotations, h, w, seed):
    rng = np.random.default_rng(seed)
    ds = {"images": [{"id": i + 1, "height": h, "width": w} for i in range(images)], "categories": [{"id": c + 1} for c in range(80)],
          "annotations": []}
    for j in range(annotations):
        parts = 1 if rng.integers(0, 8) else int(rng.integers(2, 4))
        ds["annotations"].append({"id": j + 1, "image_id": int(rng.integers(1, images + 1)), "category_id": int(rng.integers(1, 81)),
                                  "iscrowd": 0, "segmentation": [star(rng, h, w) for _ in range(parts)]})
    return ds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--annotations", type=int, default=36000)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops, polygons
    dev = torch.device("cuda:0")
    H, W = args.height, args.width
    ds = synth(args.images, args.annotations, H, W, 0)
    segs = [a["segmentation"] for a in ds["annotations"]]
    t = time.perf_counter()
    tables = polygons.flatten(segs, [(H, W)] * len(segs))
    t_flatten = (time.perf_counter() - t) * 1e3
    xy = torch.from_numpy(tables[0]).to(dev)

    names = ["points", "sort", "events", "runs"]
    sums = dict.fromkeys(names, 0.0)
    total = 0.0
    for rep in range(args.warmup + args.reps):
        marks = [torch.cuda.Event(enable_timing=True)]
        torch.cuda.synchronize()
        marks[0].record()

        def mark(_name):
            marks.append(torch.cuda.Event(enable_timing=True))
            marks[-1].record()
        counts, offsets, _area, _bbox = ops.poly_rle(xy, *tables[1:], mark=mark)
        torch.cuda.synchronize()
        if rep >= args.warmup:
            for n, a, b in zip(names, marks, marks[1:]):
                sums[n] += a.elapsed_time(b)
            total += marks[0].elapsed_time(marks[-1])
    ms = {n: sums[n] / args.reps for n in names}
    total /= args.reps

    def wall(fn):
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / args.reps
    t_dataset = wall(lambda: polygons.dataset_to_rle(ds, dev))

    per_image = max(1, round(args.annotations / args.images))
    one = polygons.polygons_to_rle(segs[:per_image], H, W, dev)
    for _ in range(args.warmup):
        ops.mask_rle_decode(one)
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(20):
        ops.mask_rle_decode(one)
    e.record()
    e.synchronize()
    t_decode = s.elapsed_time(e) / 20

    polys = int(tables[1].shape[0]) - 1
    multi = int((np.diff(tables[2]) > 1).sum())
    lines = [
        "# Polygon ground truth to run lengths on the device",
        "",
        f"tools/bench_poly_rle.py: {args.images} images of {H} x {W}, {args.annotations} annotations, {polys} star-shaped polygons of 8 to 60 "
        f"vertices ({multi} annotations with 2 or 3 parts), {int(tables[1][-1])} vertices, {int(offsets[-1])} counts in all; {args.reps} "
        f"repetitions after {args.warmup} warm-up calls.  Stage rows: HIP events recorded between the stages of one ops.poly_rle call (xy "
        "already on the device); the wall-clock rows are around synchronised calls.",
        "",
        "| stage | ms |",
        "|---|---:|",
        f"| points pass: mi355det_poly_points_count, host read of the offsets, _emit | {ms['points']:.3f} |",
        f"| sort of the point keys (torch.sort, int64) | {ms['sort']:.3f} |",
        f"| events of the multi-part annotations: mi355det_poly_events + their sort | {ms['events']:.3f} |",
        f"| runs pass: mi355det_poly_runs_count, host read of the offsets, _emit (counts, area, bbox) | {ms['runs']:.3f} |",
        f"| **ops.poly_rle, first launch to last** | **{total:.3f}** |",
        f"| host: polygons.flatten of the annotation lists (validation, one float64 array), wall clock, once | {t_flatten:.1f} |",
        f"| dataset_to_rle end to end (flatten, upload, conversion, count lists), wall clock | {t_dataset:.1f} |",
        f"| ops.mask_rle_decode of one image's masks ({per_image} x {H} x {W}) | {t_decode:.3f} |",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
