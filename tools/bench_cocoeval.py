#!/usr/bin/env python3
"""COCO evaluation on the device at COCO-val size: 5000 images, 80 categories, about 36 000 ground truths, 100 detections per image,
synthetic boxes (most detections are jittered ground truths, the rest random), `bbox`.
    python tools/bench_cocoeval.py --reps 100 --warmup 5 --out profiles/r13_cocoeval.md
evaluate(), its two halves (the front end and IoU + match) and accumulate() are timed with HIP events after a warm-up and, because they end
in a host read, with the wall clock around synchronised calls as well; the kernels alone are timed on the grouped arrays evaluate() leaves
behind.  For context the numpy
restatement of the rules that the tests compare against (tests/cocoeval_oracle.py - the test oracle, not pycocotools) is timed on a
subset of the images.  Prints the markdown table and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = dict(images=5000, categories=80, ground_truths=36000, detections=100)             # the defaults below; tools/bench_tide.py uses them too


def device_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def synth(images, cats, gts, dets, seed):
    """-> dataset dict, and the detections as arrays (image id, category id, score, box)."""
    rng = np.random.RandomState(seed)
    g_img = np.sort(rng.randint(0, images, gts)) + 1
    g_cat = rng.randint(0, cats, gts) + 1
    side = np.exp(rng.uniform(np.log(8), np.log(300), (gts, 2)))
    g_box = np.concatenate([rng.rand(gts, 2) * 400, side], 1)
    crowd = rng.rand(gts) < 0.02
    anns = [{"id": j + 1, "image_id": int(g_img[j]), "category_id": int(g_cat[j]), "bbox": g_box[j].tolist(),
             "area": float(g_box[j, 2] * g_box[j, 3]), "iscrowd": int(crowd[j])} for j in range(gts)]
    dataset = {"images": [{"id": i + 1} for i in range(images)], "categories": [{"id": c + 1} for c in range(cats)], "annotations": anns}
    n = images * dets
    d_img = np.repeat(np.arange(images) + 1, dets)
    src = rng.randint(0, gts, n)                                  # 70 %: a ground truth of the same image, jittered; else random
    first = np.searchsorted(g_img, d_img, "left")
    count = np.searchsorted(g_img, d_img, "right") - first
    near = (rng.rand(n) < 0.7) & (count > 0)
    src = np.where(near, first + src % np.maximum(count, 1), src)
    d_box = np.where(near[:, None], g_box[src] * (1 + rng.randn(n, 4) * 0.08), np.concatenate([rng.rand(n, 2) * 400, side[src]], 1))
    d_box[:, 2:] = np.maximum(d_box[:, 2:], 1.0)
    d_cat = np.where(near & (rng.rand(n) < 0.9), g_cat[src], rng.randint(0, cats, n) + 1)
    d_score = rng.rand(n).astype(np.float32)
    return dataset, (d_img, d_cat, d_score, d_box.astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=SIZES["images"])
    ap.add_argument("--categories", type=int, default=SIZES["categories"])
    ap.add_argument("--ground-truths", type=int, default=SIZES["ground_truths"])
    ap.add_argument("--detections", type=int, default=SIZES["detections"], help="per image")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-images", type=int, default=100, help="images of the subset the numpy test oracle is timed on (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops
    from object_detectors_amd.cocoeval import COCOEval
    dev = torch.device("cuda:0")
    dataset, (d_img, d_cat, d_score, d_box) = synth(args.images, args.categories, args.ground_truths, args.detections, 0)
    e = COCOEval(dataset, "bbox", device=dev)
    e.add(torch.from_numpy(d_img).to(dev), torch.from_numpy(d_cat).to(dev), torch.from_numpy(d_score).to(dev), boxes=torch.from_numpy(d_box).to(dev))
    t_eval_dev = device_ms(e.evaluate, args.reps, args.warmup)
    t_eval = wall_ms(e.evaluate, args.reps, 0)
    t_front_dev = device_ms(e._group, args.reps, args.warmup)
    t_front = wall_ms(e._group, args.reps, 0)
    iou_size = e._group()
    t_im_dev = device_ms(lambda: e._match(iou_size), args.reps, args.warmup)
    t_im = wall_ms(lambda: e._match(iou_size), args.reps, 0)
    t_acc_dev = device_ms(e.accumulate, args.reps, args.warmup)
    t_acc = wall_ms(e.accumulate, args.reps, 0)
    e.summarize()
    # the kernels alone, on what evaluate() left
    thr = torch.from_numpy(np.ascontiguousarray(e.iou_thrs)).to(dev)
    rng = torch.from_numpy(np.ascontiguousarray(e.area_rng)).to(dev)
    rec = torch.from_numpy(np.ascontiguousarray(e.rec_thrs)).to(dev)
    t_iou = device_ms(lambda: ops.coco_iou(e.dt_offsets, e.gt_offsets, e.iou_offsets, iou_size, e.dt_boxes, e.gt_boxes, e.gt_crowd),
                      args.reps, args.warmup)
    t_match = device_ms(lambda: ops.coco_match(e.dt_offsets, e.gt_offsets, e.iou_offsets, e.iou, e.dt_area, e.gt_area, e.gt_flag, thr, rng),
                        args.reps, args.warmup)
    t_accum = device_ms(lambda: ops.coco_accumulate(e.cat_dt_offsets, e.cat_gt_offsets, e.order, e.dt_rank, e.dt_score, e.dt_match, e.dt_ignore,
                                                    e.gt_ignore, e.max_dets, rec), args.reps, args.warmup)
    lines = [
        "# COCO evaluation on the device at COCO-val size",
        "",
        f"tools/bench_cocoeval.py, `bbox`: {args.images} images, {args.categories} categories, {args.ground_truths} ground truths, "
        f"{args.detections} detections per image ({e.num_added} in all, {e.num_dt} after the cut to 100 per group), synthetic boxes; "
        f"{e.num_groups} (image, category) groups, {iou_size} IoU pairs.  {args.reps} repetitions after {args.warmup} warm-up calls.  "
        "Device column: HIP events around the calls; wall column: wall clock around synchronised calls.",
        "",
        "| section | device ms | wall ms |",
        "|---|---:|---:|",
        f"| **COCOEval.evaluate()** (grouping sorts, mi355det_coco_iou, mi355det_coco_match, one host read) | **{t_eval_dev:.3f}** | {t_eval:.3f} |",
        f"| front end (cut to 100 per group, grouping: torch sorts and searches, one host read) | {t_front_dev:.3f} | {t_front:.3f} |",
        f"| IoU + match (mi355det_coco_iou, mi355det_coco_match, output allocation) | {t_im_dev:.3f} | {t_im:.3f} |",
        f"| **COCOEval.accumulate()** (per-category sort, mi355det_coco_accumulate, results to the host) | **{t_acc_dev:.3f}** | {t_acc:.3f} |",
        f"| mi355det_coco_iou alone (output allocation included) | {t_iou:.3f} | |",
        f"| mi355det_coco_match alone (output allocation and zeroing included) | {t_match:.3f} | |",
        f"| mi355det_coco_accumulate alone (output allocation included) | {t_accum:.3f} | |",
        "",
        f"AP = {e.stats[0]:.4f}, AP50 = {e.stats[1]:.4f}, AR@100 = {e.stats[8]:.4f} on this synthetic set (they say nothing about a model).",
    ]
    if args.oracle_images > 0:
        from tests import cocoeval_oracle as co
        keep = set(range(1, args.oracle_images + 1))
        sub = dict(dataset, images=[im for im in dataset["images"] if im["id"] in keep],
                   annotations=[a for a in dataset["annotations"] if a["image_id"] in keep])
        m = d_img <= args.oracle_images
        rows = [{"image_id": int(i), "category_id": int(c), "score": float(s), "bbox": [float(v) for v in b]}
                for i, c, s, b in zip(d_img[m], d_cat[m], d_score[m], d_box[m])]
        t = time.perf_counter()
        ev = co.evaluate(sub, rows)
        t_o_eval = time.perf_counter() - t
        t = time.perf_counter()
        co.accumulate(ev)
        t_o_acc = time.perf_counter() - t
        lines += ["",
                  f"For context only: the numpy test oracle (tests/cocoeval_oracle.py, plain loops; not pycocotools, which is not installed) "
                  f"takes {t_o_eval:.2f} s to evaluate and {t_o_acc:.2f} s to accumulate a {args.oracle_images}-image subset of this set on one "
                  "CPU core."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
