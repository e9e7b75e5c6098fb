#!/usr/bin/env python3
"""LVIS evaluation on the device at LVIS-v1-val size: 19 809 images, 1203 categories (337 rare, 461 common, 405 frequent), 244 707 ground
truths, 300 detections per image, synthetic boxes (most detections are jittered ground truths of their image, the rest random), `bbox`.
    python tools/bench_lviseval.py --reps 20 --warmup 3 --out profiles/r14_lviseval.md
Three sections are timed apart, with HIP events after a warm-up and, because each ends in or next to a host read, with the wall clock around
synchronised calls as well: the front end (cut to 300 per image, federated filter, grouping: torch sorts and searches), IoU + match
(mi355det_coco_iou, mi355det_lvis_match) and accumulate().  The kernels alone are timed on the grouped arrays the front end leaves behind.
For context the numpy restatement of the rules that the tests compare against (tests/lviseval_oracle.py - the test oracle, not lvis-api)
is timed on a subset of the images.  Prints the markdown table and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_cocoeval import device_ms, wall_ms  # noqa: E402

SIZES = dict(images=19809, categories=1203, ground_truths=244707, detections=300)        # the defaults below; tools/bench_tide.py uses them too


def synth(images, cats, gts, dets, seed):
    """-> LVIS dataset dict, and the detections as arrays (image id, category id, score, box)."""
    rng = np.random.RandomState(seed)
    g_img = np.sort(rng.randint(0, images, gts)) + 1
    # a long tail: each image draws its ground truths from a few categories, frequent ones more often
    weight = 1.0 / (1.0 + np.arange(cats))[::-1]
    g_cat = rng.choice(cats, gts, p=weight / weight.sum()) + 1
    side = np.exp(rng.uniform(np.log(8), np.log(300), (gts, 2)))
    g_box = np.concatenate([rng.rand(gts, 2) * 400, side], 1)
    ignore = rng.rand(gts) < 0.01
    anns = [{"id": j + 1, "image_id": int(g_img[j]), "category_id": int(g_cat[j]), "bbox": g_box[j].tolist(),
             "area": float(g_box[j, 2] * g_box[j, 3])} for j in range(gts)]
    for j in np.flatnonzero(ignore):
        anns[j]["ignore"] = 1
    n_rare, n_common = (cats * 337) // 1203, (cats * 461) // 1203
    freq = ["r"] * n_rare + ["c"] * n_common + ["f"] * (cats - n_rare - n_common)
    positive = [set() for _ in range(images + 1)]
    for i, c in zip(g_img, g_cat):
        positive[i].add(int(c))
    imgs = []
    for i in range(1, images + 1):
        neg = [int(c) for c in rng.randint(0, cats, 6) + 1 if int(c) not in positive[i]]
        nel = [c for c in sorted(positive[i]) if rng.rand() < 0.1]
        imgs.append({"id": i, "neg_category_ids": sorted(set(neg)), "not_exhaustive_category_ids": nel})
    dataset = {"images": imgs, "categories": [{"id": c + 1, "frequency": freq[c]} for c in range(cats)], "annotations": anns}
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
    ap.add_argument("--oracle-images", type=int, default=50, help="images of the subset the numpy test oracle is timed on (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops
    from object_detectors_amd.lviseval import NO_CUT, LVISEval
    dev = torch.device("cuda:0")
    dataset, (d_img, d_cat, d_score, d_box) = synth(args.images, args.categories, args.ground_truths, args.detections, 0)
    e = LVISEval(dataset, device=dev)
    e.add(torch.from_numpy(d_img).to(dev), torch.from_numpy(d_cat).to(dev), torch.from_numpy(d_score).to(dev), torch.from_numpy(d_box).to(dev))
    t_front_dev = device_ms(e._group, args.reps, args.warmup)      # the host-side sort of the annotations happens once, in the warm-up
    t_front = wall_ms(e._group, args.reps, 0)
    iou_size = e._group()
    t_match_dev = device_ms(lambda: e._match(iou_size), args.reps, args.warmup)
    t_match = wall_ms(lambda: e._match(iou_size), args.reps, 0)
    t_acc_dev = device_ms(e.accumulate, args.reps, args.warmup)
    t_acc = wall_ms(e.accumulate, args.reps, 0)
    t_eval = wall_ms(e.evaluate, args.reps, 0)
    res = e.summarize()
    # the kernels alone, on what the front end left
    thr =torch.from_numpy(np.ascontiguousarray(e.iou_thrs)).to(dev)
    rng = torch.from_numpy(np.ascontiguousarray(e.area_rng)).to(dev)
    rec = torch.from_numpy(np.ascontiguousarray(e.rec_thrs)).to(dev)
    t_iou_k = device_ms(lambda: ops.coco_iou(e.dt_offsets, e.gt_offsets, e.iou_offsets, iou_size, e.dt_boxes, e.gt_boxes, e.gt_crowd),
                        args.reps, args.warmup)
    t_match_k = device_ms(lambda: ops.lvis_match(e.dt_offsets, e.gt_offsets, e.iou_offsets, e.iou, e.dt_area, e.gt_area, e.gt_flag,
                                                 e.group_not_exhaustive, thr, rng), args.reps, args.warmup)
    t_accum_k = device_ms(lambda: ops.coco_accumulate(e.cat_dt_offsets, e.cat_gt_offsets, e.order, e.dt_rank, e.dt_score, e.dt_match, e.dt_ignore,
                                                      e.gt_ignore, [NO_CUT], rec), args.reps, args.warmup)
    lines = [
        "# LVIS evaluation on the device at LVIS-v1-val size",
        "",
        f"tools/bench_lviseval.py, `bbox`: {args.images} images, {args.categories} categories, {args.ground_truths} ground truths, "
        f"{args.detections} detections per image ({e.num_added} in all, {e.num_dt} after the cut to 300 per image and the federated filter), "
        f"synthetic boxes; {e.num_groups} (image, category) groups, {iou_size} IoU pairs.  {args.reps} repetitions after {args.warmup} warm-up "
        "calls.  Device column: HIP events around the calls; wall column: wall clock around synchronised calls.",
        "",
        "| section | device ms | wall ms |",
        "|---|---:|---:|",
        f"| **front end** (cut, federated filter, grouping: torch sorts and searches, one host read) | **{t_front_dev:.3f}** | {t_front:.3f} |",
        f"| **IoU + match** (mi355det_coco_iou, mi355det_lvis_match, output allocation) | **{t_match_dev:.3f}** | {t_match:.3f} |",
        f"| **LVISEval.accumulate()** (per-category sort, mi355det_coco_accumulate, results to the host) | **{t_acc_dev:.3f}** | {t_acc:.3f} |",
        f"| LVISEval.evaluate() = front end + IoU + match | | {t_eval:.3f} |",
        f"| mi355det_coco_iou alone (output allocation included) | {t_iou_k:.3f} | |",
        f"| mi355det_lvis_match alone (output allocation and zeroing included) | {t_match_k:.3f} | |",
        f"| mi355det_coco_accumulate alone (output allocation included) | {t_accum_k:.3f} | |",
        "",
        f"AP = {res['AP']:.4f}, APr = {res['APr']:.4f}, APc = {res['APc']:.4f}, APf = {res['APf']:.4f}, AR@300 = {res['AR@300']:.4f} on this "
        "synthetic set (they say nothing about a model).",
    ]
    if args.oracle_images > 0:
        from tests import lviseval_oracle as lo
        keep = set(range(1, args.oracle_images + 1))
        sub = dict(dataset, images=[im for im in dataset["images"] if im["id"] in keep],
                   annotations=[a for a in dataset["annotations"] if a["image_id"] in keep])
        m = d_img <= args.oracle_images
        rows = [{"image_id": int(i), "category_id": int(c), "score": float(s), "bbox": [float(v) for v in b]}
                for i, c, s, b in zip(d_img[m], d_cat[m], d_score[m], d_box[m])]
        t = time.perf_counter()
        ev = lo.evaluate(sub, rows)
        t_o_eval = time.perf_counter() - t
        t = time.perf_counter()
        lo.accumulate(ev)
        t_o_acc = time.perf_counter() - t
        lines += ["",
                  f"For context only: the numpy test oracle (tests/lviseval_oracle.py, plain loops; not lvis-api, which is not installed) "
                  f"takes {t_o_eval:.2f} s to evaluate and {t_o_acc:.2f} s to accumulate a {args.oracle_images}-image subset of this set on one "
                  "CPU core."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
