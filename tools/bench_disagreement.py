#!/usr/bin/env python3
"""The model comparison on the device at validation-set sizes, synthetic boxes (most detections are jittered ground truths, the rest random):
    coco   5000 images, 36 000 ground truths, 2 x 500 000 detections (100 per image), 80 categories
    lvis   19 809 images, 244 707 ground truths, 2 x 5 942 700 detections (300 per image, max_dets = 300), 1203 categories
    python tools/bench_disagreement.py --reps 20 --warmup 3 --out profiles/r17_model_compare.md
Disagreement.run() is timed with HIP events after a warm-up and, because it ends in a host read, with the wall clock around synchronised
calls as well; its three parts (the torch filters and sorts, mi355det_box_disagreement, the sums) are timed alone with HIP events.  For
context the notebook's own loop - per image a box IoU call on the device (ops.box_iou, float32), max over the detections, Python sets - is
timed on a subset of the images with the wall clock.  Prints the markdown report and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"coco": dict(images=5000, gts=36000, dets=100, cats=80, max_dets=None),
         "lvis": dict(images=19809, gts=244707, dets=300, cats=1203, max_dets=300)}


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


def synth(images, gts, dets, cats, seed):
    """-> ground truth (image id, category id, box) and two detection sets (image id, category id, score, box) as arrays; boxes [x, y, w, h]."""
    rng = np.random.RandomState(seed)
    g_img = np.sort(rng.randint(0, images, gts)) + 1
    g_cat = rng.randint(0, cats, gts) + 1
    side = np.exp(rng.uniform(np.log(8), np.log(300), (gts, 2)))
    g_box = np.concatenate([rng.rand(gts, 2) * 400, side], 1)
    n = images * dets
    d_img = np.repeat(np.arange(images) + 1, dets)
    first = np.searchsorted(g_img, d_img, "left")
    count = np.searchsorted(g_img, d_img, "right") - first
    models = []
    for _m in range(2):
        src = rng.randint(0, gts, n)                              # 70 %: a ground truth of the same image, jittered; else random
        near = (rng.rand(n) < 0.7) & (count > 0)
        src = np.where(near, first + src % np.maximum(count, 1), src)
        d_box = np.where(near[:, None], g_box[src] * (1 + rng.randn(n, 4) * 0.08), np.concatenate([rng.rand(n, 2) * 400, side[src]], 1))
        d_box[:, 2:] = np.maximum(d_box[:, 2:], 1.0)
        d_cat = np.where(near & (rng.rand(n) < 0.8), g_cat[src], rng.randint(0, cats, n) + 1)
        order = rng.permutation(n)                                # results files are not grouped by image
        models.append((d_img[order], d_cat[order], rng.rand(n).astype(np.float32), d_box[order].astype(np.float32)))
    return (g_img, g_cat, g_box), models


def literal_loop(gt, models, image_ids, thr, conf, dev):
    """The notebook's loop on the device for the given images -> (counts, seconds).  Detections are grouped per image beforehand (not timed),
    as COCO.loadRes does when it builds its index."""
    from object_detectors_amd import ops
    g_img, g_cat, g_box = gt
    xyxy = lambda b: torch.cat([b[:, :2], b[:, :2] + b[:, 2:]], 1)
    per = []
    for img in image_ids:
        sel = g_img == img
        row = [(xyxy(torch.from_numpy(g_box[sel]).to(dev)), torch.from_numpy(g_cat[sel]).to(dev))]
        for d_img, d_cat, d_score, d_box in models:
            s = d_img == img
            row.append((xyxy(torch.from_numpy(d_box[s]).to(dev)), torch.from_numpy(d_cat[s]).to(dev), torch.from_numpy(d_score[s]).to(dev)))
        per.append(row)
    torch.cuda.synchronize()
    yes_yes = yes_no = no_yes = no_no = missed = 0
    t = time.perf_counter()
    for (g, gl), *sides in per:
        try:
            if g.shape[0] == 0:
                raise IndexError("no annotation")              # the notebook's convert_gt_to_numpy on an empty list
            lists = []
            for b, l, s in sides:
                keep = s > conf
                b, l = b[keep], l[keep]
                iou = ops.box_iou(b, g)
                values, indices = iou.max(dim=0)
                mask = values >= thr
                correct = gl[mask] == l[indices[mask]]
                lists.append(torch.arange(g.shape[0], device=dev)[mask][correct].tolist())
            a, b = set(lists[0]), set(lists[1])
            yes_no += len(a - b)
            no_yes += len(b - a)
            yes_yes += len(a & b)
            no_no += g.shape[0] - len(a | b)
        except IndexError:                                      # max over no detections
            missed += 1
    torch.cuda.synchronize()
    return (yes_yes, yes_no, no_yes, no_no, missed), time.perf_counter() - t


def bench(name, args, dev):
    from object_detectors_amd import ops
    from object_detectors_amd.compare import Disagreement
    cfg = SIZES[name]
    gt, models = synth(cfg["images"], cfg["gts"], cfg["dets"], cfg["cats"], 0)
    g_img, g_cat, g_box = gt
    dataset = {"images": [{"id": i + 1} for i in range(cfg["images"])], "categories": [{"id": c + 1} for c in range(cfg["cats"])],
               "annotations": [{"id": j + 1, "image_id": int(g_img[j]), "category_id": int(g_cat[j]), "bbox": g_box[j].tolist()}
                               for j in range(cfg["gts"])]}
    d = Disagreement(dataset, device=dev, max_dets=cfg["max_dets"])
    for m, (d_img, d_cat, d_score, d_box) in enumerate(models):
        d.add(m, torch.from_numpy(d_img).to(dev), torch.from_numpy(d_cat).to(dev), torch.from_numpy(d_score).to(dev), torch.from_numpy(d_box).to(dev))
    thr, conf = args.iou_threshold, args.confidence
    run = lambda: d.run(thr, conf)
    t_run_dev = device_ms(run, args.reps, args.warmup)
    t_run = wall_ms(run, args.reps, 0)
    r = d.run(thr, conf)
    a, b = d._kept(d._det[0], conf), d._kept(d._det[1], conf)
    t_front = device_ms(lambda: (d._kept(d._det[0], conf), d._kept(d._det[1], conf)), args.reps, args.warmup)
    t_kernel = device_ms(lambda: ops.box_disagreement(d.gt_offsets, d.gt_box, d.gt_label, a[:3], b[:3], thr), args.reps, args.warmup)
    t_sums = device_ms(lambda: d._tally(a[3], b[3]), args.reps, args.warmup)
    kept = int(a[1].shape[0]) + int(b[1].shape[0])
    pairs = int((d.gt_count * (a[3] + b[3])).sum())
    stat, p = d.report(file=open(os.devnull, "w"))
    lines = [
        f"## {name}: {cfg['images']} images, {cfg['gts']} ground truths, 2 x {cfg['images'] * cfg['dets']} detections"
        + (f", max_dets = {cfg['max_dets']}" if cfg["max_dets"] else ""),
        "",
        f"{kept} detections kept (score > {conf}), {pairs} (ground truth, detection) pairs.  Table: yes_yes {r['yes_yes']}, yes_no {r['yes_no']}, "
        f"no_yes {r['no_yes']}, no_no {r['no_no']}, total {r['total']}, missed {r['missed']}; McNemar statistic {stat:.4f}, p = {p:.4g} "
        "(synthetic boxes: it says nothing about a model).",
        "",
        "| section | device ms | wall ms |",
        "|---|---:|---:|",
        f"| **Disagreement.run()** (filters and sorts, mi355det_box_disagreement, sums, one host read) | **{t_run_dev:.3f}** | {t_run:.3f} |",
        f"| front end alone: both models' confidence filter, image sort" + (", score sort and cut" if cfg["max_dets"] else "") + f", offsets | {t_front:.3f} | |",
        f"| mi355det_box_disagreement alone (output allocation included) | {t_kernel:.3f} | |",
        f"| the sums alone (no host read) | {t_sums:.3f} | |",
        "",
        f"Kernel alone: {pairs / t_kernel / 1e6:.2f} G pairs/s.",
    ]
    if args.loop_images > 0:
        ids = list(range(1, args.loop_images + 1))
        literal_loop(gt, models, ids[:20], thr, conf, dev)                      # warm-up
        counts, secs = literal_loop(gt, models, ids, thr, conf, dev)
        sub = Disagreement(dict(dataset, images=[{"id": i} for i in ids], annotations=[x for x in dataset["annotations"] if x["image_id"] <= ids[-1]]),
                           device=dev, max_dets=cfg["max_dets"])
        for m, (d_img, d_cat, d_score, d_box) in enumerate(models):
            s = d_img <= ids[-1]
            sub.add(m, torch.from_numpy(d_img[s]).to(dev), torch.from_numpy(d_cat[s]).to(dev), torch.from_numpy(d_score[s]).to(dev),
                    torch.from_numpy(d_box[s]).to(dev))
        t_sub = wall_ms(lambda: sub.run(thr, conf), args.reps, args.warmup)
        rs = sub.run(thr, conf)
        lines += ["",
                  f"For context: the notebook's loop on the device (per image and model one ops.box_iou call in float32, max over the detections, "
                  f"Python sets; the per-image grouping not timed) takes {secs * 1e3:.1f} ms wall for the first {args.loop_images} images "
                  f"(table {counts[:4]}, missed {counts[4]}); Disagreement.run() on the same {args.loop_images} images takes {t_sub:.3f} ms wall "
                  f"(table {(rs['yes_yes'], rs['yes_no'], rs['no_yes'], rs['no_no'])}, missed {rs['missed']}; float64, so single instances at "
                  "the threshold may fall the other way)."]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["coco", "lvis"], choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iou_threshold", type=float, default=0.5)
    ap.add_argument("--confidence", type=float, default=0.0)
    ap.add_argument("--loop-images", type=int, default=500, help="images of the subset the notebook's per-image loop is timed on (0: skip)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_disagreement.py needs the GPU"
    dev = torch.device("cuda:0")
    lines = ["# Model comparison on the device at validation-set sizes", "",
             f"tools/bench_disagreement.py: synthetic boxes (70 % of the detections are jittered ground truths "
             f"of their image, the rest random), IoU threshold {args.iou_threshold}, confidence {args.confidence}.  {args.reps} repetitions after "
             f"{args.warmup} warm-up calls, one process, one run.  Device column: HIP events around the calls; wall column: wall clock around "
             "synchronised calls.", ""]
    for name in args.sizes:
        lines += bench(name, args, dev) + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
