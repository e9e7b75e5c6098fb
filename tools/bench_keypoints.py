#!/usr/bin/env python3
"""COCO keypoint evaluation (COCOEval(gt, "keypoints"), csrc/oks_kernels.hip) at person-keypoints-val size, on a synthetic set: 5000 images,
1 category, about 11 000 ground truths of which roughly 40 % have no labelled keypoint, 100 000 detections.
    python tools/bench_keypoints.py --reps 20 --warmup 3 --rounds 2 --out profiles/r28_keypoint_eval.md
The front end, coco_oks, keypoints_match, accumulate() and the whole of evaluate() are timed separately with HIP events after a warm-up.
Beside them, on the first --loop-images images, the route a user has without the kernels: the literal per-group host form the tests compare
against (tests/oks_oracle.py: computeOks as Python loops over pairs and keypoints, then the greedy match), one CPU core.  The routes alternate
within one process, --rounds times; the table shows every round, so the spread between two runs of the same code is on the page.  Prints the
markdown and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.bench_cocoeval import device_ms  # noqa: E402

SIZES = {"images": 5000, "ground_truths": 11000, "detections": 100000}
K = 17


def synth(images, ground_truths, detections, seed, blank=0.4):
    """-> (dataset dict, (image id [n], score [n], keypoints [n, K, 3]) as numpy).  People are boxes of 30..300 px in a 640 x 480 image;
    `blank` of them carry no labelled keypoint (num_keypoints 0, as about 40 % of person-keypoints annotations do), a few are crowds.  Two
    thirds of the detections are a ground truth of their image moved by a few per cent of its size, the rest lie anywhere."""
    rng = np.random.RandomState(seed)
    g_img = np.sort(rng.randint(1, images + 1, ground_truths))
    w, h = 30 + 270 * rng.rand(ground_truths), 30 + 270 * rng.rand(ground_truths)
    x, y = rng.rand(ground_truths) * (640 - w).clip(1), rng.rand(ground_truths) * (480 - h).clip(1)
    v = rng.randint(0, 3, (ground_truths, K))
    v[rng.rand(ground_truths) < blank] = 0
    kx, ky = x[:, None] + rng.rand(ground_truths, K) * w[:, None], y[:, None] + rng.rand(ground_truths, K) * h[:, None]
    kp = np.stack([np.where(v > 0, kx, 0.0), np.where(v > 0, ky, 0.0), v.astype(np.float64)], 2)
    crowd = rng.rand(ground_truths) < 0.02
    anns = [{"id": j + 1, "image_id": int(g_img[j]), "category_id": 1, "bbox": [float(x[j]), float(y[j]), float(w[j]), float(h[j])],
             "area": float(0.5 * w[j] * h[j]), "iscrowd": int(crowd[j]), "num_keypoints": int((v[j] > 0).sum()),
             "keypoints": kp[j].reshape(-1).tolist()} for j in range(ground_truths)]
    dataset = {"images": [{"id": i} for i in range(1, images + 1)], "categories": [{"id": 1}], "annotations": anns}
    src = rng.randint(0, ground_truths, detections)
    near = rng.rand(detections) < 2 / 3
    d_img = np.where(near, g_img[src], rng.randint(1, images + 1, detections)).astype(np.int64)
    s = (0.02 + 0.1 * rng.rand(detections)) * np.sqrt(0.5 * w[src] * h[src])
    jx = np.where(v[src] > 0, kx[src], x[src][:, None] + rng.rand(detections, K) * w[src][:, None]) + rng.randn(detections, K) * s[:, None]
    jy = np.where(v[src] > 0, ky[src], y[src][:, None] + rng.rand(detections, K) * h[src][:, None]) + rng.randn(detections, K) * s[:, None]
    far = np.stack([rng.rand(detections, K) * 640, rng.rand(detections, K) * 480], 2)
    d_kp = np.concatenate([np.where(near[:, None, None], np.stack([jx, jy], 2), far), np.ones((detections, K, 1))], 2)
    return dataset, (d_img, rng.rand(detections), d_kp)


def subset_rows(dataset, dets, images):
    d_img, d_score, d_kp = dets
    sub = dict(dataset, images=dataset["images"][:images], annotations=[a for a in dataset["annotations"] if a["image_id"] <= images])
    m = d_img <= images
    rows = [{"image_id": int(i), "category_id": 1, "score": float(s), "keypoints": kp.reshape(-1).tolist()}
            for i, s, kp in zip(d_img[m], d_score[m], d_kp[m])]
    return sub, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the set (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="how often the routes alternate; every round is reported")
    ap.add_argument("--loop-images", type=int, default=250, help="images the host form covers")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops
    from object_detectors_amd.cocoeval import COCOEval
    from tests import oks_oracle
    sizes = {k: max(1, int(v * args.scale)) for k, v in SIZES.items()}
    dev = torch.device("cuda:0")
    dataset, dets = synth(sizes["images"], sizes["ground_truths"], sizes["detections"], 0)
    d_img, d_score, d_kp = dets
    to = lambda a: torch.from_numpy(a).to(dev)
    ev = COCOEval(dataset, "keypoints", device=dev)
    ev.add(to(d_img), torch.ones(len(d_img), dtype=torch.int64, device=dev), to(d_score), keypoints=to(d_kp))
    ev.evaluate().accumulate()
    stats = ev.summarize(file=open(os.devnull, "w"))
    thr, rng_, _rec = ev._params()
    iou_size = int(ev.iou.shape[0])
    oks = lambda: ops.coco_oks(ev.dt_offsets, ev.gt_offsets, ev.iou_offsets, iou_size, ev.dt_kp, ev.gt_kp, ev.gt_boxes, ev.gt_area,
                               ev._ground_truth()["vars"])
    match = lambda: ops.keypoints_match(ev.dt_offsets, ev.gt_offsets, ev.iou_offsets, ev.iou, ev.dt_area, ev.gt_area, ev.gt_flag, ev.gt_crowd,
                                        thr, rng_)
    loop_images = min(args.loop_images, sizes["images"])
    sub, rows = subset_rows(dataset, dets, loop_images)
    rounds = []
    for _ in range(args.rounds):
        r = {"front": device_ms(ev._group, args.reps, args.warmup), "oks": device_ms(oks, args.reps, args.warmup),
             "match": device_ms(match, args.reps, args.warmup), "evaluate": device_ms(ev.evaluate, args.reps, args.warmup),
             "accumulate": device_ms(ev.accumulate, args.reps, args.warmup)}
        t0 = time.perf_counter()
        host = oks_oracle.evaluate(sub, rows)
        r["host"] = (time.perf_counter() - t0) * 1e3
        r["host_scaled"] = r["host"] * sizes["images"] / loop_images
        rounds.append(r)
    # the host form and the device agree on the images the host form covers
    I = len(ev.img_ids)
    keys = ev.group_keys.cpu().numpy()
    off = ev.iou_offsets.cpu().numpy()
    got = ev.iou.cpu().numpy()
    worst, pairs = 0.0, 0
    for (_k, i), g in host["groups"].items():
        j = int(np.searchsorted(keys, i))
        assert keys[j] == i and I == sizes["images"]
        worst = max(worst, float(np.abs(got[off[j]:off[j + 1]] - g["iou"].reshape(-1)).max()) if g["iou"].size else 0.0)
        pairs += g["iou"].size
    cols = " | ".join(f"round {j + 1}" for j in range(args.rounds))
    row = lambda label, key: f"| {label} | " + " | ".join(f"{r[key]:.3f}" for r in rounds) + " |"
    blank = sum(a["num_keypoints"] == 0 for a in dataset["annotations"])
    lines = [
        "# COCO keypoint evaluation on the device (COCOEval(gt, \"keypoints\"))",
        "",
        "tools/bench_keypoints.py.  All routes run in one process and alternate; a column is one round, so two columns of a row are two runs of "
        "the same code and their difference is the spread.  The workload is small and bound by launch and latency; no roofline is claimed.",
        "",
        "## person-keypoints-val size",
        "",
        f"{sizes['images']} images, 1 category, {sizes['ground_truths']} ground truths ({blank} without a labelled keypoint), "
        f"{sizes['detections']} detections, K = {K}, synthetic; {ev.num_dt} detection slots after the cut to 20 per image, {ev.num_groups} "
        f"groups, {iou_size} (detection, ground truth) pairs.  AP = {stats[0]:.4f}, AR = {stats[5]:.4f} (synthetic: they say nothing about a model).",
        "",
        f"| section (ms, HIP events, mean of {args.reps} calls after {args.warmup} warm-up calls) | {cols} |",
        "|---|" + "---:|" * args.rounds,
        row("front end: sorts, the cut to 20, area and box from the keypoints, the slot layout (one host read)", "front"),
        row("mi355det_coco_oks (output allocation included)", "oks"),
        row("mi355det_keypoints_match (output allocation included)", "match"),
        row("**evaluate()**: the three above", "evaluate"),
        row("accumulate() (per-category sort, mi355det_coco_accumulate, three arrays to the host)", "accumulate"),
        row(f"the literal host form (tests/oks_oracle.py: similarity and match, no accumulate), first {loop_images} images, one CPU core, wall clock",
            "host"),
        row(f"the same, scaled by {sizes['images']} / {loop_images} images", "host_scaled"),
        "",
        f"The host form covers {loop_images} of {sizes['images']} images ({pairs} pairs); its scaled row is an extrapolation, the device rows "
        f"cover the whole set.  On those images the largest difference between the device's similarities and the host form's is {worst:.3e}.",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
