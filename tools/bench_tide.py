#!/usr/bin/env python3
"""The error breakdown (object_detectors_amd/tide.py) at COCO-val and LVIS-v1-val size, on the synthetic sets of tools/bench_cocoeval.py and
tools/bench_lviseval.py.
    python tools/bench_tide.py --sets coco lvis --reps 20 --warmup 3 --rounds 2 --out profiles/r21_tide.md
The five sections of ErrorBreakdown.run() - front end, tide_classify, tide_fixes and the two accumulate calls - are timed separately with
HIP events after a warm-up.  Beside them, on the first --loop-images images, the two routes a user has without the kernels: the same
classification as a per-image loop of torch ops on the device, and the literal host form the tests compare against (tests/tide_oracle.py,
plain Python loops).  The routes alternate within one process, --rounds times; the table shows every round, so the spread between two runs
of the same code is on the page.  Prints the markdown and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools import bench_cocoeval, bench_lviseval  # noqa: E402
from tools.bench_cocoeval import device_ms  # noqa: E402


def torch_loop(b, f, images, fg, bg):
    """tide_classify's kinds, image by image, with torch ops on the device: what one writes without the kernel.  -> kind uint8 [num_dt] (the
    slots of the other images stay 0)."""
    ev = b.ev
    dt_off, dt_slots, gt_off, gt_slots = f["view"]
    dt_off, gt_off = dt_off.tolist(), gt_off.tolist()
    kind = torch.zeros(int(ev.num_dt), dtype=torch.uint8, device=ev.device)
    for i in range(images):
        d = dt_slots[dt_off[i]:dt_off[i + 1]]
        d = d[f["dt_fp"][d] != 0]
        g = gt_slots[gt_off[i]:gt_off[i + 1]]
        g = g[f["gt_counted"][g] != 0]
        db, gb = ev.dt_boxes[d], f["gt_box"][g]
        w = torch.minimum((db[:, 0] + db[:, 2])[:, None], (gb[:, 0] + gb[:, 2])[None]) - torch.maximum(db[:, 0][:, None], gb[:, 0][None])
        h = torch.minimum((db[:, 1] + db[:, 3])[:, None], (gb[:, 1] + gb[:, 3])[None]) - torch.maximum(db[:, 1][:, None], gb[:, 1][None])
        inter = w * h
        iou = torch.where((w > 0) & (h > 0), inter / ((db[:, 2] * db[:, 3])[:, None] + (gb[:, 2] * gb[:, 3])[None] - inter), torch.zeros_like(inter))
        same = f["dt_cat"][d][:, None] == f["gt_cat"][g][None]
        zero = torch.zeros((int(d.shape[0]), 1), dtype=iou.dtype, device=iou.device)
        s = torch.cat([torch.where(same, iou, torch.zeros_like(iou)), zero], 1).max(1).values
        o = torch.cat([torch.where(same, torch.zeros_like(iou), iou), zero], 1).max(1).values
        k = torch.full_like(s, 3, dtype=torch.uint8)
        k = torch.where(torch.maximum(s, o) <= bg, torch.full_like(k, 5), k)
        k = torch.where(s >= fg, torch.full_like(k, 4), k)
        k = torch.where(o >= fg, torch.full_like(k, 1), k)
        k = torch.where((s >= bg) & (s < fg), torch.full_like(k, 2), k)
        kind[d] = k
    return kind


def subset_rows(dataset, dets, images):
    d_img, d_cat, d_score, d_box = dets
    keep = set(range(1, images + 1))
    sub = dict(dataset, images=[im for im in dataset["images"] if im["id"] in keep],
               annotations=[a for a in dataset["annotations"] if a["image_id"] in keep])
    m = d_img <= images
    rows = [{"image_id": int(i), "category_id": int(c), "score": float(s), "bbox": [float(v) for v in bx]}
            for i, c, s, bx in zip(d_img[m], d_cat[m], d_score[m], d_box[m])]
    return sub, rows


def bench_set(name, args):
    from object_detectors_amd.tide import ErrorBreakdown
    lvis = name == "lvis"
    mod = bench_lviseval if lvis else bench_cocoeval
    sizes = dict(mod.SIZES)
    if args.scale != 1.0:
        sizes = {k: (v if k in ("categories", "detections") else max(1, int(v * args.scale))) for k, v in sizes.items()}
    dev = torch.device("cuda:0")
    dataset, dets = mod.synth(sizes["images"], sizes["categories"], sizes["ground_truths"], sizes["detections"], 0)
    d_img, d_cat, d_score, d_box = dets
    to = lambda a: torch.from_numpy(a).to(dev)
    if lvis:
        from object_detectors_amd.lviseval import LVISEval
        ev = LVISEval(dataset, device=dev)
        ev.add(to(d_img), to(d_cat), to(d_score), to(d_box))
    else:
        from object_detectors_amd.cocoeval import COCOEval
        ev = COCOEval(dataset, "bbox", device=dev)
        ev.add(to(d_img), to(d_cat), to(d_score), boxes=to(d_box))
    ev.evaluate()
    b = ErrorBreakdown(ev)
    res = b.run()
    fg, bg, t = 0.5, 0.1, int(np.flatnonzero(np.isclose(ev.iou_thrs, 0.5))[0])
    rec = torch.from_numpy(np.ascontiguousarray(ev.rec_thrs, np.float64)).to(dev)
    f = b._front_end(t)
    loop_images = min(args.loop_images, sizes["images"])
    counted = f["gt_counted"] != 0
    pairs = int((torch.bincount(ev.dt_image.to(torch.int64)[f["dt_fp"] != 0], minlength=len(ev.img_ids)) *
                 torch.bincount(ev.gt_image.to(torch.int64)[counted], minlength=len(ev.img_ids))).sum())
    sub, rows = subset_rows(dataset, dets, loop_images) if args.oracle else (None, None)
    oracle_ev = None
    if args.oracle:
        from tests import cocoeval_oracle, lviseval_oracle, tide_oracle
        t0 = time.perf_counter()
        oracle_ev = (lviseval_oracle if lvis else cocoeval_oracle).evaluate(sub, rows)
        t_oracle_eval = time.perf_counter() - t0
    rounds = []
    for _ in range(args.rounds):
        r = {"front": device_ms(lambda: b._front_end(t), args.reps, args.warmup),
             "classify": device_ms(lambda: b._classify(f, fg, bg), args.reps, args.warmup),
             "fixes": device_ms(lambda: b._fixes(f), args.reps, args.warmup),
             "acc8": device_ms(lambda: b._price_in_place(rec), args.reps, args.warmup),
             "acc_cls": device_ms(lambda: b._price_cls(f, rec), args.reps, args.warmup),
             "run": device_ms(b.run, args.reps, args.warmup),
             "loop": device_ms(lambda: torch_loop(b, f, loop_images, fg, bg), 1, 1 if not rounds else 0)}
        if args.oracle:
            t0 = time.perf_counter()
            an = tide_oracle.analyse(sub, rows, lvis=lvis, ev=oracle_ev, prices=False)
            r["oracle"] = (time.perf_counter() - t0) * 1e3
        rounds.append(r)
    # the loop and the kernel name the same kinds on the images the loop covers
    first = ev.dt_image.to(torch.int64) < loop_images
    same_kinds = bool(torch.equal(torch_loop(b, f, loop_images, fg, bg)[first], b.kind[first]))
    if args.oracle:
        n = len(an["kind"])
        assert n == int(first.sum()), (n, int(first.sum()))
    title = "LVIS-v1-val" if lvis else "COCO-val"
    cols = " | ".join(f"round {j + 1}" for j in range(args.rounds))
    row = lambda label, key: f"| {label} | " + " | ".join(f"{r[key]:.3f}" for r in rounds) + " |"
    lines = [
        f"## {title} size",
        "",
        f"{sizes['images']} images, {sizes['categories']} categories, {sizes['ground_truths']} ground truths, {sizes['detections']} detections per "
        f"image, synthetic boxes (tools/bench_{'lvis' if lvis else 'coco'}eval.py); {ev.num_dt} kept detection slots, {int(f['dt_fp'].sum())} of them "
        f"false positives at IoU 0.5; {int(counted.sum())} counted ground truths; {pairs} (false positive, counted ground truth) pairs, the "
        f"overlaps tide_classify computes.  AP50 = {res['ap_base']:.4f}; counts Cls, Loc, Both, Dupe, Bkg, Miss = {res['counts'][:6].tolist()} "
        "(synthetic: they say nothing about a model).",
        "",
        f"| section (ms, HIP events, mean of {args.reps} calls after {args.warmup} warm-up calls) | {cols} |",
        "|---|" + "---:|" * args.rounds,
        row("front end: the image-major view (torch sorts), categories, flags", "front"),
        row("mi355det_tide_classify (output allocation included)", "classify"),
        row("mi355det_tide_fixes (output allocation included)", "fixes"),
        row("coco_accumulate, base + seven fixes as 8 area ranges (with its per-category sort)", "acc8"),
        row("coco_accumulate, the Cls fix (with the re-sort of the slots by their new categories)", "acc_cls"),
        row("**ErrorBreakdown.run()**, all of the above and the tables on the host", "run"),
        row(f"the classification as a per-image loop of torch ops on the device, first {loop_images} images, one pass", "loop"),
    ]
    if args.oracle:
        lines.append(row(f"the literal host form (tests/tide_oracle.py, classification and flags only), the same {loop_images} images, one CPU core",
                         "oracle"))
    lines += ["",
              f"The loop names the same kinds as the kernel on its {loop_images} images: {same_kinds}.  The loop and the host form cover "
              f"{loop_images} of {sizes['images']} images; tide_classify's row covers all of them."]
    if args.oracle:
        lines.append(f"The host form starts from the match output of the numpy restatement of the evaluator, which took {t_oracle_eval:.1f} s "
                     f"for those {loop_images} images and is not in its row.")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["coco", "lvis"], choices=["coco", "lvis"])
    ap.add_argument("--scale", type=float, default=1.0, help="shrink the image and ground-truth counts (a rehearsal, not a measurement)")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2, help="how often the routes alternate; every round is reported")
    ap.add_argument("--loop-images", type=int, default=500, help="images the torch loop and the host form cover")
    ap.add_argument("--no-oracle", dest="oracle", action="store_false", help="skip the host form")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = ["# Error breakdown of AP50 on the device (object_detectors_amd/tide.py)",
             "",
             "tools/bench_tide.py.  All routes run in one process and alternate; a column is one round, so two columns of a row are two runs of "
             "the same code and their difference is the spread.  No ratio is claimed between rows that cover different numbers of images.",
             ""]
    for name in args.sets:
        lines += bench_set(name, args) + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
