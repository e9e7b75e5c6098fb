#!/usr/bin/env python3
"""Weighted boxes fusion on the device at validation-set sizes.  Two synthetic models, both made by jittering one detection set (a model
keeps a detection of the set with probability 0.85, moves its box by a few percent and draws its own score):
    coco   5000 images, 80 categories, 2 x up to 500 000 detections (100 per image in the set)
    lvis   19 809 images, 1203 categories, 2 x up to 5 942 700 detections (300 per image in the set)
    python tools/bench_fusion.py --reps 10 --warmup 2 --rounds 2 --host-images 200 --out profiles/r29_box_fusion.md
WeightedBoxesFusion.run() and its three parts (front end, mi355det_wbf_fuse, compaction) are timed with HIP events after a warm-up, run() with
the wall clock as well, since it ends in a host read.  For context the literal host form (tests/wbf_oracle.py: numpy float64, member lists, one
CPU core) is timed on the first --host-images images and SCALED by the number of images; the row says so.  All routes run in one process and
alternate: a column of the table is one round.  --cut-offsets adds a row: the kernel with the offsets table cut behind the last real group
(the front end's table has one group per candidate, because run() sizes nothing on the host before the launch; the row says what the
empty groups behind the last real one cost).  Prints the markdown report and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"coco": dict(images=5000, dets=100, cats=80), "lvis": dict(images=19809, dets=300, cats=1203)}


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


def wall_ms(fn, reps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def synth(images, dets, cats, seed):
    """-> two models as (image id, category id, score float32, box float32 [x, y, w, h]) arrays.  The set: per image `dets` boxes in a few
    categories of that image, so that a group holds several objects."""
    rng = np.random.RandomState(seed)
    n = images * dets
    img = np.repeat(np.arange(images) + 1, dets)
    per_image = rng.randint(0, cats, (images, 8))                   # an image shows up to 8 categories
    cat = per_image[img - 1, rng.randint(0, 8, n)] + 1
    box = np.concatenate([rng.rand(n, 2) * 500, np.exp(rng.uniform(np.log(8), np.log(300), (n, 2)))], 1)
    models = []
    for _m in range(2):
        keep = rng.rand(n) < .85
        k = int(keep.sum())
        b = box[keep] * (1 + rng.randn(k, 4) * .03)
        b[:, 2:] = np.maximum(b[:, 2:], 1.0)
        order = rng.permutation(k)                                  # a results file is not grouped
        models.append((img[keep][order], cat[keep][order], (rng.randint(1, 1000, k) / 1000).astype(np.float32)[order], b[order].astype(np.float32)))
    return models


def host_form(models, image_count, kw):
    """tests/wbf_oracle.fuse on the detections of the first `image_count` images -> (fused detections, seconds)."""
    from tests import wbf_oracle
    rows = [[{"image_id": int(i), "category_id": int(c), "score": float(s), "bbox": [float(v) for v in b]}
             for i, c, s, b in zip(*(a[m[0] <= image_count] for a in m))] for m in models]
    t = time.perf_counter()
    out = wbf_oracle.fuse(rows, list(range(1, image_count + 1)), **kw)
    return out, time.perf_counter() - t


def bench(name, args, dev):
    from object_detectors_amd import ops
    from object_detectors_amd.ensemble import WeightedBoxesFusion
    cfg = SIZES[name]
    models = synth(cfg["images"], cfg["dets"], cfg["cats"], 0)
    kw = dict(iou_thr=args.iou_thr, conf_type=args.conf_type)
    f = WeightedBoxesFusion(list(range(1, cfg["images"] + 1)), device=dev, weights=(1, 1), **kw)
    for m, (d_img, d_cat, d_score, d_box) in enumerate(models):
        f.add(m, torch.from_numpy(d_img).to(dev), torch.from_numpy(d_cat).to(dev), torch.from_numpy(d_score).to(dev), torch.from_numpy(d_box).to(dev))
    r = f.run()
    fr = f._front()
    out = f._kernel(fr)
    members = r["members"]
    groups = int((fr["offsets"][1:] > fr["offsets"][:-1]).sum())
    sizes = (fr["offsets"][1:] - fr["offsets"][:-1])
    cut = fr["offsets"][:groups + 1].contiguous()                   # the real groups come first
    rows = {k: [] for k in ("run", "wall", "front", "kernel", "cut", "finish", "host")}
    sub = None
    for _round in range(args.rounds):
        rows["run"].append(device_ms(f.run, args.reps, args.warmup))
        rows["wall"].append(wall_ms(f.run, args.reps))
        rows["front"].append(device_ms(f._front, args.reps, args.warmup))
        rows["kernel"].append(device_ms(lambda: f._kernel(fr), args.reps, args.warmup))
        if args.cut_offsets:
            rows["cut"].append(device_ms(lambda: ops.wbf_fuse(cut, fr["boxes"], fr["scores"], f.iou_thr, f.conf_type, f.weight_sum, f.weight_max),
                                         args.reps, args.warmup))
        rows["finish"].append(device_ms(lambda: f._finish(fr, out), args.reps, args.warmup))
        if args.host_images > 0:
            sub, secs = host_form(models, args.host_images, dict(kw, weights=(1, 1)))
            rows["host"].append(secs * 1e3 * cfg["images"] / args.host_images)
    same = "not checked"
    if sub is not None:                                             # the first images of the device result against the host form, bit for bit
        k = int((r["image_id"] <= args.host_images).sum())
        bits = lambda x: np.ascontiguousarray(x, np.float64).view(np.int64)
        same = str(k == len(sub["score"]) and np.array_equal(bits(r["score"][:k].cpu().numpy()), bits(sub["score"]))
                   and np.array_equal(bits(r["box"][:k].cpu().numpy()), bits(sub["box"])))
    cols = "".join(f" round {k + 1} |" for k in range(args.rounds))
    line = lambda label, key, fmt="{:.3f}": f"| {label} |" + "".join(" " + fmt.format(v) + " |" for v in rows[key])
    n = int(fr["n"])
    lines = [
        f"## {name}: {cfg['images']} images, {cfg['cats']} categories, 2 models x {cfg['images'] * cfg['dets']} detections in the set", "",
        f"{n} detections added ({' + '.join(str(len(m[0])) for m in models)}), dropped {r['dropped']}; {groups} (image, category) groups, the "
        f"largest of {int(sizes.max())} candidates; {int(members.shape[0])} fused detections, {int((members > 1).sum())} of them with more than "
        f"one member, the largest cluster of {int(members.max())}.  iou_thr {args.iou_thr}, conf_type {args.conf_type}, weights (1, 1).", "",
        f"| section (ms; HIP events, mean of {args.reps} calls after {args.warmup} warm-up calls, unless the row says otherwise) |{cols}",
        "|---|" + "---:|" * args.rounds,
        line("**WeightedBoxesFusion.run()** (front end, kernel, compaction, one host read)", "run", "**{:.3f}**"),
        line("run(), wall clock around synchronised calls", "wall"),
        line("front end alone: filter, weigh, three stable sorts, group offsets", "front"),
        line("mi355det_wbf_fuse alone (output allocation included)", "kernel"),
        line("compaction alone: founders, output order, cluster_of (with its host read)", "finish"),
    ]
    if args.cut_offsets:
        lines.insert(-1, line(f"mi355det_wbf_fuse with the offsets table cut on the host to the {groups} real groups (of {n} in the table; not "
                              "part of run())", "cut"))
    if args.host_images > 0:
        lines += [line(f"the literal host form (tests/wbf_oracle.py, one CPU core), measured on the first {args.host_images} images and SCALED by "
                       f"{cfg['images']}/{args.host_images}", "host", "{:.0f}"), "",
                  f"The device result on those {args.host_images} images has the bits of the host form: {same}."]
    lines += ["", f"Kernel alone: {n / np.mean(rows['kernel']) / 1e3:.1f} M candidates/s, {groups / np.mean(rows['kernel']) / 1e3:.1f} M groups/s."]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", default=["coco", "lvis"], choices=sorted(SIZES))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--iou_thr", type=float, default=0.55)
    ap.add_argument("--conf_type", default="avg", choices=["avg", "max"])
    ap.add_argument("--host-images", type=int, default=200, help="images of the subset the literal host form is timed on (0: skip)")
    ap.add_argument("--cut-offsets", action="store_true", help="add the kernel's time with the offsets table cut behind the last real group")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_fusion.py needs the GPU"
    dev = torch.device("cuda:0")
    lines = ["# Weighted boxes fusion on the device at validation-set sizes", "",
             "tools/bench_fusion.py: two synthetic models jittered from one detection set (synthetic boxes: the numbers of clusters say nothing "
             "about a model).  All routes run in one process and alternate; a column is one round, so two columns of a row are two runs of the "
             "same code and their difference is the spread.", ""]
    for name in args.sizes:
        lines += bench(name, args, dev) + [""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
