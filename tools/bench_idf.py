#!/usr/bin/env python3
"""The TF-IDF class table from annotations at COCO-train and LVIS-v1-train size (synthetic index pairs with a long-tailed category
distribution, shuffled).
    python tools/bench_idf.py --sets coco lvis --rounds 20 --out profiles/r19_idf_table.md
Two routes from the device index pair to the frequencies and the 14 columns, timed in one process with HIP events around whole routes,
alternated round by round after a warm-up of each (a timed sample is --calls back-to-back calls of one route, reported per call):
    (a) dataset_stats.category_frequencies (mi355det_category_frequencies, with the read of its error counter) and, for the table, the
        compaction and mi355det_idf_table;
    (b) torch ops on the same device: torch.unique over image * n_categories + category keys and two bincount calls; for the table the same
        compaction and the formulas in float64 torch ops (torch.special.ndtri).
Before the timing the two routes' counts are compared (equal) and their columns (largest relative difference, printed).  For scale the
reference's per-image loop (tests/idf_oracle.py: bincount, coo_matrix, vstack per image) is timed on the CPU at --loop-images images; its
vstack is quadratic, so the figure says nothing about the full sizes.  Prints the markdown report and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"coco": dict(images=118287, categories=91, annotations=860001),
         "lvis": dict(images=100170, categories=1204, annotations=1270141)}


def synth(images, categories, annotations, seed):
    """Category ids 1 .. categories - 1 with probability proportional to 1 / rank (the hottest takes about a fifth at 90 ids, an eighth at
    1203), images uniform, order shuffled: int32 numpy (image_index, category_index)."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, categories)
    cat = rng.choice(np.arange(1, categories), annotations, p=p / p.sum())
    return rng.integers(0, images, annotations).astype(np.int32), cat.astype(np.int32)


def once_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_frequencies(im, cat, n_images, n_cats):
    keys = torch.unique(im.long() * n_cats + cat.long())
    return torch.bincount(cat, minlength=n_cats), torch.bincount(keys % n_cats, minlength=n_cats)


def torch_columns(img, inst, n_images):
    def family(total, freq):
        freq = freq.double()
        p = freq / total
        return [torch.log((total + 1) / (freq + 1)) + 1, torch.log(total / freq), torch.log((total - freq) / freq), -torch.special.ndtri(p),
                -torch.log(-torch.log(1 - p)), -torch.log2(p), -torch.log10(p)]
    return torch.stack(family(float(n_images), img) + family(inst.sum().double(), inst))


def bench(kind, size, rounds, calls, dev):
    from object_detectors_amd import dataset_stats as ds
    im_np, cat_np = synth(size["images"], size["categories"], size["annotations"], 0)
    im, cat = torch.from_numpy(im_np).to(dev), torch.from_numpy(cat_np).to(dev)
    I, K = size["images"], size["categories"]

    def table_of(freq):
        inst, img = freq(im, cat, I, K)
        ids = torch.nonzero(inst > 0).flatten()
        return ids, inst[ids].contiguous(), img[ids].contiguous()

    def kernel_table():
        _ids, inst, img = table_of(ds.category_frequencies)
        return ds.idf_columns(img.int(), inst.int(), I)

    def torch_table():
        _ids, inst, img = table_of(torch_frequencies)
        return torch_columns(img, inst, I)

    routes = {"a_freq": lambda: ds.category_frequencies(im, cat, I, K), "b_freq": lambda: torch_frequencies(im, cat, I, K),
              "a_table": kernel_table, "b_table": torch_table}
    a, b = routes["a_freq"](), routes["b_freq"]()
    assert torch.equal(a[0].long(), b[0]) and torch.equal(a[1].long(), b[1]), "the two routes count differently"
    ta, tb = routes["a_table"](), routes["b_table"]()
    fin = torch.isfinite(tb) & (tb != 0)
    rel = float(((ta - tb).abs()[fin] / tb.abs()[fin]).max())
    for _ in range(3):
        for r in routes.values():
            r()
    times = {r: [] for r in routes}
    for _ in range(rounds):
        for r, fn in routes.items():
            times[r].append(once_ms(lambda: [fn() for _ in range(calls)]) / calls)
    med = lambda xs: float(np.median(xs))
    span = lambda xs: f"{med(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"
    spread = lambda xs: 100.0 * (max(xs) - min(xs)) / med(xs)
    words = (K + 31) // 32
    lines = [f"## {kind.upper()}-train size: {I} images, {K} category ids, {size['annotations']} annotations; {int((a[0] > 0).sum())} present "
             f"categories, hottest category {int(a[0].max())} annotations, {int(a[1].sum())} distinct (image, category) pairs; bitmap "
             f"{I} x {words} words = {I * words * 4 / 1e6:.1f} MB", "",
             f"Counts of the two routes equal; largest relative difference of a finite column entry between them {rel:.2e}.", "",
             "| | (a) kernels ms | (b) torch ops ms | (b) / (a) | spread of (a) % | spread of (b) % |", "|---|---:|---:|---:|---:|---:|"]
    for label, ka, kb in (("frequencies", "a_freq", "b_freq"), ("frequencies + compaction + 14 columns", "a_table", "b_table")):
        lines.append(f"| {label} | **{span(times[ka])}** | **{span(times[kb])}** | **{med(times[kb]) / med(times[ka]):.2f}x** | "
                     f"{spread(times[ka]):.1f} | {spread(times[kb]):.1f} |")
    return lines + [""]


def cpu_loop(n_images, size):
    from tests import idf_oracle
    im, cat = synth(n_images, size["categories"], int(size["annotations"] * n_images / size["images"]), 1)
    ims = [[] for _ in range(n_images)]
    for i, c in zip(im.tolist(), cat.tolist()):
        ims[i].append(c)
    t0 = time.perf_counter()
    idf_oracle.reference_table(ims, size["categories"])
    return time.perf_counter() - t0, len(im)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["coco", "lvis"], choices=sorted(SIZES))
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls of a route per timed sample")
    ap.add_argument("--loop-images", type=int, default=5000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["# The TF-IDF class table from annotations on the device", "",
             f"tools/bench_idf.py on one MI355X, one process.  Per set 3 warm-up calls of every route, then {args.rounds} rounds; in each round "
             f"the four routes run one after the other, each {args.calls} times back to back between two HIP events (host work and the read of the "
             "error counter included); per call: median (min .. max) over the rounds, spread = (max - min) / median.", ""]
    for kind in args.sets:
        lines += bench(kind, SIZES[kind], args.rounds, args.calls, dev)
        torch.cuda.empty_cache()
    if args.loop_images > 0:
        lines += ["## The reference's per-image loop on the CPU, for scale", ""]
        for kind in args.sets:
            sec, n = cpu_loop(args.loop_images, SIZES[kind])
            lines.append(f"- {kind}: {args.loop_images} images, {n} annotations, {SIZES[kind]['categories']} ids: {sec:.2f} s (one run; the vstack "
                         "per image is quadratic in the images, do not extrapolate).")
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
