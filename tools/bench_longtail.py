#!/usr/bin/env python3
"""The long-tail baselines at LVIS width: Seesaw loss and Equalization loss v1, forward + gradient, at n = 2048 rows (4 images x 512
RoIs) and k = 1204 classes, and the repeat factors at LVIS-v1-train size (100 170 images, 1.27 million synthetic annotations).
    python tools/bench_longtail.py --rounds 20 --out profiles/r32_longtail.md
Per loss three routes, timed in one process with HIP events around whole routes, alternated round by round after a warm-up of each (a
timed sample is --calls back-to-back calls of one route, reported per call):
    (a) ops.fastrcnn_loss_longtail (csrc/longtail_kernels.hip): losses and both gradients from one launch sequence;
    (b) the same rule written as torch ops on the same device, forward and autograd backward to the logits and the box deltas;
    (c) 'ce' on the existing kernel (ops.fastrcnn_loss), the floor: two reads of the logits where Seesaw makes three.
Before the timing (a) is compared with (b): losses and gradients, largest difference printed.  The repeat factors are timed as
ops.repeat_factors on device-resident index vectors (the read of the error counter included) against the numpy form on the host.
Prints the markdown report and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, K = 2048, 1204
LVIS = dict(images=100170, categories=1204, annotations=1270141)


def once_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def torch_box(breg, labels, tgt):
    n, k = labels.shape[0], breg.shape[1] // 4
    pos = torch.where(labels > 0)[0]
    d = breg.reshape(n, k, 4)[pos, labels[pos]] - tgt[pos]
    a = d.abs()
    return torch.where(a < 1, 0.5 * d * d, a - 0.5).sum() / n


def torch_seesaw(logits, breg, labels, tgt, scale, counts, p=0.8, q=2.0, eps=1e-2):
    x = logits * scale
    rows = torch.arange(x.shape[0], device=x.device)
    with torch.no_grad():
        counts = counts + torch.bincount(labels, minlength=x.shape[1])
        ln = torch.log(counts.clamp(min=1).float())
        dn = ln[None, :] - ln[labels][:, None]
        ls = torch.log_softmax(x, 1)
        dr = ls - torch.clamp(ls[rows, labels], min=float(np.log(eps)))[:, None]
        shift = p * dn.clamp(max=0) + q * dr.clamp(min=0)
        shift[rows, labels] = 0
    return torch.nn.functional.cross_entropy(x + shift, labels), torch_box(breg, labels, tgt)


def torch_eql(logits, breg, labels, tgt, scale, tail):
    x = logits * scale
    n = x.shape[0]
    t = torch.zeros_like(x)
    t[torch.arange(n, device=x.device), labels] = 1
    t[:, 0] = 0
    w = 1 - (labels > 0).float()[:, None] * tail.float()[None, :] * (1 - t)
    return torch.nn.functional.binary_cross_entropy_with_logits(x, t, weight=w, reduction="sum") / n, torch_box(breg, labels, tgt)


def synth_annotations(seed):
    """Category ids 1 .. categories - 1 with probability proportional to rank^-1.6, images uniform: steeper than tools/bench_idf.py's
    1 / rank draw, under which no category falls below t = 1e-3 and nothing would repeat."""
    rng = np.random.default_rng(seed)
    p = np.arange(1, LVIS["categories"]) ** -1.6
    cat = rng.choice(np.arange(1, LVIS["categories"]), LVIS["annotations"], p=p / p.sum())
    return rng.integers(0, LVIS["images"], LVIS["annotations"]).astype(np.int32), cat.astype(np.int32)


def numpy_repeat_factors(im, cat, n_images, n_cat, t):
    pairs = np.unique(im.astype(np.int64) * n_cat + cat)
    f = np.bincount(pairs % n_cat, minlength=n_cat) / np.float64(n_images)
    with np.errstate(divide="ignore"):
        r_c = np.maximum(1.0, np.sqrt(t / f))
    r = np.ones(n_images)
    np.maximum.at(r, im, r_c[cat])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--calls", type=int, default=10, help="back-to-back calls of a route per timed sample")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import dataset_stats as ds
    from object_detectors_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cpu").manual_seed(0)
    logits = (torch.randn(N, K, generator=g) * 2).to(dev)
    breg = torch.randn(N, 4 * K, generator=g).to(dev)
    tgt = torch.randn(N, 4, generator=g).to(dev)
    labels = torch.randint(1, K, (N,), generator=g)
    labels[torch.rand(N, generator=g) < 0.75] = 0                  # three RoIs in four are background
    labels = labels.to(dev)
    scale = (0.5 + torch.rand(K, generator=g)).to(dev)
    counts0 = torch.randint(1, 10 ** 6, (K,), generator=g).to(dev)
    tail = (torch.rand(K, generator=g) < 0.3).to(torch.uint8)
    tail[0] = 0
    tail = tail.to(dev)

    def torch_route(fn, *state):
        lg, bg = logits.detach().requires_grad_(True), breg.detach().requires_grad_(True)
        c, b = fn(lg, bg, labels, tgt, scale, *state)
        gl, = torch.autograd.grad(c, lg)
        gb, = torch.autograd.grad(b, bg)
        return torch.stack([c.detach(), b.detach()]), gl, gb

    counts = counts0.clone()
    routes = {"seesaw_a": lambda: ops.fastrcnn_loss_longtail(logits, breg, labels, tgt, "seesaw", class_scale=scale, counts=counts, update_counts=False),
              "seesaw_b": lambda: torch_route(torch_seesaw, counts0 - torch.bincount(labels, minlength=K)),
              "eql_a": lambda: ops.fastrcnn_loss_longtail(logits, breg, labels, tgt, "eql", class_scale=scale, tail=tail),
              "eql_b": lambda: torch_route(torch_eql, tail),
              "ce": lambda: ops.fastrcnn_loss(logits, breg, labels, tgt, class_scale=scale, loss_type="ce")}
    # seesaw (a) reads counts0 as it is; (b) adds this batch to counts0 - bincount: the same counts, and (b) pays the histogram as (a) does
    # in training.  (a) with update_counts=True is timed as a sixth route, its counts growing from call to call.
    routes["seesaw_a_counting"] = lambda: ops.fastrcnn_loss_longtail(logits, breg, labels, tgt, "seesaw", class_scale=scale, counts=counts)
    agree = []
    for name in ("seesaw", "eql"):
        a, b = routes[name + "_a"](), routes[name + "_b"]()
        agree.append(f"- {name}: losses {a[0].tolist()} (a) against {b[0].tolist()} (b); largest |difference| of the class gradient "
                     f"{float((a[1] - b[1]).abs().max()):.2e} (largest entry {float(b[1].abs().max()):.2e}), of the box gradient "
                     f"{float((a[2] - b[2]).abs().max()):.2e}")
    for _ in range(3):
        for r in routes.values():
            r()
    counts.copy_(counts0)
    times = {r: [] for r in routes}
    for _ in range(args.rounds):
        for r, fn in routes.items():
            times[r].append(once_ms(lambda: [fn() for _ in range(args.calls)]) / args.calls)
    med = lambda xs: float(np.median(xs))
    span = lambda xs: f"{med(xs):.3f} ({min(xs):.3f} .. {max(xs):.3f})"
    ce = med(times["ce"])
    lines = ["# Long-tail baselines: Seesaw loss, EQL and repeat factors", "",
             f"tools/bench_longtail.py on one MI355X, one process.  n = {N} rows, k = {K} classes, float32, class scale on, three labels in four "
             f"background.  3 warm-up calls of every route, then {args.rounds} rounds; in each round the routes run one after the other, each "
             f"{args.calls} times back to back between two HIP events (host work included); per call: median (min .. max) over the rounds.", "",
             "The kernel route against the torch route, before the timing:", ""] + agree + ["",
             "| route | ms per call | against 'ce' |", "|---|---:|---:|"]
    names = {"ce": "(c) 'ce', existing kernel", "seesaw_a": "(a) seesaw kernel, counts read", "seesaw_a_counting": "(a) seesaw kernel, counts updated",
             "seesaw_b": "(b) seesaw torch ops + autograd", "eql_a": "(a) eql kernel", "eql_b": "(b) eql torch ops + autograd"}
    for r in ("ce", "seesaw_a", "seesaw_a_counting", "seesaw_b", "eql_a", "eql_b"):
        lines.append(f"| {names[r]} | **{span(times[r])}** | {med(times[r]) / ce:.2f}x |")
    lines += ["", f"Torch route over kernel route: seesaw {med(times['seesaw_b']) / med(times['seesaw_a_counting']):.1f}x, "
              f"eql {med(times['eql_b']) / med(times['eql_a']):.1f}x.", ""]

    # ---- repeat factors
    im_np, cat_np = synth_annotations(0)
    I, C, t = LVIS["images"], LVIS["categories"], 1e-3
    im, cat = torch.from_numpy(im_np).to(dev), torch.from_numpy(cat_np).to(dev)
    _inst, df = ds.category_frequencies(im, cat, I, C)
    r_dev = ops.repeat_factors(im, cat, df, I, t)
    host = []
    for _ in range(3):
        t0 = time.perf_counter()
        r_host = numpy_repeat_factors(im_np, cat_np, I, C, t)
        host.append((time.perf_counter() - t0) * 1e3)
    equal = bool(np.array_equal(r_dev.cpu().numpy(), r_host))
    rf, rf_all = [], []
    for _ in range(args.rounds):
        rf.append(once_ms(lambda: [ops.repeat_factors(im, cat, df, I, t) for _ in range(args.calls)]) / args.calls)
        rf_all.append(once_ms(lambda: [ds.repeat_factors({"image_index": im, "category_index": cat, "n_images": I, "n_categories": C}, t)
                                       for _ in range(args.calls)]) / args.calls)
    lines += [f"## Repeat factors at LVIS-v1-train size: {I} images, {C} category ids, {LVIS['annotations']} annotations, t = {t:g}", "",
              f"{int((r_host > 1).sum())} images with r > 1, implied epoch {r_host.sum():.0f} images; device result equal to the numpy form bit "
              f"for bit: {equal}.", "",
              "| route | ms per call |", "|---|---:|",
              f"| ops.repeat_factors (frequencies given) | **{span(rf)}** |",
              f"| dataset_stats.repeat_factors (frequencies + factors) | **{span(rf_all)}** |",
              f"| numpy on the host (unique, bincount, maximum.at), 3 runs | **{span(host)}** |", ""]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
