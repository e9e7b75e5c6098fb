#!/usr/bin/env python3
"""Anchor k-means at COCO-train and LVIS-v1-train size (synthetic log-uniform boxes over 640 x 480 images, shuffled).
    python tools/bench_anchors.py --sets coco lvis --rounds 3 --out profiles/r20_anchors.md
Two jobs: the reference's (kmeans_anchors.py: the selected boxes in 3 area bands, k = 3 on four features, 10 restarts) and the YOLO one
(k = 9 on (w, h) under 1 - IoU, 10 restarts).  Routes, timed in one process with HIP events around whole routes, alternated round by round
after a warm-up of each, all from the same initial centres:
    (a) anchors.kmeans: every problem and restart in one sweep of the points per pass (mi355det_kmeans_passes), the flag read every 8 passes,
        the check of the points, the final assignment and all host work included.  Its time per enqueued pass is the difference of a run cut
        at 24 passes and one cut at 8, over 16, which cancels the fixed costs;
    (b) the same Lloyd passes as torch ops on the same device, per problem and restart: broadcast distance in the stated operation order,
        argmin, index_add_ and bincount, centre = sum / count where count > 0 - for exactly the passes (a) took, without any convergence
        check or host read, on per-problem point tensors gathered outside the timing.  index_add_ is float64 atomics onto k rows, which
        makes a pass cost tens of milliseconds at these sizes, so only the first --torch-restarts restarts of every problem are run (their
        labels are compared with (a)'s) and the whole job is the measured time per pass times (a)'s pass count, marked as not run;
    (c) scikit-learn's KMeans(init=C0, n_init=1, tol=0, algorithm="lloyd") on the host where it imports, for --sklearn-restarts restarts of
        every problem (one run each, wall clock).
Prints the markdown report and, with --out, writes it."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES = {"coco": dict(images=118287, annotations=860001), "lvis": dict(images=100170, annotations=1270141)}


def synth(images, annotations, seed):
    rng = np.random.default_rng(seed)
    wh = np.exp(rng.uniform(np.log(0.004), np.log(0.98), (annotations, 2))) * np.array([640.0, 480.0])
    return {"box_wh": wh, "image_index": rng.integers(0, images, annotations).astype(np.int32),
            "image_size": np.tile(np.array([[640, 480]], np.int32), (images, 1)), "n_images": images}


def once_ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def torch_distance(X, C, metric):
    if metric == "iou":
        i = torch.minimum(X[:, None, 0], C[None, :, 0]) * torch.minimum(X[:, None, 1], C[None, :, 1])
        return 1.0 - i / (X[:, None, 0] * X[:, None, 1] + C[None, :, 0] * C[None, :, 1] - i)
    sq = (X[:, None, :] - C[None, :, :]) ** 2
    d = sq[..., 0]
    for j in range(1, X.shape[1]):
        d = d + sq[..., j]
    return d


def torch_lloyd(Xs, init, passes, metric):
    """Route (b): Xs[p] the points of problem p, init [P, R, k, F], passes[p][r] assignments -> labels [P][R]."""
    out = []
    for p, X in enumerate(Xs):
        row = []
        for r in range(init.shape[1]):
            C = init[p, r].clone()
            k = C.shape[0]
            for it in range(passes[p][r]):
                labels = torch.argmin(torch_distance(X, C, metric), dim=1)
                if it + 1 < passes[p][r]:
                    sums = torch.zeros_like(C).index_add_(0, labels, X)
                    counts = torch.bincount(labels, minlength=k)
                    C = torch.where((counts > 0)[:, None], sums / counts.clamp(min=1)[:, None], C)
            row.append(labels)
        out.append(row)
    return out


def bench(kind, job, size, rounds, max_iter, sk_restarts, torch_restarts, dev):
    from object_detectors_amd import anchors as A
    feats = A.box_features(synth(size["images"], size["annotations"], 0), device=dev)
    if job == "reference":
        X, problem, P, k, metric = feats["features"], feats["band"], 3, 3, "euclid"
    else:
        X, problem, P, k, metric = feats["features"][feats["keep"]][:, :2].contiguous(), None, 1, 9, "iou"
    R = 10
    rows = [torch.arange(X.shape[0], device=dev)] if problem is None else [torch.nonzero(problem == p).flatten() for p in range(P)]
    sel = A.seeded_rows([int(r.numel()) for r in rows], k, R, 0).to(dev)
    init = torch.stack([X[rows[p][sel[p]]] for p in range(P)]).contiguous()
    Xs = [X[r].contiguous() for r in rows]
    args = dict(problem=problem, n_problems=P, metric=metric, init=init)
    full = lambda: A.kmeans(X, k, max_iter=max_iter, **args)
    cut = lambda n: (lambda: A.kmeans(X, k, max_iter=n, **args))
    a = full()
    passes = a["n_iter"].cpu().tolist()
    TR = max(1, min(torch_restarts, R))
    route_b = lambda: torch_lloyd(Xs, init[:, :TR], passes, metric)
    b = route_b()
    differ = sum(int((b[p][r] != a_labels).sum()) for p in range(P) for r in range(TR)
                 for a_labels in [A.assign(Xs[p], a["all_centers"][p, r], metric=metric)[0].long()])
    b_passes = sum(sum(row[:TR]) for row in passes)
    routes = {"a": full, "a8": cut(8), "a24": cut(24), "b": route_b}
    times = {r: [] for r in routes}
    for _ in range(rounds):
        for r, fn in routes.items():
            times[r].append(once_ms(fn)[0])
    med = lambda xs: float(np.median(xs))
    span = lambda xs: f"{med(xs):.1f} ({min(xs):.1f} .. {max(xs):.1f})"
    n_pass = max(max(row) for row in passes)
    total = sum(sum(row) for row in passes)
    per_pass = (med(times["a24"]) - med(times["a8"])) / 16
    lines = [f"### {kind.upper()}-train size, the {job} job: {X.shape[0]} points x {X.shape[1]} features, problems of "
             f"{[int(r.numel()) for r in rows]} points, k = {k}, {R} restarts, {metric}", "",
             f"Passes per (problem, restart): {passes}; the longest took {n_pass} (max_iter {max_iter}), {total} in all.  Labels of (b) that "
             f"differ from (a)'s, over all problems and the {TR} restart(s) it ran: {differ} of {sum(int(r.numel()) for r in rows) * TR}.", "",
             "| route | end to end ms: median (min .. max) | per pass ms |", "|---|---:|---:|",
             f"| (a) kernels, {n_pass} sweeps | **{span(times['a'])}** | **{per_pass:.3f}** per sweep of all {P * R} (problem, restart) "
             f"(24-pass run {med(times['a24']):.1f} ms, 8-pass run {med(times['a8']):.1f} ms) |",
             f"| (b) torch ops, {TR} restart(s) of each problem, {b_passes} passes | **{span(times['b'])}** | "
             f"**{med(times['b']) / b_passes:.3f}** per (problem, restart) pass, {med(times['b']) / b_passes * P * R:.1f} per sweep of all "
             f"{P * R} |",
             f"| (b) all {R} restarts at that rate (NOT run): {total} passes | {med(times['b']) / b_passes * total:.0f} | |",
             f"| (b) / (a), whole job, (b) extrapolated | **{med(times['b']) / b_passes * total / med(times['a']):.0f}x** | |", ""]
    if sk_restarts > 0:
        try:
            from sklearn.cluster import KMeans
        except ImportError:
            lines += ["(c) scikit-learn does not import here: left out.", ""]
        else:
            sec, sk_passes = 0.0, 0
            for p in range(P):
                Xh = Xs[p].cpu().numpy()
                for r in range(min(sk_restarts, R)):
                    t0 = time.perf_counter()
                    km = KMeans(n_clusters=k, init=init[p, r].cpu().numpy(), n_init=1, tol=0, max_iter=max_iter, algorithm="lloyd").fit(Xh)
                    sec += time.perf_counter() - t0
                    sk_passes += km.n_iter_
            note = "Euclidean only: the (w, h) points under its own distance, not 1 - IoU; " if metric == "iou" else ""
            lines += [f"(c) scikit-learn on the host ({note}{os.cpu_count()} CPUs reported, thread pools as the environment sets them), "
                      f"{min(sk_restarts, R)} restart(s) of each problem, one run: {sec:.2f} s for {sk_passes} passes = "
                      f"{1e3 * sec / max(sk_passes, 1):.1f} ms per (problem, restart) pass; all {R} restarts were not run.", ""]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", nargs="+", default=["coco", "lvis"], choices=sorted(SIZES))
    ap.add_argument("--jobs", nargs="+", default=["reference", "yolo"], choices=["reference", "yolo"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=300)
    ap.add_argument("--sklearn-restarts", type=int, default=1, help="restarts per problem that scikit-learn runs on the host (0: none)")
    ap.add_argument("--torch-restarts", type=int, default=1, help="restarts per problem that the torch route runs")
    ap.add_argument("--annotations", type=int, default=None, help="override the sets' annotation counts (a rehearsal at a small size)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.annotations:
        for size in SIZES.values():
            size["annotations"] = args.annotations
    dev = torch.device("cuda:0")
    lines = ["# Anchor k-means on the device", "",
             f"tools/bench_anchors.py on one MI355X, one process.  Per set and job one warm-up run of every route (the one that also gives the "
             f"pass counts and the labels), then {args.rounds} rounds; in each round the routes run one after the other between two HIP events, host "
             "work and synchronising reads included.", ""]
    for kind in args.sets:
        for job in args.jobs:
            lines += bench(kind, job, SIZES[kind], args.rounds, args.max_iter, args.sklearn_restarts, args.torch_restarts, dev)
            print("\n".join(lines[-12:]), flush=True)
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
