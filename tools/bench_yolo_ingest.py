#!/usr/bin/env python3
"""The input side of the YOLO step: decoded uint8 images to the normalised 640-px batch, ResizeToTensor.batch against two routes that run
without OpenCV.
    python tools/bench_yolo_ingest.py --reps 30 --out profiles/r25_yolo_ingest.md
Workload: a batch of 32 images of 480 x 640 with 7 boxes each, to 640 px, every second image flipped (synthetic: no dataset is read).  Four
routes, alternated inside one process so that they see the same machine:
  (y) ResizeToTensor.batch from CPU uint8 tensors: pack into the pinned buffer, one upload, one image and one box launch
  (z) ResizeToTensor.batch from uint8 tensors already on the device
  (a) upload the uint8 images, then permute, float, F.interpolate(mode="bicubic"), / 255 and normalise as torch operations on the device
      (a float bicubic without the uint8 rounding: not the same values, timed as the obvious stand-in)
  (b) upload the finished float32 [32, 3, 640, 640] batch from pageable host memory: what the reference's loader hands over after its
      per-sample host work (cv2.resize, / 255, normalise, helper.collate_fn), none of which is timed
(y), (a) and (b) are timed with the wall clock around a synchronised call, (z) with HIP events.  The last rows time mi355det_yolo_ingest_u8
alone (events around a run of launches) and a device-to-device copy of its output, and set the kernel's store rate against the copy's.
Prints the markdown table and, with --out, writes it."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), min(ms), q[0], q[2], max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--boxes", type=int, default=7)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    import torch.nn.functional as F
    from object_detectors_amd import _lib, ops
    from object_detectors_amd.yolo.dsets import transformations as tr
    assert torch.cuda.is_available(), "bench_yolo_ingest needs the GPU"
    dev = torch.device("cuda:0")
    N, H, W, S = args.batch, args.height, args.width, args.size
    g = torch.Generator().manual_seed(0)
    u8 = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) for _ in range(N)]
    flips = [bool(i & 1) for i in range(N)]
    rng = np.random.default_rng(0)
    targets = []
    for i in range(N):
        xy, wh = rng.random((args.boxes, 2)) * 0.5 * [W, H], (0.1 + rng.random((args.boxes, 2)) * 0.4) * [W, H]
        targets.append({"bbox": np.concatenate([xy, wh], 1), "category_id": rng.integers(0, 80, args.boxes), "area": wh[:, 0] * wh[:, 1], "image_id": i})
    u8_dev = [i.to(dev) for i in u8]
    t = tr.ResizeToTensor(S)
    mean = torch.tensor(tr.MEAN, device=dev)[:, None, None]
    std = torch.tensor(tr.STD, device=dev)[:, None, None]

    def route_y():
        return t.batch(u8, targets, flips)[0]

    def route_z():
        return t.batch(u8_dev, targets, flips)[0]

    def route_a():
        x = torch.stack([i.to(dev, non_blocking=True) for i in u8]).permute(0, 3, 1, 2).float()
        x = F.interpolate(x, size=(S, S), mode="bicubic", align_corners=False)
        return (x / 255.0 - mean) / std

    ref = route_y()
    finished = ref.cpu()                                # pageable, as torch.cat in helper.collate_fn leaves it

    def route_b():
        return finished.to(dev)

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def events(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)

    routes = [("y", route_y, wall), ("z", route_z, events), ("a", route_a, wall), ("b", route_b, wall)]
    assert torch.equal(route_z(), ref) and torch.equal(route_b(), ref)            # (y), (z) and (b) hold the same batch
    unflipped = [i for i in range(N) if not flips[i]]
    stand_in = float((route_a()[unflipped] - ref[unflipped]).abs().max())          # (a) does not flip, clamp or round to bytes
    ms = {name: [] for name, _, _ in routes}
    for rep in range(args.warmup + args.reps):
        for name, fn, timer in routes:
            v = timer(fn)
            if rep >= args.warmup:
                ms[name].append(v)

    # the image kernel alone, and a device copy of its output
    table = (_lib.YoloImage * N)(*[_lib.YoloImage(i * 3 * H * W, H, W, 3, int(flips[i]), 0, S) for i in range(N)])
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev)
    taps = np.concatenate([tr.cubic_taps(W, S), tr.cubic_taps(H, S)])
    taps_dev = torch.from_numpy(taps.view(np.uint8).copy()).to(dev)
    packed = torch.cat([i.reshape(-1) for i in u8_dev])
    lut = tr.normalised_bytes().to(dev)
    out = torch.empty((N, 3, S, S), dtype=torch.float32, device=dev)
    copy = torch.empty_like(out)

    def kernel():
        ops.yolo_ingest_u8(packed, table, table_dev, taps_dev, lut, S, out=out)
    for _ in range(args.warmup):
        kernel()
        copy.copy_(out)
    assert torch.equal(out, ref)
    k_ms, c_ms = [], []
    for _ in range(args.reps):
        k_ms.append(events(lambda: [kernel() for _ in range(10)]) / 10)
        c_ms.append(events(lambda: [copy.copy_(out) for _ in range(10)]) / 10)
    written, read = N * 3 * S * S * 4, N * 3 * H * W
    k_med, c_med = statistics.median(k_ms), statistics.median(c_ms)

    name = f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})"
    desc = {"y": "(y) ResizeToTensor.batch, CPU uint8 HWC: pack, 1 upload, 1 image + 1 box launch", "z": "(z) ResizeToTensor.batch, images on the device",
            "a": "(a) uint8 uploads, then torch float bicubic and normalise on the device", "b": "(b) upload of the finished float32 batch (pageable)"}
    lines = [
        "# YOLO ingest: uint8 images through the fixed-point bicubic resize",
        "",
        f"tools/bench_yolo_ingest.py on one {name}: batch {N} of {H} x {W} images, {args.boxes} boxes each, to {S} px -> {N} x 3 x {S} x {S}; every "
        f"second image flipped.  {args.reps} repetitions of each route after {args.warmup} warm-up rounds, the routes alternated round by round in "
        f"one process.  (y), (a), (b): wall clock around a synchronised call, uploads included ((y) and (a) upload {read / 1e6:.1f} MB, (b) "
        f"{written / 1e6:.1f} MB).  (z): HIP events.  (y), (z) and (b) were checked to hold the same bits before timing; (a) is a float bicubic "
        f"without flip, clamp or byte rounding (largest difference on the unflipped images {stand_in:.3f}).",
        "",
        "| route | median ms | min | p25 | p75 | max |",
        "|---|---:|---:|---:|---:|---:|",
    ]
    stats = {k: spread(v) for k, v in ms.items()}
    for k in "yzab":
        m, lo, q1, q3, hi = stats[k]
        lines.append(f"| {desc[k]} | {m:.3f} | {lo:.3f} | {q1:.3f} | {q3:.3f} | {hi:.3f} |")
    for label, v in (("mi355det_yolo_ingest_u8 alone (10 launches between two events, per launch)", k_ms),
                     ("device-to-device copy of its output (10 copies between two events, per copy)", c_ms)):
        m, lo, q1, q3, hi = spread(v)
        lines.append(f"| {label} | {m:.4f} | {lo:.4f} | {q1:.4f} | {q3:.4f} | {hi:.4f} |")
    lines += [
        "",
        f"The kernel writes {written / 1e6:.1f} MB (N * 3 * S * S * 4) and reads {read / 1e6:.1f} MB of pixels: {written / (k_med * 1e-3) / 1e12:.2f} TB/s "
        f"of stores at the median.  The copy writes the same bytes at {written / (c_med * 1e-3) / 1e12:.2f} TB/s (and reads as many): the kernel's "
        f"store rate is {100 * c_med / k_med:.0f}% of the copy's.",
        "",
        f"(y) <= (b): {'yes' if stats['y'][0] <= stats['b'][0] else 'NO'} ({stats['y'][0]:.3f} against {stats['b'][0]:.3f} ms; spread of (b) "
        f"{stats['b'][1]:.3f} .. {stats['b'][4]:.3f}).  (y) <= (a): {'yes' if stats['y'][0] <= stats['a'][0] else 'NO'} ({stats['y'][0]:.3f} against "
        f"{stats['a'][0]:.3f} ms; spread of (a) {stats['a'][1]:.3f} .. {stats['a'][4]:.3f}).",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
