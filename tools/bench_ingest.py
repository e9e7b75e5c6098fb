#!/usr/bin/env python3
"""The input side of the torchvision-path models: decoded images to the padded batch, the float route against the uint8 route.
    python tools/bench_ingest.py --reps 30 --out profiles/r16_ingest.md
Workload: a batch of 16 images of 480 x 640 with 7 boxes each, min side 800 / max side 1333, every second image flipped (synthetic: no
dataset is read).  Four routes, alternated inside one process so that they see the same machine:
  (a) float route from the CPU: float32 CHW images in [0, 1] (flipped on the host beforehand, not timed), each uploaded on its own, then
      `transform(list, targets)`: one resize launch and one box launch per image
  (b) uint8 route from the CPU: `transform.ingest(uint8 HWC list, targets, flips)`, packing and upload included
  (c) the float route with the images already on the device
  (d) the uint8 route with the images already on the device
(a) and (b) are timed with the wall clock around a synchronised call, (c) and (d) with HIP events.  The last rows time mi355det_ingest_u8
alone (events around a run of launches) and set the bytes it writes against the time.  Prints the markdown table and, with --out, writes it."""
import argparse
import ctypes
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_ACHIEVABLE = 6.3e12         # bytes/s a float4 copy reaches on an MI355X (8 TB/s is the specification)


def spread(ms):
    q = statistics.quantiles(ms, n=4)
    return statistics.median(ms), min(ms), q[0], q[2], max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--height", type=int, default=480)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--boxes", type=int, default=7)
    ap.add_argument("--min-size", type=int, default=800)
    ap.add_argument("--max-size", type=int, default=1333)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    from object_detectors_amd import _lib
    from object_detectors_amd.tvision.engine import IMAGE_MEAN, IMAGE_STD
    from object_detectors_amd.tvision.transform import GeneralizedRCNNTransform, plan_ingest
    assert torch.cuda.is_available(), "bench_ingest needs the GPU"
    dev = torch.device("cuda:0")
    N, H, W = args.batch, args.height, args.width
    g = torch.Generator().manual_seed(0)
    u8 = [torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, generator=g) for _ in range(N)]
    flips = [bool(i & 1) for i in range(N)]
    xy = torch.rand(N, args.boxes, 2, generator=g) * 0.5
    boxes = [torch.cat([p, p + 0.1 + torch.rand(args.boxes, 2, generator=g) * 0.4], 1) * torch.tensor([W, H, W, H], dtype=torch.float32) for p in xy]
    f32 = [(i.permute(2, 0, 1).float().div(255).flip(-1) if f else i.permute(2, 0, 1).float().div(255)).contiguous() for i, f in zip(u8, flips)]
    boxes_flipped = []
    for b, f in zip(boxes, flips):
        b = b.clone()
        if f:
            b[:, [0, 2]] = W - b[:, [2, 0]]
        boxes_flipped.append(b)
    u8_dev, f32_dev = [i.to(dev) for i in u8], [i.to(dev) for i in f32]
    boxes_dev, boxes_flipped_dev = [b.to(dev) for b in boxes], [b.to(dev) for b in boxes_flipped]
    t = GeneralizedRCNNTransform(args.min_size, args.max_size, list(IMAGE_MEAN), list(IMAGE_STD))
    t.eval()

    def route_a():
        return t([i.to(dev, non_blocking=True) for i in f32], [{"boxes": b.to(dev, non_blocking=True)} for b in boxes_flipped])

    def route_b():
        return t.ingest(u8, [{"boxes": b} for b in boxes], flips)

    def route_c():
        return t(f32_dev, [{"boxes": b} for b in boxes_flipped_dev])

    def route_d():
        return t.ingest(u8_dev, [{"boxes": b} for b in boxes_dev], flips)

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

    routes = [("a", route_a, wall), ("b", route_b, wall), ("c", route_c, events), ("d", route_d, events)]
    ref, ref_t = route_c()
    for name, fn, _ in routes:                      # the four routes compute the same batch and the same boxes
        il, tg = fn()
        assert torch.equal(il.tensors, ref.tensors), name
        assert all(torch.equal(x["boxes"], y["boxes"]) for x, y in zip(tg, ref_t)), name
    ms = {name: [] for name, _, _ in routes}
    for rep in range(args.warmup + args.reps):
        for name, fn, timer in routes:
            v = timer(fn)
            if rep >= args.warmup:
                ms[name].append(v)

    # the image kernel alone
    plan = plan_ingest([(H, W)] * N, float(args.min_size), float(args.max_size), t.size_divisible)
    table = (_lib.IngestImage * N)(*[_lib.IngestImage(plan.offsets[i], H, W, plan.sizes[i][0], plan.sizes[i][1], int(flips[i]), plan.first_tile[i])
                                     for i in range(N)])
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev)
    packed = torch.cat([i.reshape(-1) for i in u8_dev])
    ph, pw = plan.pad
    out = torch.empty((N, 3, ph, pw), dtype=torch.float32, device=dev)
    mean, std = t._mean_std(dev)

    def kernel():
        _lib.check(_lib.lib().mi355det_ingest_u8(_lib.ptr(packed), plan.nbytes, ctypes.cast(table, ctypes.c_void_p), _lib.ptr(table_dev), N,
                                                 _lib.ptr(mean), _lib.ptr(std), _lib.ptr(out), ph, pw, _lib.stream_ptr()), "ingest_u8")
    for _ in range(args.warmup):
        kernel()
    assert torch.equal(out, ref.tensors)
    k_ms = []
    for _ in range(args.reps):
        k_ms.append(events(lambda: [kernel() for _ in range(10)]) / 10)
    written, read = N * 3 * ph * pw * 4, plan.nbytes
    k_med = statistics.median(k_ms)

    name = f"{torch.cuda.get_device_name(0)} ({torch.cuda.get_device_properties(0).gcnArchName.split(':')[0]})"
    desc = {"a": "(a) float route, CPU float32 CHW: N uploads, N resize + N box launches", "b": "(b) uint8 route, CPU uint8 HWC: pack, 1 upload, 1 image + 1 box launch",
            "c": "(c) float route, images on the device", "d": "(d) uint8 route, images on the device"}
    lines = [
        "# Batched uint8 ingest against the float route",
        "",
        f"tools/bench_ingest.py on one {name}: batch {N} of {H} x {W} images, {args.boxes} boxes each, min side {args.min_size} / max side "
        f"{args.max_size} -> batch {N} x 3 x {ph} x {pw}; every second image flipped.  {args.reps} repetitions of each route after {args.warmup} "
        "warm-up rounds, the routes alternated round by round in one process.  (a) and (b): wall clock around a synchronised call, uploads "
        "included ((a) uploads " f"{N * 3 * H * W * 4 / 1e6:.1f} MB, (b) {plan.nbytes / 1e6:.1f} MB; the host-side flip and division of (a) "
        "are done beforehand and not timed).  (c) and (d): HIP events.  The four routes were checked to give the same bits before timing.",
        "",
        "| route | median ms | min | p25 | p75 | max |",
        "|---|---:|---:|---:|---:|---:|",
    ]
    stats = {k: spread(v) for k, v in ms.items()}
    for k in "abcd":
        m, lo, q1, q3, hi = stats[k]
        lines.append(f"| {desc[k]} | {m:.3f} | {lo:.3f} | {q1:.3f} | {q3:.3f} | {hi:.3f} |")
    km, klo, kq1, kq3, khi = spread(k_ms)
    lines += [
        f"| mi355det_ingest_u8 alone (10 launches between two events, per launch) | {km:.4f} | {klo:.4f} | {kq1:.4f} | {kq3:.4f} | {khi:.4f} |",
        "",
        f"The kernel writes {written / 1e6:.1f} MB (N * 3 * pad_h * pad_w * 4) and reads {read / 1e6:.1f} MB of pixels: "
        f"{written / (k_med * 1e-3) / 1e12:.2f} TB/s of stores at the median, {100 * written / (k_med * 1e-3) / HBM_ACHIEVABLE:.0f}% of the "
        f"{HBM_ACHIEVABLE / 1e12:.1f} TB/s a copy achieves on this GPU ({100 * (written + read) / (k_med * 1e-3) / HBM_ACHIEVABLE:.0f}% with the reads).",
        "",
        f"(b) <= (a): {'yes' if stats['b'][0] <= stats['a'][0] else 'NO'} ({stats['b'][0]:.3f} against {stats['a'][0]:.3f} ms; spread of (a) "
        f"{stats['a'][1]:.3f} .. {stats['a'][4]:.3f}).  (d) <= (c): {'yes' if stats['d'][0] <= stats['c'][0] else 'NO'} ({stats['d'][0]:.3f} against "
        f"{stats['c'][0]:.3f} ms; spread of (c) {stats['c'][1]:.3f} .. {stats['c'][4]:.3f}).",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
