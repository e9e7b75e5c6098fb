#!/usr/bin/env python3
"""Mask results to COCO run lengths: the dense route (paste_masks -> `> 0.5` -> .cpu(), all there was before the run-length kernels) against
the fused route (mask_rle_paste + to_coco()), at the reference's inference shape: D = 100 detections on an 800 x 1216 image, synthetic
elliptical 28 x 28 probabilities.
    python tools/bench_mask_rle.py --reps 20 --out profiles/r12_mask_rle.md
Device sections are timed with HIP events after a warm-up; the end-to-end figures (host read and string building included) with the wall
clock around a synchronised call.  Prints the markdown table and, with --out, writes it."""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def synth(d, h, w, m, seed):
    """Boxes like tools/bench_maskrcnn.py's instances and the 28 x 28 probabilities of an ellipse inscribed in each (soft edge)."""
    g = torch.Generator().manual_seed(seed)
    tl = torch.rand((d, 2), generator=g) * torch.tensor([w, h]) * 0.6
    wh = torch.rand((d, 2), generator=g) * torch.tensor([w, h]) * 0.3 + 16
    boxes = torch.cat([tl, tl + wh], 1)
    yy, xx = torch.meshgrid(torch.arange(m, dtype=torch.float32), torch.arange(m, dtype=torch.float32), indexing="ij")
    c = (m - 1) / 2.0
    r = (0.25 + 0.2 * torch.rand((d, 2), generator=g)) * m
    dist = ((xx[None] - c) / r[:, 0, None, None]) ** 2 + ((yy[None] - c) / r[:, 1, None, None]) ** 2
    probs = torch.sigmoid((1.0 - dist) * 6.0)
    return probs[:, None].contiguous(), boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--detections", type=int, default=100)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1216)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops
    dev = torch.device("cuda:0")
    D, H, W, M = args.detections, args.height, args.width, 28
    probs, boxes = synth(D, H, W, M, 0)
    probs, boxes = probs.to(dev), boxes.to(dev)

    # ---- the dense route, section by section and end to end
    t_paste = device_ms(lambda: ops.paste_masks(probs, boxes, (H, W)), args.reps, args.warmup)
    pasted = ops.paste_masks(probs, boxes, (H, W))
    t_thr = device_ms(lambda: pasted > 0.5, args.reps, args.warmup)
    bits = pasted > 0.5
    t_copy = wall_ms(lambda: bits.cpu(), args.reps, args.warmup)
    t_dense = wall_ms(lambda: (ops.paste_masks(probs, boxes, (H, W)) > 0.5).cpu(), args.reps, args.warmup)
    # ---- the fused route
    L = ops.lib()
    from object_detectors_amd._lib import check, ptr, stream_ptr
    nbytes = L.mi355det_mask_rle_workspace(D, W)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    roff = torch.empty(D + 1, dtype=torch.int64, device=dev)
    src = (None, ptr(probs), ptr(boxes), D, M, 1, H, W, 0.5)
    t_count = device_ms(lambda: check(L.mi355det_mask_rle_count(*src, ptr(roff), ptr(ws), nbytes, stream_ptr()), "count"), args.reps, args.warmup)
    total = int(roff[-1])
    counts = torch.empty(total, dtype=torch.int32, device=dev)
    area = torch.empty(D, dtype=torch.int64, device=dev)
    bbox = torch.empty((D, 4), dtype=torch.int32, device=dev)
    t_emit = device_ms(lambda: check(L.mi355det_mask_rle_emit(*src, ptr(roff), total, ptr(counts), total, ptr(area), ptr(bbox), ptr(ws), nbytes,
                                                              stream_ptr()), "emit"), args.reps, args.warmup)
    t_rle = wall_ms(lambda: ops.mask_rle_paste(probs, boxes, (H, W)), args.reps, args.warmup)
    t_fused = wall_ms(lambda: ops.mask_rle_paste(probs, boxes, (H, W)).to_coco(), args.reps, args.warmup)
    batch = ops.mask_rle_paste(probs, boxes, (H, W))
    coco = batch.to_coco()
    # ---- the dense kernel on pasted masks (the reference's contract), and agreement of the two routes
    t_rle_dense = wall_ms(lambda: ops.mask_rle_dense(pasted), args.reps, args.warmup)
    same = torch.equal(batch.decode(), bits[:, 0].cpu().to(torch.uint8))

    px = D * H * W
    in_bytes = probs.numel() * 4 + boxes.numel() * 4
    dense_hbm = in_bytes + px * 4 + px * 4 + px + px        # paste write, threshold read + write, copy read
    dense_host = px
    fused_hbm = 2 * in_bytes + 2 * nbytes + (D + 1) * 8 + total * 4 + D * 24      # tables written by count, read by scan / emit (upper bound: whole)
    fused_host = (D + 1) * 8 + total * 4
    mb = lambda b: f"{b / 1e6:.2f}"
    lines = [
        "# Mask results to COCO run lengths: dense route against fused route",
        "",
        f"tools/bench_mask_rle.py, D = {D} detections, image {H} x {W}, 28 x 28 synthetic elliptical probabilities, padding 1, threshold 0.5; "
        f"{args.reps} repetitions after {args.warmup} warm-up calls.  Device sections: HIP events; end-to-end rows: wall clock around "
        "synchronised calls (they include the host reads).",
        "",
        "| route | section | ms | HBM MB | device->host MB |",
        "|---|---|---:|---:|---:|",
        f"| dense | mi355det_paste_masks (writes fp32 [D, H, W]) | {t_paste:.3f} | {mb(in_bytes + px * 4)} | |",
        f"| dense | `> 0.5` (reads fp32, writes bool) | {t_thr:.3f} | {mb(px * 5)} | |",
        f"| dense | `.cpu()` of the bool masks | {t_copy:.3f} | {mb(px)} | {mb(px)} |",
        f"| dense | **paste -> `> 0.5` -> `.cpu()`, end to end** | **{t_dense:.3f}** | {mb(dense_hbm)} | {mb(dense_host)} |",
        f"| fused | mi355det_mask_rle_count (column transitions, scans, offsets) | {t_count:.3f} | {mb(in_bytes + 2 * nbytes)} | |",
        f"| fused | mi355det_mask_rle_emit ({total} counts, area, bbox) | {t_emit:.3f} | {mb(in_bytes + nbytes + total * 4)} | |",
        f"| fused | ops.mask_rle_paste (count, offsets read, emit) | {t_rle:.3f} | {mb(fused_hbm)} | {mb((D + 1) * 8)} |",
        f"| fused | **mask_rle_paste + to_coco(), end to end** | **{t_fused:.3f}** | {mb(fused_hbm)} | {mb(fused_host)} |",
        f"| dense masks in | ops.mask_rle_dense on the pasted masks (two reads of fp32 [D, H, W]) | {t_rle_dense:.3f} | {mb(2 * px * 4)} | {mb((D + 1) * 8)} |",
        "",
        f"End to end the fused route takes {t_fused:.3f} ms against {t_dense:.3f} ms: {t_dense / t_fused:.1f}x.  The dense route still has to "
        "run-length encode its bitmaps on the host afterwards; the fused figure already includes the strings.",
        f"Counts in all: {total} ({total / D:.1f} per detection); string bytes: {sum(len(r['counts']) for r in coco)}.  "
        f"Decoded fused result equals the dense route's bits: {same}.",
        "HBM MB are the bytes each section's kernels read and write by construction (the column tables counted whole: an upper bound), "
        "not counters.",
        "",
        f"Where the time goes.  The dense route is its host copy: {t_copy:.3f} of {t_dense:.3f} ms move the bool masks to the host, and the fused "
        f"route has nothing of that size to move.  On the device alone the margin is smaller than the traffic suggests: paste + threshold take "
        f"{t_paste + t_thr:.3f} ms at HBM speed, count + emit {t_count + t_emit:.3f} ms while moving under 10 MB, far below HBM speed.  What bounds "
        "them was not profiled; by their structure it is latency: one thread walks the box rows of its column in sequence (up to a few hundred pixels, each the four taps and the two-stage "
        "blend of the paste rule), once per pass, and the count pass is followed by two small scan launches.  Of the fused end-to-end time, "
        f"{t_fused - t_rle:.3f} ms is the host side of to_coco() (one copy of the counts, one codec call per mask).",
    ]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
