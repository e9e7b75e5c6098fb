#!/usr/bin/env python3
"""Keypoint R-CNN ResNet-50-FPN (tvision/keypoint_rcnn.py) on synthetic person-like data.  GPU only; not a test.

  * training step: bs 4, 800 px, beside FasterRCNN on the same box, the two routes alternated in one process: what the branch costs;
  * eval tail: mi355det_heatmaps_to_keypoints for 100 and 1000 detections with COCO-like box sizes, beside the reference's per-RoI loop of
    torch ops (two .item() reads, one bicubic interpolate, one argmax per RoI) on the same device;
  * ingest: GeneralizedRCNNTransform.ingest with and without keypoints in the targets (the difference is the keypoint launch and its copies),
    and the launch alone.

    python tools/bench_keypointrcnn.py --rounds 3 --out profiles/r31_keypoint_rcnn.md
Prints one JSON line; --out appends a markdown table of every round."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3 / reps


def persons(batch, px, gt, K, gen, dev):
    out = []
    for _ in range(batch):
        tl = torch.rand((gt, 2), generator=gen) * px * 0.6
        wh = torch.rand((gt, 2), generator=gen) * px * torch.tensor([0.15, 0.3]) + 24        # upright boxes
        kp = torch.cat([tl[:, None] + torch.rand((gt, K, 2), generator=gen) * wh[:, None], torch.randint(0, 3, (gt, K, 1), generator=gen).float()], 2)
        kp[kp[..., 2] == 0] = 0
        out.append({"boxes": torch.cat([tl, tl + wh], 1).to(dev), "labels": torch.ones(gt, dtype=torch.int64, device=dev), "keypoints": kp.to(dev)})
    return out


def coco_like_boxes(n, gen):
    """Person boxes of an 800 x 1333 image: heights log-uniform between 16 and 600 px, widths 0.3 .. 0.8 of the height (at least 12 px)."""
    h = torch.exp(torch.rand(n, generator=gen) * (np.log(600) - np.log(16)) + np.log(16))
    w = (h * (0.3 + 0.5 * torch.rand(n, generator=gen))).clamp(min=12)
    x1, y1 = torch.rand(n, generator=gen) * (1333 - w).clamp(min=0), torch.rand(n, generator=gen) * (800 - h).clamp(min=0)
    return torch.stack([x1, y1, x1 + w, y1 + h], 1)


def reference_loop(maps, rois):
    """roi_heads.py:274-327 as the reference runs it, on the device the tensors are on."""
    import torch.nn.functional as F
    k = maps.shape[1]
    w = (rois[:, 2] - rois[:, 0]).clamp(min=1)
    h = (rois[:, 3] - rois[:, 1]).clamp(min=1)
    wc, hc = w.ceil(), h.ceil()
    xy = torch.zeros((len(rois), 3, k), dtype=torch.float32, device=maps.device)
    sc = torch.zeros((len(rois), k), dtype=torch.float32, device=maps.device)
    for i in range(len(rois)):
        ow, oh = int(wc[i].item()), int(hc[i].item())
        big = F.interpolate(maps[i][None], size=(oh, ow), mode="bicubic", align_corners=False)[0]
        pos = big.reshape(k, -1).argmax(dim=1)
        xi = pos % ow
        yi = (pos - xi) // ow
        xy[i, 0] = (xi.float() + 0.5) * (w[i] / ow) + rois[i, 0]
        xy[i, 1] = (yi.float() + 0.5) * (h[i] / oh) + rois[i, 1]
        xy[i, 2] = 1
        sc[i] = big[torch.arange(k, device=maps.device), yi, xi]
    return xy.permute(0, 2, 1), sc


def near_tie_gap(maps, rois, xy, same):
    """The near-tie rule of the tests on the pairs whose position differs from the loop's: the reference's upsampled map at its own arg-max
    minus its value at the kernel's position, the largest over those pairs, over max|map| (0.0 when no pair differs)."""
    import torch.nn.functional as F
    worst = 0.0
    for i, k in torch.nonzero(~same).tolist():
        w, h = (rois[i, 2] - rois[i, 0]).clamp(min=1), (rois[i, 3] - rois[i, 1]).clamp(min=1)
        ow, oh = int(w.ceil().item()), int(h.ceil().item())
        big = F.interpolate(maps[i, k][None, None], size=(oh, ow), mode="bicubic", align_corners=False)[0, 0]
        xi = int(torch.round((xy[i, k, 0] - rois[i, 0]) / (w / ow) - 0.5).clamp(0, ow - 1).item())
        yi = int(torch.round((xy[i, k, 1] - rois[i, 1]) / (h / oh) - 0.5).clamp(0, oh - 1).item())
        worst = max(worst, float((big.max() - big[yi, xi]) / maps[i, k].abs().max()))
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--px", type=int, default=800)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--gt", type=int, default=7, help="persons per image")
    ap.add_argument("--routes", default="faster_rcnn,keypoint_rcnn", help="which models to build and time (one name: that model alone in the process)")
    ap.add_argument("--extra-streams", type=int, default=0, help="create this many idle streams before the models (what a second model in the "
                    "process does to the stream-to-hardware-queue mapping, without the model)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from object_detectors_amd import ops
    from object_detectors_amd.optim import FlatSGD
    from object_detectors_amd.parallel import step_stream
    from object_detectors_amd.tvision.frcnn import fasterrcnn_resnet50_fpn
    from object_detectors_amd.tvision.keypoint_rcnn import keypointrcnn_resnet50_fpn
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(step_stream(dev))
    K, P = 17, args.px
    gen = torch.Generator().manual_seed(0)
    imgs = torch.rand((args.batch, 3, P, P), generator=gen).to(dev)
    targets = persons(args.batch, P, args.gt, K, gen, dev)
    box_targets = [{k: v for k, v in t.items() if k != "keypoints"} for t in targets]
    routes = {}
    idle = [torch.cuda.Stream(device=dev) for _ in range(args.extra_streams)]
    known = {"faster_rcnn": (fasterrcnn_resnet50_fpn, box_targets), "keypoint_rcnn": (keypointrcnn_resnet50_fpn, targets)}
    for name in args.routes.split(","):                                  # built, warmed and timed in the order given
        ctor, tg = known[name]
        torch.manual_seed(0)
        model = ctor(num_classes=2, device=dev, min_size=P, max_size=P)
        eng = model.engine
        for sp in eng.specs:          # stable random-init residual stack (tools/bench_frcnn.py)
            if sp.bn and sp.bn.endswith(".bn3"):
                eng.buffers[sp.bn + ".weight"].fill_(0.2)
        eng.refresh_frozen()
        opt = FlatSGD.for_engine(eng, lr=1e-3, momentum=0.9, weight_decay=1e-4)
        opt_head = torch.optim.SGD(model.head_parameters(), lr=1e-3, momentum=0.9, weight_decay=1e-4)
        model.train()

        def step(model=model, opt=opt, opt_head=opt_head, tg=tg):
            opt_head.zero_grad(set_to_none=True)
            losses = model(imgs, tg)
            opt.step()
            opt_head.step()
            return losses
        for _ in range(args.warmup):
            step()
        routes[name] = (model, step)
    rounds = []
    for _ in range(args.rounds):
        row = {}
        for name, (model, step) in routes.items():                   # alternated: one window per route per round; a step spans several
            row[name + "_step_ms"] = round(wall(step, args.steps), 3)     # streams, so the host clock around a synchronise times it
            row[name + "_step_ms_events"] = round(timed(step, args.steps), 3)
        rounds.append(row)
    if "keypoint_rcnn" not in routes:
        print(json.dumps({"metric": "keypointrcnn_resnet50_fpn", "routes": args.routes, "extra_streams": len(idle), "rounds": rounds}))
        return
    kmodel = routes["keypoint_rcnn"][0]
    rows_seen = kmodel.last_keypoint_rows
    # ---- eval tail
    tail = {}
    for n in (100, 1000):
        boxes = coco_like_boxes(n, gen).to(dev)
        yy, xx = torch.meshgrid(torch.arange(56.0), torch.arange(56.0), indexing="ij")
        c = torch.rand(n, K, 2, generator=gen) * 56
        maps = (10 * torch.exp(-((yy - c[..., 0, None, None]) ** 2 + (xx - c[..., 1, None, None]) ** 2) / 18)
                + 0.01 * torch.randn(n, K, 56, 56, generator=gen)).to(dev)
        xy, sc = ops.heatmaps_to_keypoints(maps, boxes)
        rxy, rsc = reference_loop(maps, boxes)
        same = ((xy - rxy).abs() <= 1e-3 * (1 + rxy.abs())).all(-1)
        agree = float(same.float().mean())
        gap = near_tie_gap(maps, boxes, xy, same)
        tail[str(n)] = {"pixels_per_map_mean": round(float(((boxes[:, 2] - boxes[:, 0]).ceil() * (boxes[:, 3] - boxes[:, 1]).ceil()).mean())),
                        "positions_agree": round(agree, 4), "differing_pairs": int((~same).sum()),
                        "largest_gap_at_a_differing_pair_over_max_map": gap, "kernel_ms": [], "reference_loop_ms": []}
        for _ in range(args.rounds):
            tail[str(n)]["kernel_ms"].append(round(timed(lambda: ops.heatmaps_to_keypoints(maps, boxes), 20), 4))
            tail[str(n)]["reference_loop_ms"].append(round(wall(lambda: reference_loop(maps, boxes), 1 if n > 100 else 3), 2))
    # ---- ingest
    tr = kmodel.transform
    tr.eval()
    shapes = [(480, 640), (427, 640), (640, 480), (500, 375)][:args.batch]
    u8 = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=gen) for h, w in shapes]
    tg_cpu = [{k: v.cpu() for k, v in t.items()} for t in persons(len(shapes), 375, args.gt, K, gen, "cpu")]
    no_kp = [{k: v for k, v in t.items() if k != "keypoints"} for t in tg_cpu]
    flips = [True, False, True, False][:len(shapes)]
    ingest = {"with_keypoints_ms": [], "boxes_only_ms": [], "keypoint_launch_us": []}
    il, tg_dev = tr.ingest(u8, tg_cpu, flips)
    kps = torch.cat([t["keypoints"] for t in tg_cpu]).to(dev)
    from object_detectors_amd._lib import IngestImage, check, lib, ptr, stream_ptr
    import ctypes
    table = (IngestImage * len(shapes))(*[IngestImage(0, h, w, oh, ow, int(f), 0) for (h, w), (oh, ow), f in zip(shapes, il.image_sizes, flips)])
    table_dev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev)
    offs = torch.tensor([args.gt * i for i in range(len(shapes) + 1)], dtype=torch.int64, device=dev)
    out = torch.empty_like(kps)

    def launch():
        check(lib().mi355det_flip_resize_keypoints(ptr(kps), ptr(out), kps.shape[0], K, ptr(offs), ctypes.cast(table, ctypes.c_void_p),
                                                   ctypes.c_void_p(table_dev.data_ptr()), len(shapes),
                                                   stream_ptr()), "flip_resize_keypoints")
    for _ in range(args.rounds):
        ingest["with_keypoints_ms"].append(round(wall(lambda: tr.ingest(u8, tg_cpu, flips), 20), 3))
        ingest["boxes_only_ms"].append(round(wall(lambda: tr.ingest(u8, no_kp, flips), 20), 3))
        ingest["keypoint_launch_us"].append(round(1e3 * timed(launch, 200), 2))
    res = {"metric": "keypointrcnn_resnet50_fpn", "routes": args.routes, "extra_streams": len(idle), "batch": args.batch, "px": P, "persons_per_image": args.gt, "steps_per_window": args.steps,
           "rounds": rounds, "keypoint_rows_last_step": rows_seen, "eval_tail": tail, "ingest": ingest}
    print(json.dumps(res))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n### `tools/bench_keypointrcnn.py` " + " ".join(sys.argv[1:]) + "\n\n")
            f.write("| round | Faster R-CNN step (ms) | Keypoint R-CNN step (ms) | branch (ms) | the same by device events on the step's stream |\n|---|---|---|---|---|\n")
            for i, r in enumerate(rounds):
                fr = r.get("faster_rcnn_step_ms", float("nan"))
                f.write(f"| {i} | {fr} | {r['keypoint_rcnn_step_ms']} | {r['keypoint_rcnn_step_ms'] - fr:.3f} | "
                        f"{r.get('faster_rcnn_step_ms_events')} / {r['keypoint_rcnn_step_ms_events']} |\n")
            f.write(f"\nKeypoint rows of the last step: {rows_seen}.\n\n| detections | mean pixels per upsampled map | kernel (ms), per round | reference loop on the device (ms), per round | positions agree |\n|---|---|---|---|---|\n")
            for n, t in tail.items():
                f.write(f"| {n} | {t['pixels_per_map_mean']} | {t['kernel_ms']} | {t['reference_loop_ms']} | {t['positions_agree']} |\n")
            f.write(f"\nIngest of {len(shapes)} images, {args.gt} persons each, host clock around a synchronise, per round: with keypoints "
                    f"{ingest['with_keypoints_ms']} ms, boxes only {ingest['boxes_only_ms']} ms; the keypoint launch alone (device events) "
                    f"{ingest['keypoint_launch_us']} us.\n")


if __name__ == "__main__":
    main()
