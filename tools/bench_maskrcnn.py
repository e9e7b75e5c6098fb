#!/usr/bin/env python3
"""Mask R-CNN ResNet-50-FPN (tvision/mask_rcnn.py), synthetic COCO 800 px with synthetic instance masks: training step time, inference time
per image, and the time of each mask-branch section (device events around the sections, run on the last step's RoIs).
    python tools/bench_maskrcnn.py --batch 4 --steps 10
Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--px", type=int, default=800)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--gt", type=int, default=7, help="instances per image")
    ap.add_argument("--full-rows", type=int, default=None, help="also time the sections at this many rows (the last step's RoIs tiled; "
                    "default box_batch_size_per_image * positive_fraction * batch = 128 * batch, the largest bucket)")
    args = ap.parse_args()
    from object_detectors_amd import ops
    from object_detectors_amd.optim import FlatSGD
    from object_detectors_amd.parallel import step_stream
    from object_detectors_amd.tvision.mask_rcnn import _rows_for, maskrcnn_resnet50_fpn
    dev = torch.device("cuda:0")
    torch.cuda.set_stream(step_stream(dev))
    torch.manual_seed(0)
    model = maskrcnn_resnet50_fpn(num_classes=91, device=dev)
    eng = model.engine
    for sp in eng.specs:          # stable random-init residual stack (tools/bench_frcnn.py)
        if sp.bn and sp.bn.endswith(".bn3"):
            eng.buffers[sp.bn + ".weight"].fill_(0.2)
    eng.refresh_frozen()
    opt = FlatSGD.for_engine(eng, lr=1e-2, momentum=0.9, weight_decay=1e-4)
    opt_head = torch.optim.SGD(model.head_parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(0)
    P, G = args.px, args.gt
    imgs = torch.rand((args.batch, 3, P, P), generator=g).to(dev)
    yy, xx = torch.meshgrid(torch.arange(P, dtype=torch.float32), torch.arange(P, dtype=torch.float32), indexing="ij")
    targets = []
    for _ in range(args.batch):
        tl = torch.rand((G, 2), generator=g) * P * 0.6
        wh = torch.rand((G, 2), generator=g) * P * 0.3 + 16
        boxes = torch.cat([tl, tl + wh], 1)
        c, r = (boxes[:, :2] + boxes[:, 2:]) / 2, wh / 2
        masks = ((((xx[None] - c[:, 0, None, None]) / r[:, 0, None, None]) ** 2 + ((yy[None] - c[:, 1, None, None]) / r[:, 1, None, None]) ** 2)
                 <= 1.0).to(torch.uint8)
        targets.append({"boxes": boxes.to(dev), "labels": torch.randint(1, 91, (G,), generator=g).to(dev), "masks": masks.to(dev)})
    model.train()
    model.keep_mask_inputs = True

    def step():
        opt_head.zero_grad(set_to_none=True)
        losses = model(imgs, targets)
        opt.step()
        opt_head.step()
        return losses
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(args.steps):
        losses = step()
    e.record()
    e.synchronize()
    step_ms = s.elapsed_time(e) / args.steps
    # ---- mask-branch sections on the last step's inputs (same bucket)
    mi = model.last_mask_inputs
    r = mi["rois"].shape[0]
    rows = _rows_for(r)
    pad = lambda t: torch.cat([t, t[:1].expand(rows - r, *t.shape[1:])]) if rows > r else t
    rois, gt, lab = pad(mi["rois"]).contiguous(), pad(mi["gt_index"]).contiguous(), pad(mi["labels"]).contiguous()
    feats = eng.feature_maps_nhwc(4)
    shapes = [(P, P)] * args.batch
    lv = model.mask_roi_pool.levels_nhwc(feats, shapes)
    masks = [t["masks"] for t in targets]
    lg = model.mask_predictor.mask_fcn_logits
    wl = lg.weight.detach().reshape(91, 256)

    def sections(rois, gt, lab, r, reps=20):
        sec = {}
        sec["targets"] = timed(lambda: ops.mask_targets(masks, rois, gt, 28, num_rois=r), reps)
        sec["roi_pool"] = timed(lambda: ops.mask_roi_pool(feats, rois, *lv), reps)
        sec["forward_pool_convs_deconv"] = timed(lambda: model._mask_forward(feats, rois, shapes), reps)
        acts, z, _ = model._mask_forward(feats, rois, shapes)
        tgt = ops.mask_targets(masks, rois, gt, 28, num_rois=r)
        sec["loss_fused"] = timed(lambda: ops.mask_loss(z, wl, lg.bias.detach(), lab, tgt, r), reps)
        sec["backward_total"] = timed(lambda: model._mask_backward(feats, rois, acts, z, lv, lab, tgt, r), reps)
        for p in model.head_parameters():
            p.grad = None
        return {k: round(v, 3) for k, v in sec.items()}
    sec = sections(rois, gt, lab, r)
    full = args.full_rows or 128 * args.batch
    idx = torch.arange(full, device=dev) % r
    sec_full = sections(mi["rois"][idx].contiguous(), mi["gt_index"][idx].contiguous(), mi["labels"][idx].contiguous(), full)
    # ---- inference per image
    model.eval()
    with torch.no_grad():
        for _ in range(2):
            model(imgs)
        torch.cuda.synchronize()
        s.record()
        for _ in range(args.steps):
            det = model(imgs)
        e.record()
        e.synchronize()
    infer_ms = s.elapsed_time(e) / args.steps / args.batch
    flop_conv = 2.0 * rows * 196 * 256 * 256 * 9
    flop_deconv = 2.0 * rows * 196 * 1024 * 256
    print(json.dumps({"metric": "maskrcnn_resnet50_fpn", "batch": args.batch, "px": P, "train_step_ms": round(step_ms, 3),
                      "infer_ms_per_image": round(infer_ms, 3), "mask_rows": r, "mask_bucket_rows": rows,
                      "mask_sections_ms": sec, "mask_branch_fwd_gflop": round((4 * flop_conv + flop_deconv) / 1e9, 1),
                      "full_rows": full, "mask_sections_full_ms": sec_full,
                      "mask_branch_fwd_gflop_full": round(full / rows * (4 * flop_conv + flop_deconv) / 1e9, 1),
                      "loss_mask": float(losses["loss_mask"]), "detections": [int(d["boxes"].shape[0]) for d in det]}))


if __name__ == "__main__":
    main()
