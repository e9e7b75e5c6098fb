#!/usr/bin/env python3
"""Generate tests/golden/g18_keypoint_rcnn.npz by running the REFERENCE's own keypoint functions on small seeded cases.

    python tools/make_golden_keypoint.py

Follows tools/make_golden_mask.py: the reference tree is imported as-is under tools/make_golden.py's permissive torchvision stubs, with
torchvision._is_tracing() false.  What runs is the reference's keypoints_to_heatmap, keypointrcnn_loss (value and autograd gradient with
respect to the logits), heatmaps_to_keypoints, keypointrcnn_inference (tvision/roi_heads.py), resize_keypoints (tvision/transform.py) and
_flip_coco_person_keypoints (detection/transforms.py).  Data only: small inputs and the reference's outputs; the heatmaps come from
oracle.detrand by seed and are not stored.  Arrays only (np.load(allow_pickle=False))."""
import os
import sys

import numpy as np
import torch

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden  # noqa: E402
from oracle import detrand  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g18_keypoint_rcnn.npz")
K, S = 17, 56
LOGITS_SEED, MAPS_SEED, INFER_SEED = 1801, 1802, 1803


def target_case(rng):
    """Two images (3 and 2 persons), 24 RoIs: keypoints inside, on the RoI's right / bottom edge, outside the RoI, v = 0, a row with none
    valid."""
    gts, props, mis = [], [], []
    for i, (g, r) in enumerate(((3, 14), (2, 10))):
        x1 = rng.uniform(5, 60, r).astype(np.float32)
        y1 = rng.uniform(5, 60, r).astype(np.float32)
        p = np.stack([x1, y1, x1 + rng.uniform(8, 50, r).astype(np.float32), y1 + rng.uniform(8, 50, r).astype(np.float32)], 1).astype(np.float32)
        mi = rng.integers(0, g, r).astype(np.int64)
        kp = np.zeros((g, K, 3), np.float32)
        kp[..., 0] = rng.uniform(0, 120, (g, K))
        kp[..., 1] = rng.uniform(0, 120, (g, K))
        kp[..., 2] = rng.integers(0, 3, (g, K))
        # RoI 0 of the image takes its corners from keypoints of its matched person: keypoint 0 at the top-left corner (index 0), keypoint 1
        # on the right edge, keypoint 2 on the bottom edge, keypoint 3 on both
        j = mi[0]
        kp[j, :4, 2] = 2
        p[0] = [kp[j, 0, 0], kp[j, 0, 1], kp[j, 0, 0] + 30.5, kp[j, 0, 1] + 21.25]
        kp[j, 1, 0], kp[j, 1, 1] = p[0, 2], p[0, 1] + 3.0
        kp[j, 2, 0], kp[j, 2, 1] = p[0, 0] + 7.0, p[0, 3]
        kp[j, 3, 0], kp[j, 3, 1] = p[0, 2], p[0, 3]
        # RoI 1: far away from every keypoint -> a row with none valid
        p[1] = [500.0, 400.0, 530.0, 470.0]
        # RoI 2: wraps its whole person, so most visible keypoints land inside
        j = mi[2]
        p[2] = [kp[j, :, 0].min() - 1.5, kp[j, :, 1].min() - 0.75, kp[j, :, 0].max() + 2.25, kp[j, :, 1].max() + 1.0]
        gts.append(kp)
        props.append(p.astype(np.float32))
        mis.append(mi)
    return gts, props, mis


def main():
    make_golden.stub_torchvision_permissive()
    for name in ("torchvision.transforms", "torchvision.transforms.functional", "torchvision.transforms.transforms"):
        sys.modules[name] = make_golden._Permissive(name)
    sys.modules["torchvision"]._is_tracing = lambda: False
    from tvision import roi_heads, transform
    from detection import transforms as det_transforms
    assert not sys.modules["torchvision"]._is_tracing()
    rng = np.random.default_rng(18)
    d = {"seeds": np.array([LOGITS_SEED, MAPS_SEED, INFER_SEED])}

    # ---- keypoints_to_heatmap + keypointrcnn_loss
    gts, props, mis = target_case(rng)
    heat, valid = [], []
    for kp, p, mi in zip(gts, props, mis):
        h, v = roi_heads.keypoints_to_heatmap(torch.from_numpy(kp)[torch.from_numpy(mi)], torch.from_numpy(p), S)
        heat.append(h.numpy())
        valid.append(v.numpy())
    for i in range(2):
        d[f"gt_keypoints{i}"], d[f"props{i}"], d[f"matched{i}"] = gts[i], props[i], mis[i]
    d["target"], d["valid"] = np.concatenate(heat).astype(np.int64), np.concatenate(valid).astype(np.int64)
    assert d["valid"][1].sum() == 0 and d["valid"][14 + 1].sum() == 0 and d["valid"].sum() > 40
    assert d["target"][0, 0] == 0 and d["target"][0, 1] % S == S - 1 and d["target"][0, 2] // S == S - 1 and d["target"][0, 3] == S * S - 1
    rows = d["target"].shape[0]
    logits = torch.from_numpy(detrand.uniform(LOGITS_SEED, (rows, K, S, S), -4.0, 4.0)).requires_grad_(True)
    loss = roi_heads.keypointrcnn_loss(logits, [torch.from_numpy(p) for p in props], [torch.from_numpy(g) for g in gts],
                                       [torch.from_numpy(m) for m in mis])
    loss.backward()
    # the gradient is zero on the pairs that are not valid (checked here).  All of it would be 1.3 MB, so the fixture keeps, per valid pair,
    # its value at the target, its largest magnitude and its value at one drawn index
    g = logits.grad.reshape(rows * K, S * S).numpy()
    vflat = d["valid"].reshape(-1).astype(bool)
    assert not g[~vflat].any()
    d["loss"] = np.float32(loss.detach().numpy())
    d["grad_at_target"] = g[np.arange(rows * K), d["target"].reshape(-1)][vflat]
    d["grad_absmax"] = np.abs(g[vflat]).max(1)
    d["grad_probe_index"] = rng.integers(0, S * S, int(vflat.sum())).astype(np.int64)
    d["grad_probe"] = g[vflat][np.arange(int(vflat.sum())), d["grad_probe_index"]]
    # all pairs invalid, and no RoI at all: keypoint_logits.sum() * 0
    kp0 = gts[0].copy()
    kp0[..., 2] = 0
    l0 = roi_heads.keypointrcnn_loss(logits[:14], [torch.from_numpy(props[0])], [torch.from_numpy(kp0)], [torch.from_numpy(mis[0])])
    lz = roi_heads.keypointrcnn_loss(torch.zeros((0, K, S, S)), [torch.zeros((0, 4))], [torch.from_numpy(gts[0])], [torch.zeros(0, dtype=torch.int64)])
    d["loss_all_invalid"], d["loss_r0"] = np.float32(float(l0.detach())), np.float32(float(lz))

    # ---- heatmaps_to_keypoints: RoIs whose sizes ceil to 1x1 (a width below 1), thin, the map's own size, larger, non-square
    sizes = [(0.4, 0.7), (7.3, 2.6), (2.2, 7.9), (56.0, 56.0), (55.2, 111.5), (130.6, 199.1), (40.0, 23.0), (90.01, 17.5)]
    x1 = rng.uniform(-5, 200, len(sizes)).astype(np.float32)
    y1 = rng.uniform(-5, 200, len(sizes)).astype(np.float32)
    rois = np.stack([x1, y1, x1 + np.array([s[0] for s in sizes], np.float32), y1 + np.array([s[1] for s in sizes], np.float32)], 1).astype(np.float32)
    maps = torch.from_numpy(detrand.uniform(MAPS_SEED, (len(sizes), K, S, S), -4.0, 4.0))
    xy, sc = roi_heads.heatmaps_to_keypoints(maps, torch.from_numpy(rois))
    d["h2k_rois"], d["h2k_xy"], d["h2k_scores"] = rois, xy.numpy().copy(), sc.numpy()

    # ---- keypointrcnn_inference on two images (5 and 4 detections), then the transform's postprocess (resize_keypoints)
    boxes = []
    for c, (h, w) in zip((5, 4), ((48, 64), (40, 36))):
        bx = rng.uniform(0, w - 12, c).astype(np.float32)
        by = rng.uniform(0, h - 12, c).astype(np.float32)
        boxes.append(np.stack([bx, by, bx + rng.uniform(2, w * 0.6, c).astype(np.float32), by + rng.uniform(2, h * 0.6, c).astype(np.float32)], 1)
                     .astype(np.float32))
    x = torch.from_numpy(detrand.uniform(INFER_SEED, (9, K, S, S), -4.0, 4.0))
    probs, scores = roi_heads.keypointrcnn_inference(x, [torch.from_numpy(b) for b in boxes])
    im_shapes, orig = [(48, 64), (40, 36)], [(96, 130), (50, 45)]
    for i in range(2):
        d[f"det_boxes{i}"], d[f"det_xy{i}"], d[f"det_scores{i}"] = boxes[i], probs[i].numpy().copy(), scores[i].numpy()
        d[f"post_xy{i}"] = transform.resize_keypoints(probs[i], im_shapes[i], orig[i]).numpy()
    d["det_image_shapes"], d["det_original_sizes"] = np.array(im_shapes), np.array(orig)

    # ---- resize_keypoints + _flip_coco_person_keypoints on person-like targets (some v = 0)
    for j, ((h, w), (nh, nw)) in enumerate([((480, 640), (800, 1066)), ((333, 500), (704, 1057)), ((37, 53), (128, 183))]):
        g = 2 + j
        kp = np.zeros((g, K, 3), np.float32)
        kp[..., 0] = rng.uniform(0, w, (g, K))
        kp[..., 1] = rng.uniform(0, h, (g, K))
        kp[..., 2] = rng.integers(0, 3, (g, K))
        kp[kp[..., 2] == 0] = 0
        d[f"tf_in{j}"], d[f"tf_sizes{j}"] = kp, np.array([h, w, nh, nw])
        d[f"tf_resized{j}"] = transform.resize_keypoints(torch.from_numpy(kp), (h, w), (nh, nw)).numpy()
        flipped = det_transforms._flip_coco_person_keypoints(torch.from_numpy(kp.copy()), w)
        d[f"tf_flipped{j}"] = flipped.numpy().copy()
        d[f"tf_flipped_resized{j}"] = transform.resize_keypoints(flipped, (h, w), (nh, nw)).numpy()
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
