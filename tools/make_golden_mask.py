#!/usr/bin/env python3
"""Generate tests/golden/g16_maskrcnn.npz by running the REFERENCE's own mask-branch functions on small seeded cases.

    python tools/make_golden_mask.py

Follows tools/make_golden.py (g13): the reference tree is imported as-is under permissive torchvision stubs; torchvision's own ops are
restated - roi_align by tests/mask_oracle.py, misc_nn_ops.interpolate aliased to F.interpolate.  What runs is the reference's
project_masks_on_boxes, maskrcnn_loss, maskrcnn_inference, expand_masks / expand_boxes / paste_masks_in_image and the masks parts of
_resize_image_and_masks and GeneralizedRCNNTransform.postprocess.  Cases: boxes partly outside the image, sub-pixel boxes, R = 0, several
images.  Arrays only (np.load(allow_pickle=False))."""
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import make_golden  # noqa: E402
from tests import mask_oracle as mo  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g16_maskrcnn.npz")


def main():
    make_golden.stub_torchvision_permissive()
    tv = sys.modules["torchvision"]
    tv._is_tracing = lambda: False
    sys.modules["torchvision.ops"].roi_align = mo.roi_align_torch
    from tvision import roi_heads, transform
    roi_heads.roi_align = mo.roi_align_torch
    roi_heads.misc_nn_ops.interpolate = F.interpolate
    rng = np.random.default_rng(16)
    d = {}
    # ---- targets + loss: 3 images, masks of different sizes; boxes partly outside, sub-pixel boxes
    sizes = [(40, 56), (33, 47), (64, 30)]
    gts = [mo.synth_masks(160 + i, g, h, w) for i, (g, (h, w)) in enumerate(zip((3, 2, 4), sizes))]
    props, mis, labs = [], [], []
    for i, (h, w) in enumerate(sizes):
        r = 6 + 2 * i
        x1 = rng.uniform(-10, w, r).astype(np.float32)
        y1 = rng.uniform(-10, h, r).astype(np.float32)
        bw = rng.uniform(0.2, w * 0.8, r).astype(np.float32)
        bh = rng.uniform(0.2, h * 0.8, r).astype(np.float32)
        bw[:2] = rng.uniform(0.05, 0.9, 2)                     # sub-pixel boxes
        bh[:2] = rng.uniform(0.05, 0.9, 2)
        props.append(np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32))
        mis.append(rng.integers(0, gts[i].shape[0], r).astype(np.int64))
        labs.append(rng.integers(1, 7, gts[i].shape[0]).astype(np.int64))
    K = 7
    R = sum(p.shape[0] for p in props)
    logits = torch.from_numpy(np.random.default_rng(1601).normal(0, 2, (R, K, 28, 28)).astype(np.float32)).requires_grad_(True)
    loss = roi_heads.maskrcnn_loss(logits, [torch.from_numpy(p) for p in props], [torch.from_numpy(g) for g in gts],
                                   [torch.from_numpy(l) for l in labs], [torch.from_numpy(m) for m in mis])
    loss.backward()
    tg = torch.cat([roi_heads.project_masks_on_boxes(torch.from_numpy(g), torch.from_numpy(p), torch.from_numpy(m), 28)
                    for g, p, m in zip(gts, props, mis)])
    for i in range(3):
        d[f"gt_masks{i}"], d[f"props{i}"], d[f"matched{i}"], d[f"gt_labels{i}"] = gts[i], props[i], mis[i], labs[i]
    # the logits are regenerated from their seed by the tests; the gradient is stored for the label channel (zero elsewhere, checked here)
    lab_all = np.concatenate([labs[i][mis[i]] for i in range(3)])
    g = logits.grad.numpy()
    gl = g[np.arange(R), lab_all].copy()
    g[np.arange(R), lab_all] = 0
    assert not g.any()
    d["logits_seed_k"], d["targets"], d["loss"], d["grad_label"] = np.array([1601, K]), tg.numpy(), np.float64(float(loss.detach())), gl
    # ---- R = 0
    z = torch.zeros((0, K, 28, 28), requires_grad=True)
    l0 = roi_heads.maskrcnn_loss(z, [torch.zeros((0, 4))], [torch.from_numpy(gts[0])], [torch.from_numpy(labs[0])], [torch.zeros(0, dtype=torch.int64)])
    d["loss_r0"] = np.float64(float(l0))
    # ---- inference: maskrcnn_inference + paste (through postprocess of the transform) on two images
    x = torch.from_numpy(np.random.default_rng(1602).normal(0, 2, (9, K, 28, 28)).astype(np.float32))
    det_labels = [torch.from_numpy(rng.integers(1, K, 5).astype(np.int64)), torch.from_numpy(rng.integers(1, K, 4).astype(np.int64))]
    probs = roi_heads.maskrcnn_inference(x, det_labels)
    im_shapes, orig = [(48, 64), (40, 36)], [(96, 128), (50, 45)]
    result = []
    for i, (c, (h, w)) in enumerate(zip((5, 4), im_shapes)):
        x1 = rng.uniform(-6, w - 4, c).astype(np.float32)
        y1 = rng.uniform(-6, h - 4, c).astype(np.float32)
        b = np.stack([x1, y1, x1 + rng.uniform(0.3, w * 0.7, c), y1 + rng.uniform(0.3, h * 0.7, c)], 1).astype(np.float32)
        b[-1] = [w - 3.3, h - 2.2, w + 5.0, h + 4.0]                # past the lower-right corner
        result.append({"boxes": torch.from_numpy(b), "labels": det_labels[i], "masks": probs[i]})
        d[f"det_boxes{i}"], d[f"det_labels{i}"] = b, det_labels[i].numpy()
    d["det_logits_seed"] = np.array([1602])
    for i in range(2):
        d[f"det_probs{i}"] = probs[i].numpy()
    ns = types.SimpleNamespace(training=False)
    post = transform.GeneralizedRCNNTransform.postprocess(ns, result, im_shapes, orig)
    for i, r in enumerate(post):
        d[f"post_boxes{i}"], d[f"post_masks{i}"] = r["boxes"].numpy(), r["masks"].numpy()
    # paste on its own, expand_* included, at image size
    pm = torch.from_numpy(rng.uniform(0, 1, (4, 1, 28, 28)).astype(np.float32))
    pb = torch.from_numpy(np.array([[-3.7, -2.1, 10.2, 9.9], [5.5, 6.25, 5.75, 6.5], [20.0, 3.0, 39.9, 30.1], [0.0, 0.0, 1.0, 1.0]], np.float32))
    d["paste_masks"], d["paste_boxes"] = pm.numpy(), pb.numpy()
    d["paste_out"] = roi_heads.paste_masks_in_image(pm, pb, (32, 40), padding=1).numpy()
    em, sc = roi_heads.expand_masks(pm, 1)
    d["expand_scale"] = np.float64(sc)
    d["expand_boxes"] = roi_heads.expand_boxes(pb, sc).numpy()
    # ---- masks part of _resize_image_and_masks: up, down, non-integer scales
    for j, ((h, w), (mn, mx)) in enumerate([((40, 56), (80.0, 1333.0)), ((33, 47), (20.0, 1333.0)), ((64, 30), (45.0, 70.0)), ((50, 50), (100.0, 1333.0))]):
        img = torch.zeros(3, h, w)
        m = torch.from_numpy(mo.synth_masks(170 + j, 3, h, w))
        _img, tgt = transform._resize_image_and_masks(img, mn, mx, {"masks": m})
        d[f"resize_in{j}"], d[f"resize_out{j}"], d[f"resize_minmax{j}"] = m.numpy(), tgt["masks"].numpy(), np.array([mn, mx], np.float64)
    np.savez_compressed(OUT, **d)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
