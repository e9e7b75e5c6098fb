"""CPU restatement of the keypoint rules of Keypoint R-CNN, in torch float32 and the reference's operation order (tvision/roi_heads.py:186-379,
tvision/transform.py:260-275, detection/transforms.py:10-19).  tests/test_oracle_keypoint_rcnn.py holds it against
tests/golden/g18_keypoint_rcnn.npz, the reference's own outputs; the GPU tests then use it on other inputs.

Also the branch itself as an nn.Sequential (8 x Conv2d 3x3 + ReLU, ConvTranspose2d(512, K, 4, 2, 1), bilinear x2), with a switch that rounds
the activations to bf16 between layers: the storage-noise yardstick of the end-to-end test.  The layer shapes are torchvision's
KeypointRCNNHeads / KeypointRCNNPredictor written from memory (the reference does not contain keypoint_rcnn.py)."""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

FLIP_INDS = [0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15]


def keypoints_to_heatmap(keypoints, rois, size):
    """keypoints [R, K, 3] (already gathered per RoI), rois [R, 4] -> (index int64 [R, K], valid int64 [R, K])."""
    x1, y1, x2, y2 = (rois[:, i][:, None] for i in range(4))
    sx = size / (x2 - x1)
    sy = size / (y2 - y1)
    x, y = keypoints[..., 0], keypoints[..., 1]
    on_x2, on_y2 = x == x2, y == y2
    xi = ((x - x1) * sx).floor().long()
    yi = ((y - y1) * sy).floor().long()
    xi[on_x2] = size - 1
    yi[on_y2] = size - 1
    valid = ((xi >= 0) & (yi >= 0) & (xi < size) & (yi < size) & (keypoints[..., 2] > 0)).long()
    return (yi * size + xi) * valid, valid


def keypoint_targets(gt_keypoints, proposals, matched_idxs, size):
    """Per-image lists -> (index [sum R, K], valid [sum R, K]) over all images."""
    out = [keypoints_to_heatmap(kp[mi], p, size) for kp, p, mi in zip(gt_keypoints, proposals, matched_idxs)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


def keypointrcnn_loss(logits, proposals, gt_keypoints, matched_idxs):
    n, k, h, w = logits.shape
    target, valid = keypoint_targets(gt_keypoints, proposals, matched_idxs, h)
    sel = torch.nonzero(valid.reshape(-1)).squeeze(1)
    if target.numel() == 0 or sel.numel() == 0:
        return logits.sum() * 0
    return F.cross_entropy(logits.reshape(n * k, h * w)[sel], target.reshape(-1)[sel])


def heatmaps_to_keypoints(maps, rois):
    """maps [R, K, S, S], rois [R, 4] -> (xy [R, K, 3], scores [R, K]): one bicubic resize and arg-max per RoI."""
    r, k = maps.shape[:2]
    w = (rois[:, 2] - rois[:, 0]).clamp(min=1)
    h = (rois[:, 3] - rois[:, 1]).clamp(min=1)
    wc, hc = w.ceil(), h.ceil()
    xy = torch.zeros((r, k, 3), dtype=torch.float32)
    scores = torch.zeros((r, k), dtype=torch.float32)
    for i in range(r):
        ow, oh = int(wc[i].item()), int(hc[i].item())
        big = F.interpolate(maps[i][None], size=(oh, ow), mode="bicubic", align_corners=False)[0]
        pos = big.reshape(k, -1).argmax(dim=1)
        xi = pos % ow
        yi = (pos - xi) // ow
        xy[i, :, 0] = (xi.float() + 0.5) * (w[i] / ow) + rois[i, 0]
        xy[i, :, 1] = (yi.float() + 0.5) * (h[i] / oh) + rois[i, 1]
        xy[i, :, 2] = 1
        scores[i] = big[torch.arange(k), yi, xi]
    return xy, scores


def keypointrcnn_inference(maps, boxes):
    outs = [heatmaps_to_keypoints(m, b) for m, b in zip(maps.split([b.shape[0] for b in boxes]), boxes)]
    return [o[0] for o in outs], [o[1] for o in outs]


def resize_keypoints(keypoints, original_size, new_size):
    rh, rw = (torch.tensor(n, dtype=torch.float32) / torch.tensor(o, dtype=torch.float32) for n, o in zip(new_size, original_size))
    out = keypoints.clone()
    out[..., 0] *= rw
    out[..., 1] *= rh
    return out


def flip_coco_person_keypoints(kps, width):
    out = kps[:, FLIP_INDS]
    out[..., 0] = width - out[..., 0]
    out[out[..., 2] == 0] = 0
    return out


# ---- ConvTranspose2d(Cin, K, 4, stride 2, padding 1) as a 3x3 / padding 1 convolution to the four sub-pixel phases
def subpixel_weight(w, kp):
    """w [Cin, K, 4, 4] -> [4 * kp, Cin, 3, 3]: channel (2a + b) * kp + k is output pixel (2i + a, 2j + b); tap (dy, dx) of phase (a, b) holds
    w[:, k, a + 1 - 2 dy, b + 1 - 2 dx] where both indices fall in 0..3."""
    cin, k = w.shape[:2]
    w3 = torch.zeros(4, kp, cin, 3, 3, dtype=w.dtype)
    for a in range(2):
        for b in range(2):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    ky, kx = a + 1 - 2 * dy, b + 1 - 2 * dx
                    if 0 <= ky < 4 and 0 <= kx < 4:
                        w3[2 * a + b, :k, :, dy + 1, dx + 1] = w[:, :, ky, kx].t()
    return w3.reshape(4 * kp, cin, 3, 3)


def depth_to_space(z, k):
    """NCHW [R, 4 * kp, 14, 14] -> [R, k, 28, 28]."""
    r, c = z.shape[:2]
    kp = c // 4
    return z.reshape(r, 2, 2, kp, 14, 14)[:, :, :, :k].permute(0, 3, 4, 1, 5, 2).reshape(r, k, 28, 28)


def space_to_depth(g, kp):
    """[R, k, 28, 28] -> NHWC sub-pixel [R, 14, 14, 4 * kp] (zeros in the padded channels): the layout the kernels use."""
    r, k = g.shape[:2]
    out = torch.zeros(r, 14, 14, 2, 2, kp, dtype=g.dtype)
    out[..., :k] = g.reshape(r, k, 14, 2, 14, 2).permute(0, 2, 4, 3, 5, 1)
    return out.reshape(r, 14, 14, 4 * kp)


# ---- the branch
def bf16_round(x):
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


class Upsample2(nn.Module):
    def forward(self, x):
        return F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=False, recompute_scale_factor=False)


def branch(num_keypoints, dtype=torch.float64):
    layers, cin = [], 256
    for _ in range(8):
        layers += [nn.Conv2d(cin, 512, 3, padding=1), nn.ReLU()]
        cin = 512
    layers += [nn.ConvTranspose2d(512, num_keypoints, 4, stride=2, padding=1), Upsample2()]
    return nn.Sequential(*layers).to(dtype)


def run_branch(net, x, storage_rounding=False):
    """net(x); with storage_rounding the weights are used rounded to bf16, every ReLU output is rounded to bf16 (as the kernels store it)
    and - in the backward - so is the gradient that reaches each ReLU output."""
    if not storage_rounding:
        return net(x)

    class Round(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return bf16_round(t)

        @staticmethod
        def backward(ctx, g):
            return bf16_round(g)

    class RoundGrad(torch.autograd.Function):      # the 28 x 28 logits stay fp32; their gradient is stored in bf16
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g):
            return bf16_round(g)

    for m in net:
        if isinstance(m, nn.Conv2d):
            x = F.conv2d(x, bf16_round(m.weight.detach()) + (m.weight - m.weight.detach()), m.bias, padding=1)
        elif isinstance(m, nn.ConvTranspose2d):
            x = RoundGrad.apply(F.conv_transpose2d(x, bf16_round(m.weight.detach()) + (m.weight - m.weight.detach()), m.bias, stride=2, padding=1))
        elif isinstance(m, nn.ReLU):
            x = Round.apply(torch.relu(x))
        else:
            x = m(x)
    return x


def synth_persons(seed, px, num_images, num_keypoints=17):
    """3 + i persons in image i: boxes inside the px x px image, keypoints inside their box, about a fifth with v = 0 (x = y = 0, the COCO
    convention) and v in {1, 2} otherwise."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(num_images):
        g = 3 + i
        x1, y1 = rng.uniform(0, px - 48, g), rng.uniform(0, px - 48, g)
        bw, bh = rng.uniform(16, 46, g), rng.uniform(16, 46, g)
        boxes = np.stack([x1, y1, x1 + bw, y1 + bh], 1).astype(np.float32)
        kp = np.zeros((g, num_keypoints, 3), np.float32)
        kp[..., 0] = x1[:, None] + rng.uniform(0.05, 0.95, (g, num_keypoints)) * bw[:, None]
        kp[..., 1] = y1[:, None] + rng.uniform(0.05, 0.95, (g, num_keypoints)) * bh[:, None]
        kp[..., 2] = rng.integers(1, 3, (g, num_keypoints))
        kp[rng.uniform(0, 1, (g, num_keypoints)) < 0.2] = 0
        out.append({"boxes": boxes, "labels": np.ones(g, np.int64), "keypoints": kp})
    return out
