"""numpy / torch-CPU restatement of the Mask R-CNN mask-branch ops (tvision/roi_heads.py:99-183,403-537, tvision/transform.py:26-62,228-247),
in float32 with the operation order of the CPU kernels they stand for.  tests/test_oracle_mask.py pins it to the reference's own functions
(tests/golden/g16_maskrcnn.npz, tools/make_golden_mask.py); tests/test_gpu_mask.py holds the HIP kernels to it."""
import numpy as np
import torch
import torch.nn.functional as F

f32 = np.float32


def roi_align(inp, rois, out_hw, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
    """torchvision.ops.roi_align (CPU kernel) on inp [N, C, H, W] float32, rois [K, 5] -> [K, C, ph, pw] float32."""
    inp = np.asarray(inp, f32)
    rois = np.asarray(rois, f32)
    ph, pw = out_hw
    N, Cc, H, W = inp.shape
    out = np.zeros((rois.shape[0], Cc, ph, pw), f32)
    off = f32(0.5) if aligned else f32(0.0)
    sc = f32(spatial_scale)
    for k in range(rois.shape[0]):
        b = int(rois[k, 0])
        x1, y1, x2, y2 = (rois[k, 1] * sc - off, rois[k, 2] * sc - off, rois[k, 3] * sc - off, rois[k, 4] * sc - off)
        rw, rh = f32(x2 - x1), f32(y2 - y1)
        if not aligned:
            rw, rh = max(rw, f32(1.0)), max(rh, f32(1.0))
        bh, bw = f32(rh / f32(ph)), f32(rw / f32(pw))
        gh = sampling_ratio if sampling_ratio > 0 else int(np.ceil(f32(rh / f32(ph))))
        gw = sampling_ratio if sampling_ratio > 0 else int(np.ceil(f32(rw / f32(pw))))
        cnt = f32(max(gh * gw, 1))
        for py in range(ph):
            for px in range(pw):
                acc = np.zeros(Cc, f32)
                for iy in range(gh):
                    y = f32(f32(y1 + f32(f32(py) * bh)) + f32(f32(f32(iy) + f32(0.5)) * bh) / f32(gh))
                    for ix in range(gw):
                        x = f32(f32(x1 + f32(f32(px) * bw)) + f32(f32(f32(ix) + f32(0.5)) * bw) / f32(gw))
                        if y < -1.0 or y > H or x < -1.0 or x > W:
                            continue
                        yy, xx = max(y, f32(0)), max(x, f32(0))
                        yl, xl = int(yy), int(xx)
                        if yl >= H - 1:
                            yh = yl = H - 1
                            yy = f32(yl)
                        else:
                            yh = yl + 1
                        if xl >= W - 1:
                            xh = xl = W - 1
                            xx = f32(xl)
                        else:
                            xh = xl + 1
                        ly, lx = f32(yy - f32(yl)), f32(xx - f32(xl))
                        hy, hx = f32(f32(1) - ly), f32(f32(1) - lx)
                        w1, w2, w3, w4 = hy * hx, hy * lx, ly * hx, ly * lx
                        v = inp[b, :, yl, xl] * w1 + inp[b, :, yl, xh] * w2
                        v = v + inp[b, :, yh, xl] * w3
                        v = v + inp[b, :, yh, xh] * w4
                        acc = acc + v
                out[k, :, py, px] = acc / cnt
    return out


def roi_align_torch(inp, boxes, output_size, spatial_scale=1.0, sampling_ratio=-1, aligned=False):
    """The same with torchvision's signature on torch tensors (rois [K,5] or a list of [Ki,4])."""
    if isinstance(boxes, (list, tuple)):
        boxes = torch.cat([torch.cat([torch.full((b.shape[0], 1), float(i)), b], 1) for i, b in enumerate(boxes)])
    hw = (output_size, output_size) if isinstance(output_size, int) else tuple(output_size)
    return torch.from_numpy(roi_align(inp.detach().float().numpy(), boxes.detach().float().numpy(), hw, spatial_scale, sampling_ratio, aligned))


def project_masks_on_boxes(gt_masks, boxes, matched_idxs, M=28):
    """roi_heads.py:131-144 -> [R, M, M] float32."""
    rois = np.concatenate([np.asarray(matched_idxs, f32)[:, None], np.asarray(boxes, f32)], 1)
    return roi_align(np.asarray(gt_masks, f32)[:, None], rois, (M, M), 1.0)[:, 0]


def maskrcnn_loss(mask_logits, labels, targets):
    """roi_heads.py:147-183 on concatenated labels / targets: (loss, d loss / d mask_logits) via torch CPU autograd."""
    x = torch.as_tensor(np.asarray(mask_logits, f32)).clone().requires_grad_(True)
    lab = torch.as_tensor(np.asarray(labels, np.int64))
    t = torch.as_tensor(np.asarray(targets, f32))
    if t.numel() == 0:
        loss = x.sum() * 0
    else:
        loss = F.binary_cross_entropy_with_logits(x[torch.arange(lab.shape[0]), lab], t)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def nearest_index(out_size, in_size):
    if out_size == in_size:
        return np.arange(out_size)
    if out_size == 2 * in_size:
        return np.arange(out_size) >> 1
    scale = f32(in_size) / f32(out_size)
    return np.minimum(np.floor(np.arange(out_size).astype(f32) * scale).astype(np.int64), in_size - 1)


def resize_masks_nearest(masks, size):
    """F.interpolate(masks[:, None].float(), size, mode='nearest')[:, 0].byte()."""
    m = np.asarray(masks, np.uint8)
    iy, ix = nearest_index(size[0], m.shape[1]), nearest_index(size[1], m.shape[2])
    return m[:, iy][:, :, ix]


def expand_boxes(boxes, scale):
    b = np.asarray(boxes, f32)
    w_half = (b[:, 2] - b[:, 0]) * f32(0.5)
    h_half = (b[:, 3] - b[:, 1]) * f32(0.5)
    x_c = (b[:, 2] + b[:, 0]) * f32(0.5)
    y_c = (b[:, 3] + b[:, 1]) * f32(0.5)
    w_half = w_half * f32(scale)
    h_half = h_half * f32(scale)
    return np.stack([x_c - w_half, y_c - h_half, x_c + w_half, y_c + h_half], 1).astype(f32)


def _lin(out_size, in_size):
    scale = f32(in_size) / f32(out_size)
    src = scale * (np.arange(out_size).astype(f32) + f32(0.5)) - f32(0.5)
    src = np.maximum(src, f32(0))
    i0 = np.minimum(np.floor(src).astype(np.int64), in_size - 1)
    lam = np.clip(src - i0.astype(f32), f32(0), f32(1)).astype(f32)
    i1 = i0 + (i0 < in_size - 1)
    return i0, i1, (f32(1) - lam).astype(f32), lam


def resize_bilinear(m, h, w):
    """F.interpolate(m[None, None], size=(h, w), mode='bilinear', align_corners=False)[0, 0] in the CPU kernel's order."""
    y0, y1, wy0, wy1 = _lin(h, m.shape[0])
    x0, x1, wx0, wx1 = _lin(w, m.shape[1])
    t0 = m[y0][:, x0] * wx0[None] + m[y0][:, x1] * wx1[None]
    t1 = m[y1][:, x0] * wx0[None] + m[y1][:, x1] * wx1[None]
    return (t0 * wy0[:, None] + t1 * wy1[:, None]).astype(f32)


def paste_masks_in_image(masks, boxes, img_shape, padding=1):
    """roi_heads.py:403-537: masks [D, 1, M, M], boxes [D, 4] -> [D, 1, H, W] float32."""
    masks = np.asarray(masks, f32)
    D, M = masks.shape[0], masks.shape[-1]
    H, W = img_shape
    scale = float(M + 2 * padding) / M
    padded = np.pad(masks[:, 0], ((0, 0), (padding, padding), (padding, padding)))
    bx = expand_boxes(boxes, scale).astype(np.int64) if D else np.zeros((0, 4), np.int64)
    out = np.zeros((D, 1, H, W), f32)
    for d in range(D):
        b0, b1, b2, b3 = (int(v) for v in bx[d])
        w, h = max(b2 - b0 + 1, 1), max(b3 - b1 + 1, 1)
        r = resize_bilinear(padded[d], h, w)
        x0, x1, y0, y1 = max(b0, 0), min(b2 + 1, W), max(b1, 0), min(b3 + 1, H)
        if x1 > x0 and y1 > y0:
            out[d, 0, y0:y1, x0:x1] = r[y0 - b1:y1 - b1, x0 - b0:x1 - b0]
    return out


def synth_masks(seed, g, h, w):
    """Seeded uint8 instance masks: ellipses with random centres / radii (values 0 / 1)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    out = np.zeros((g, h, w), np.uint8)
    for i in range(g):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(2, max(3, h / 2)), rng.uniform(2, max(3, w / 2))
        out[i] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0).astype(np.uint8)
    return out
