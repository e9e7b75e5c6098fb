"""Mirror of yolo/dsets/transformations.py: the input side of the YOLO step.

    sample = ResizeToTensor(640)((img, target))                   # the reference's per-sample form: img uint8 [H, W, 3] or [H, W]
    imgs, targets = ResizeToTensor(640).batch(images, targets, flips)      # a whole batch: one image launch, one box launch

`ResizeToTensor` is cv2.resize(img, (S, S), INTER_CUBIC), / 255, normalise and the box conversion of transformations.py:10-53.  The resize is
OpenCV's 8-bit fixed-point bicubic, restated in include/mi355det.h; it runs on the device (mi355det_yolo_ingest_u8) from the decoded bytes,
so a batch uploads its uint8 pixels instead of the float32 tensors the reference's loader concatenates.  What needs float arithmetic that
has to match numpy's is done here on the host and handed to the kernel as tables: the per-axis taps `cubic_taps(src, dst)`, cached per
pair, and the 768 normalised values of a byte (`normalised_bytes`).  The boxes go to relative xcycwh in float64 (mi355det_yolo_targets).
`COCO91_80` and `Class1_0` are the reference's label maps; `Augment` (imgaug) is not built."""
import ctypes
import functools

import numpy as np
import torch

from ..._lib import CubicTap, YoloImage
from ...tvision.transform import _Staging

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]        # transformations.py:39-40
TAP_DTYPE = np.dtype([("s", "<i4"), ("w", "<i2", (4,))])
assert TAP_DTYPE.itemsize == ctypes.sizeof(CubicTap)


@functools.lru_cache(maxsize=4096)
def cubic_taps(src, dst):
    """The (s, w0..w3) of every output index of one axis, source size `src` to `dst`: the rule of include/mi355det.h in its literal float32
    order (each numpy operation below rounds once to float32, as each C expression does).  A read-only array of TAP_DTYPE, cached."""
    src, dst = int(src), int(dst)
    if src <= 0 or dst <= 0:
        raise ValueError(f"cubic_taps: sizes must be > 0, got {src} -> {dst}")
    f32 = np.float32
    scale = 1.0 / (dst / float(src))
    fx = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(f32)
    s = np.floor(fx)
    fx = fx - s                                                          # float32
    A, one = f32(-0.75), f32(1)
    x1, x2 = fx + one, one - fx
    c0 = ((A * x1 - f32(5) * A) * x1 + f32(8) * A) * x1 - f32(4) * A
    c1 = ((A + f32(2)) * fx - (A + f32(3))) * fx * fx + one
    c2 = ((A + f32(2)) * x2 - (A + f32(3))) * x2 * x2 + one
    c3 = one - c0 - c1 - c2
    c = np.stack([c0, c1, c2, c3], 1)
    assert c.dtype == np.float32 and fx.dtype == np.float32
    out = np.empty(dst, TAP_DTYPE)
    out["s"] = s.astype(np.int32)
    out["w"] = np.clip(np.rint(c * f32(2048)), -32768, 32767).astype(np.int16)
    out.setflags(write=False)
    return out


def normalised_bytes():
    """float32 [3, 256]: the value of every byte in every channel, by the reference's own operations (transformations.py:36-41)."""
    img = np.broadcast_to(np.arange(256, dtype=np.uint8), (3, 1, 256))
    img = img / 255.0
    img = torch.from_numpy(img).float()
    mean = torch.tensor([[MEAN]]).permute(2, 1, 0)                    # the reference's `.T` of a [1, 1, 3] tensor
    std = torch.tensor([[STD]]).permute(2, 1, 0)
    img = (img - mean) / std
    return img.reshape(3, 256).contiguous()


def _checked_arguments(images, targets, flips):
    """The refusals of `ResizeToTensor.batch`, all on the host and ahead of any launch.  Returns the images as tensors, the targets' columns
    as host or device tensors (bbox float64 [G, 4], area float64 [G], category_id int64 [K], image_id int64) and one bool per image."""
    images = [torch.as_tensor(i) for i in images]
    n = len(images)
    if n == 0:
        raise ValueError("ResizeToTensor: images is empty")
    for img in images:
        if img.dtype != torch.uint8:
            raise TypeError(f"ResizeToTensor: expected uint8 images of shape [H, W, 3] or [H, W], but found type {img.dtype}")
        if img.dim() not in (2, 3) or (img.dim() == 3 and img.shape[-1] != 3) or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError("ResizeToTensor: images is expected to be a list of uint8 tensors of shape [H, W, 3] or [H, W], got {}".format(
                tuple(img.shape)))
    if any(img.device != images[0].device for img in images):
        raise ValueError("ResizeToTensor: the images are either all on the CPU or all on one device")
    flips = [False] * n if flips is None else [bool(f) for f in flips]
    if len(flips) != n:
        raise ValueError(f"ResizeToTensor: {len(flips)} flips for {n} images")
    columns = None
    if targets is not None:
        if len(targets) != n:
            raise ValueError(f"ResizeToTensor: {len(targets)} targets for {n} images")
        columns = []
        def f64(v):             # lists and arrays through numpy's float64: torch.as_tensor of a list of floats would round them to float32
            return v.to(torch.float64) if isinstance(v, torch.Tensor) else torch.from_numpy(np.asarray(v, dtype=np.float64))
        for t in targets:
            bbox = f64(t["bbox"])
            if bbox.numel() == 0:
                bbox = bbox.reshape(0, 4)
            if bbox.dim() != 2 or bbox.shape[-1] != 4:
                raise ValueError("Expected target bbox to be a tensor of shape [G, 4], got {:}.".format(tuple(bbox.shape)))
            area = f64(t["area"]).reshape(-1)
            if area.numel() != bbox.shape[0]:
                raise ValueError(f"ResizeToTensor: {area.numel()} areas for {bbox.shape[0]} boxes")
            columns.append({"bbox": bbox, "area": area, "category_id": torch.as_tensor(t["category_id"]).to(torch.int64).reshape(-1),
                            "image_id": torch.as_tensor(t["image_id"]).to(torch.int64)})
    return images, columns, flips


class ResizeToTensor(object):
    """
    Image: Resizes and normalizes it to predefined yolo dimensions. Also it transposes it and adds extra dimension for batch.
    BOXES: Transformes them from absolute X0Y0WH to yolo dimension relative XcYcWH -> range: [0, 1]
    Also it calculates bbox area and put it in the sample
    """
    _luts = {}           # device -> normalised_bytes() there
    _staging = {}        # device -> the pinned buffers of `batch`

    def __init__(self, scale):
        if int(scale) != scale or scale <= 0:
            raise ValueError(f"ResizeToTensor: scale must be a positive integer, got {scale}")
        self.scale = int(scale)

    def __call__(self, sample):
        """transformations.py:20-53: (img uint8 [H, W, 3] or [H, W], target) -> (float32 [1, 3, S, S], targets), on the device."""
        img, target = sample
        imgs, targets = self.batch([img], [target])
        return imgs, targets[0]

    def batch(self, images, targets=None, flips=None, device=None):
        """`__call__` for a list of images of any sizes (uint8 tensors or numpy arrays, all on the CPU or all on one device), one
        horizontal-flip flag per image (the project's own addition, as in `GeneralizedRCNNTransform.ingest`).  Returns
        (imgs float32 [n, 3, S, S], list of target dicts, or None without targets); the dicts hold the reference's keys and dtypes
        (bbox float32 [G, 4], img_size int64 [h, w, 3], category_id int64, area float64 [G], image_id int64) as views into one concatenated
        device tensor per key.  A target may have zero boxes.  CPU images are packed into a pinned buffer behind the image table and the
        tap tables and go up in one copy (to `device`, default the current one)."""
        from ... import ops
        images, columns, flips = _checked_arguments(images, targets, flips)
        n, S = len(images), self.scale
        src_dev = images[0].device
        if src_dev.type != "cpu":
            dev = src_dev
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

        # layout of the first buffer: image table | tap tables, one per (src, S) pair of the batch | the pixels (CPU images only)
        tap_at, tap_parts, ntaps = {}, [], 0
        table = (YoloImage * n)()
        offset = 0
        for i, img in enumerate(images):
            h, w = int(img.shape[0]), int(img.shape[1])
            for src in (w, h):
                if src not in tap_at:
                    tap_at[src] = ntaps
                    tap_parts.append(cubic_taps(src, S))
                    ntaps += S
            ch = 3 if img.dim() == 3 else 1
            table[i] = YoloImage(offset, h, w, ch, int(flips[i]), tap_at[w], tap_at[h])
            offset += h * w * ch
        nbytes = offset
        ntable = ctypes.sizeof(table)
        ntap_bytes = ntaps * TAP_DTYPE.itemsize
        head = -(-(ntable + ntap_bytes) // 16) * 16
        on_cpu = src_dev.type == "cpu"

        # layout of the second one, with targets only: box offsets | boxes | areas | category ids | image ids | image sizes
        if columns is not None:
            counts = [int(c["bbox"].shape[0]) for c in columns]
            box_offsets = torch.zeros(n + 1, dtype=torch.int64)
            box_offsets[1:] = torch.tensor(counts, dtype=torch.int64).cumsum(0)
            sizes = torch.tensor([[t.h, t.w, 3] for t in table], dtype=torch.int64)
            id_shapes = [c["image_id"].shape for c in columns]
            parts = [box_offsets] + [torch.cat([c[k].reshape(-1).to("cpu") for c in columns]) for k in ("bbox", "area", "category_id", "image_id")] + \
                    [sizes.reshape(-1)]
            nmeta = sum(p.numel() * 8 for p in parts)                # every column is 8 bytes wide: all stay aligned
        else:
            nmeta = 0

        with torch.cuda.device(dev):
            stage = self._staging.setdefault(dev, _Staging())
            pixels, meta = stage.acquire(head + (nbytes if on_cpu else 0), max(nmeta, 8))
            pixels[:ntable].copy_(torch.from_numpy(np.frombuffer(table, dtype=np.uint8)))
            at, pinned = ntable, pixels.numpy()
            for part in tap_parts:
                pinned[at:at + part.nbytes] = part.view(np.uint8)
                at += part.nbytes
            if on_cpu:
                for img, t in zip(images, table):
                    pixels[head + t.offset:head + t.offset + img.numel()].view(img.shape).copy_(img)
                up = torch.empty(head + nbytes, dtype=torch.uint8, device=dev)
                up.copy_(pixels[:head + nbytes], non_blocking=True)
                packed = up[head:]
            else:
                up = torch.empty(head, dtype=torch.uint8, device=dev)
                up.copy_(pixels[:head], non_blocking=True)
                packed = torch.cat([img.reshape(-1) for img in images])
            if columns is not None:
                at = 0
                for p in parts:
                    meta[at:at + p.numel() * 8].copy_(p.view(torch.uint8))
                    at += p.numel() * 8
                meta_dev = torch.empty(nmeta, dtype=torch.uint8, device=dev)
                meta_dev.copy_(meta[:nmeta], non_blocking=True)
            stage.release()
            if dev not in self._luts:
                self._luts[dev] = normalised_bytes().to(dev)
            table_dev, taps_dev = up[:ntable], up[ntable:ntable + ntap_bytes]
            imgs = ops.yolo_ingest_u8(packed, table, table_dev, taps_dev, self._luts[dev], S)
            if columns is None:
                return imgs, None

            def column(dtype, count):
                nonlocal at
                v = meta_dev[at:at + count * 8].view(dtype)
                at += count * 8
                return v
            at = 0
            g, k = sum(counts), sum(int(c["category_id"].numel()) for c in columns)
            offsets_dev, boxes, area = column(torch.int64, n + 1), column(torch.float64, 4 * g).view(g, 4), column(torch.float64, g)
            labels, ids, sizes_dev = column(torch.int64, k), column(torch.int64, sum(s.numel() for s in id_shapes)), column(torch.int64, 3 * n).view(n, 3)
            bbox, rel_area = ops.yolo_targets(boxes, area, offsets_dev, table_dev, n)
            out = []
            for i, (b, a, l, d) in enumerate(zip(bbox.split(counts), rel_area.split(counts), labels.split([int(c["category_id"].numel()) for c in columns]),
                                                 ids.split([s.numel() for s in id_shapes]))):
                out.append({"bbox": b, "img_size": sizes_dev[i], "category_id": l, "area": a, "image_id": d.view(id_shapes[i])})
        return imgs, out


_COCO_80_91 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40,
               41, 42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 70, 72, 73, 74, 75, 76, 77, 78, 79,
               80, 81, 82, 84, 85, 86, 87, 88, 89, 90]


class COCO91_80():
    """COCO's 91 category ids to the 80 contiguous labels (transformations.py:57-82; the inverse of coco_80_91.json).  Plain host code."""

    def __init__(self):
        self.data_inv = {v: k for k, v in enumerate(_COCO_80_91)}

    def __call__(self, sample):
        img, targets = sample
        ids = targets['category_id']
        inv_l = [self.data_inv[label] for label in ids.tolist()]
        targets['category_id'] = torch.tensor(inv_l, dtype=torch.int64, device=ids.device if isinstance(ids, torch.Tensor) else None)
        return img, targets


class Class1_0():
    """Labels that start at 1 to labels that start at 0 (transformations.py:85-93)."""

    def __init__(self):
        pass

    def __call__(self, sample):
        img, targets = sample
        targets['category_id'] -= 1
        return img, targets


class Augment(object):
    """transformations.py:96-194 draws its augmentations from imgaug, which this package does not depend on: not built."""

    def __init__(self, num_of_augms=0):
        raise NotImplementedError("Augment needs imgaug, which is not part of this package: augment on the host with the reference's class, "
                                  "or pass flips to ResizeToTensor.batch")
