"""Mirror of the reference's detection transforms (torchvision_models/detection/transforms.py:30-239) for the uint8 route of
`GeneralizedRCNNTransform.ingest`: the `ssd` and `ssdlite` policies of detection/presets.py:12-25.

    aug = SSDAugmentation("ssd", hflip_prob=0.5)
    params, targets = aug.draw(shapes, targets)                     # shapes: [(H, W)] of the uint8 images
    image_list, targets = model.transform.ingest(images, targets, augment=params)

As in tvision/presets.py a transform here only DECIDES.  `draw` consumes torch's global CPU generator exactly as the reference's per-sample
`Compose` does (image after image, and all of one image's transforms before the next image's), so the same seed distorts, zooms, crops and
flips the same images in the same way; it returns one `AugmentParams` per image.  The pixels are touched on the device alone:
RandomPhotometricDistort by mi355det_photometric_u8, RandomZoomOut, RandomIoUCrop and RandomHorizontalFlip inside the ingest kernel
(mi355det_ingest_aug_u8), which reads the crop window of the zoom-out canvas without the canvas ever being stored.

What the reference does to the boxes before the flip (the zoom-out's shift, transforms.py:183-185; the crop's filter, shift and clamp,
:120-126) happens here, on copies and with the same float32 torch CPU operations; the flip of the boxes is left to
mi355det_flip_resize_boxes.  Masks and keypoints are refused: the reference's crop does not touch them.

`T.ColorJitter` is restated from torchvision: per executed call it draws `torch.randperm(4)` and then one
`torch.empty(1).uniform_(lo, hi)` for its single range."""
import dataclasses
from typing import Optional, Tuple

import torch


@dataclasses.dataclass
class AugmentParams:
    """What one image's transforms decided.
        ops          the photometric ops in order, (name, factor) with name in "brightness", "contrast", "saturation", "hue": at most
                     brightness, contrast, saturation, hue, contrast, and at most one contrast
        permutation  the channel permutation (output channel c is input channel permutation[c]) or None
        zoom         (canvas_h, canvas_w, left, top, fill bytes) of the zoom-out or None
        crop         (left, top, new_w, new_h) of the IoU crop, in canvas coordinates, or None
        flip         the horizontal flip of what is left"""
    ops: Tuple[Tuple[str, float], ...] = ()
    permutation: Optional[Tuple[int, int, int]] = None
    zoom: Optional[Tuple[int, int, int, int, Tuple[int, int, int]]] = None
    crop: Optional[Tuple[int, int, int, int]] = None
    flip: bool = False

    def window(self, h, w):
        """(new_h, new_w) of an [h, w] image after zoom-out and crop: the image the model sees."""
        if self.crop is not None:
            return int(self.crop[3]), int(self.crop[2])
        if self.zoom is not None:
            return int(self.zoom[0]), int(self.zoom[1])
        return int(h), int(w)


def box_iou(boxes1, boxes2):
    """torchvision.ops.boxes.box_iou in torch CPU ops: intersection / (a1 + a2 - inter)."""
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def _jitter(lo, hi):
    """One executed T.ColorJitter with a single range: the order of its four ops, then the factor."""
    torch.randperm(4)
    return float(torch.empty(1).uniform_(lo, hi))


class RandomPhotometricDistort:
    """transforms.py:190-239."""

    def __init__(self, contrast=(0.5, 1.5), saturation=(0.5, 1.5), hue=(-0.05, 0.05), brightness=(0.875, 1.125), p=0.5):
        self.contrast, self.saturation, self.hue, self.brightness, self.p = contrast, saturation, hue, brightness, p

    def draw(self):
        """(ops, permutation) of one image."""
        r = torch.rand(7)
        ops = []
        if r[0] < self.p:
            ops.append(("brightness", _jitter(*self.brightness)))
        contrast_before = r[1] < 0.5
        if contrast_before:
            if r[2] < self.p:
                ops.append(("contrast", _jitter(*self.contrast)))
        if r[3] < self.p:
            ops.append(("saturation", _jitter(*self.saturation)))
        if r[4] < self.p:
            ops.append(("hue", _jitter(*self.hue)))
        if not contrast_before:
            if r[5] < self.p:
                ops.append(("contrast", _jitter(*self.contrast)))
        permutation = None
        if r[6] < self.p:
            permutation = tuple(int(c) for c in torch.randperm(3))
        return tuple(ops), permutation


class RandomZoomOut:
    """transforms.py:132-187."""

    def __init__(self, fill=None, side_range=(1., 4.), p=0.5):
        self.fill = [0., 0., 0.] if fill is None else fill
        self.side_range = side_range
        if side_range[0] < 1. or side_range[0] > side_range[1]:
            raise ValueError("Invalid canvas side range provided {}.".format(side_range))
        self.p = p

    def draw(self, h, w, boxes):
        """The canvas of an [h, w] image, or None; `boxes` are shifted in place."""
        if torch.rand(1) < self.p:
            return None
        r = self.side_range[0] + torch.rand(1) * (self.side_range[1] - self.side_range[0])
        canvas_w = int(w * r)
        canvas_h = int(h * r)
        r = torch.rand(2)
        left = int((canvas_w - w) * r[0])
        top = int((canvas_h - h) * r[1])
        boxes[:, 0::2] += left
        boxes[:, 1::2] += top
        return canvas_h, canvas_w, left, top, tuple(int(x) for x in self.fill)


class RandomIoUCrop:
    """transforms.py:54-129."""

    def __init__(self, min_scale=0.3, max_scale=1.0, min_aspect_ratio=0.5, max_aspect_ratio=2.0, sampler_options=None, trials=40):
        self.min_scale, self.max_scale = min_scale, max_scale
        self.min_aspect_ratio, self.max_aspect_ratio = min_aspect_ratio, max_aspect_ratio
        self.options = [0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0] if sampler_options is None else sampler_options
        self.trials = trials

    def draw(self, orig_h, orig_w, boxes):
        """(crop, keep) of an [orig_h, orig_w] image: the window and the mask of the boxes whose centres lie in it, or (None, None)."""
        while True:
            idx = int(torch.randint(low=0, high=len(self.options), size=(1,)))
            min_jaccard_overlap = self.options[idx]
            if min_jaccard_overlap >= 1.0:
                return None, None
            for _ in range(self.trials):
                r = self.min_scale + (self.max_scale - self.min_scale) * torch.rand(2)
                new_w = int(orig_w * r[0])
                new_h = int(orig_h * r[1])
                aspect_ratio = new_w / new_h
                if not (self.min_aspect_ratio <= aspect_ratio <= self.max_aspect_ratio):
                    continue
                r = torch.rand(2)
                left = int((orig_w - new_w) * r[0])
                top = int((orig_h - new_h) * r[1])
                right = left + new_w
                bottom = top + new_h
                if left == right or top == bottom:
                    continue
                cx = 0.5 * (boxes[:, 0] + boxes[:, 2])
                cy = 0.5 * (boxes[:, 1] + boxes[:, 3])
                is_within_crop_area = (left < cx) & (cx < right) & (top < cy) & (cy < bottom)
                if not is_within_crop_area.any():
                    continue
                ious = box_iou(boxes[is_within_crop_area], torch.tensor([[left, top, right, bottom]], dtype=boxes.dtype))
                if ious.max() < min_jaccard_overlap:
                    continue
                return (left, top, new_w, new_h), is_within_crop_area


class RandomHorizontalFlip:
    """transforms.py:30-44."""

    def __init__(self, p=0.5):
        self.p = p

    def draw(self):
        return bool(torch.rand(1) < self.p)


def _checked_targets(shapes, targets):
    if targets is None:
        raise ValueError("The targets can't be None for this transform.")
    if len(targets) != len(shapes):
        raise ValueError(f"draw: {len(targets)} targets for {len(shapes)} images")
    for t in targets:
        for key in ("masks", "keypoints"):
            if key in t:
                raise ValueError(f"draw: targets with {key} are not supported (the reference's IoU crop does not touch them)")
        if "boxes" not in t or t["boxes"].dim() != 2 or t["boxes"].shape[-1] != 4:
            got = tuple(t["boxes"].shape) if "boxes" in t else None
            raise ValueError("Expected target boxes to be a tensor of shape [N, 4], got {:}.".format(got))


class SSDAugmentation:
    """DetectionPresetTrain("ssd" | "ssdlite") of detection/presets.py:12-25 without its ToTensor, which the ingest kernel does."""

    def __init__(self, policy="ssd", hflip_prob=0.5, mean=(123., 117., 104.)):
        if policy not in ("ssd", "ssdlite"):
            raise ValueError(f'Unknown SSD data augmentation policy "{policy}"')
        self.policy = policy
        self.distort = RandomPhotometricDistort() if policy == "ssd" else None
        self.zoom_out = RandomZoomOut(fill=list(mean)) if policy == "ssd" else None
        self.iou_crop = RandomIoUCrop()
        self.hflip = RandomHorizontalFlip(p=hflip_prob)

    def draw(self, shapes, targets):
        """shapes: [(H, W)] of the images; targets: one dict per image with `boxes` [G, 4] (and `labels` [G]).  Returns ([AugmentParams],
        targets): copies whose boxes are float32 CPU tensors in the cropped window's frame, not yet flipped."""
        _checked_targets(shapes, targets)
        params, out = [], []
        for (h, w), target in zip(shapes, targets):
            h, w = int(h), int(w)
            target = dict(target)
            boxes = target["boxes"].detach().to("cpu", torch.float32, copy=True)
            p = AugmentParams()
            if self.distort is not None:
                p.ops, p.permutation = self.distort.draw()
            if self.zoom_out is not None:
                p.zoom = self.zoom_out.draw(h, w, boxes)
            canvas_h, canvas_w = p.window(h, w)
            p.crop, keep = self.iou_crop.draw(canvas_h, canvas_w, boxes)
            if p.crop is not None:
                left, top, new_w, new_h = p.crop
                boxes = boxes[keep]
                if "labels" in target:
                    target["labels"] = target["labels"][keep.to(target["labels"].device)]
                boxes[:, 0::2] -= left
                boxes[:, 1::2] -= top
                boxes[:, 0::2].clamp_(min=0, max=new_w)
                boxes[:, 1::2].clamp_(min=0, max=new_h)
            p.flip = self.hflip.draw()
            target["boxes"] = boxes
            params.append(p)
            out.append(target)
        return params, out
