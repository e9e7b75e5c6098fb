"""Mirror of `GeneralizedRCNNTransform` (torchvision_models/tvision/transform.py:65-257) and `resize_boxes` (:279-293): the input side of the
RetinaNet / Faster R-CNN step.

    transform = GeneralizedRCNNTransform(800, 1333, image_mean, image_std)
    image_list, targets = transform(images, targets)      # images: list of [3,H,W] float tensors on the GPU, any sizes
    image_list.tensors   [N,3,Hp,Wp] normalised, bilinear-resized (min side 800 / max side 1333), zero-padded to a multiple of 32
    image_list.image_sizes   [(h,w)] of every resized image
    detections = transform.postprocess(detections, image_list.image_sizes, original_image_sizes)   # boxes back to the input frame

Normalise + resize + pad run as ONE kernel per image (mi355det_resize_bilinear) that writes straight into the image's slot of the padded
batch; the size arithmetic (float32 scale, floor of the double product) is host logic that follows the reference line by line so the
output SIZES are identical.

    image_list, targets = transform.ingest(images, targets, flips)      # images: list of uint8 [H,W,3] as a decoder hands them over

is the second route: the horizontal flip of the training preset (tvision/presets.py), ToTensor's / 255, normalise, resize and pad of the
WHOLE batch in one launch (mi355det_ingest_u8), all boxes in one more (mi355det_flip_resize_boxes); the same bits as `forward` on the
flipped float images.  `plan_ingest` is its host-side size and layout planning.

    params, targets = transforms.SSDAugmentation("ssd").draw(shapes, targets)
    image_list, targets = transform.ingest(images, targets, augment=params)

adds the reference's `ssd` / `ssdlite` policies (tvision/transforms.py): photometric distortion on the packed bytes
(mi355det_photometric_u8), zoom-out, IoU crop and flip inside the image launch (mi355det_ingest_aug_u8)."""
import collections
import ctypes
import math

import numpy as np
import torch

from .._lib import (INGEST_TILE_H, INGEST_TILE_W, PHOTO_BLOCK_PIXELS, PHOTO_MAX_OPS, PHOTO_OPS, IngestAugImage, IngestImage, PhotoImage, check, lib,
                    ptr, stream_ptr)


class ImageList:
    """tvision/image_list.py:7-27.  `original_image_sizes` [(H, W)] is set by `GeneralizedRCNNTransform.ingest`: a model given such a list
    skips its transform and maps the detections back to these frames."""

    def __init__(self, tensors, image_sizes, original_image_sizes=None):
        self.tensors = tensors
        self.image_sizes = image_sizes
        self.original_image_sizes = original_image_sizes

    def to(self, device):
        return ImageList(self.tensors.to(device), self.image_sizes, self.original_image_sizes)


def ingested_sizes(image_list):
    """The original frames of an ImageList a model is called with in place of its images."""
    if image_list.original_image_sizes is None:
        raise ValueError("an ImageList given to a model must carry original_image_sizes (GeneralizedRCNNTransform.ingest sets them)")
    return [(int(h), int(w)) for h, w in image_list.original_image_sizes]


def resized_size(h, w, self_min_size, self_max_size):
    """Output size of `_resize_image_and_masks` (transform.py:26-52): scale = min(min_size / min(h,w), max_size / max(h,w)) in float32, then
    F.interpolate(scale_factor=scale.item(), recompute_scale_factor=True) -> floor(float(size) * scale) in double."""
    # `self_min_size / min_size` in the reference has a Python float on the left and a float32 tensor on the right = Tensor.__rtruediv__ =
    # reciprocal() * scalar: two float32 roundings (1/480 * 800 = 1.6666667, not 1.6666666), which decides 800 vs 799 rows
    mn, mx = np.float32(min(h, w)), np.float32(max(h, w))
    scale = float(min((np.float32(1) / mn) * np.float32(self_min_size), (np.float32(1) / mx) * np.float32(self_max_size)))
    return int(math.floor(float(h) * scale)), int(math.floor(float(w) * scale))


def mask_resize_nearest(masks, size):
    """The masks part of `_resize_image_and_masks` (transform.py:54-60): F.interpolate(masks[:, None].float(), scale_factor, nearest,
    recompute_scale_factor=True)[:, 0].byte() - the output size is the image's (same floor of the double product)."""
    from ..ops import mask_resize_nearest as _resize
    return _resize(masks, size)


def paste_masks(masks, boxes, img_shape, padding=1):
    """paste_masks_in_image (roi_heads.py:517-537), all detections of one image in one launch."""
    from ..ops import paste_masks as _paste
    return _paste(masks, boxes, img_shape, padding)


def resize_boxes(boxes, original_size, new_size):
    """transform.py:279-293."""
    if boxes.numel() == 0:
        return boxes.clone()
    b = boxes.float().contiguous()
    out = torch.empty_like(b)
    check(lib().mi355det_resize_boxes(ptr(b), ptr(out), b.shape[0], int(original_size[0]), int(original_size[1]), int(new_size[0]), int(new_size[1]),
                                      stream_ptr()), "resize_boxes")
    return out


def padded_size(sizes, size_divisible):
    """batch_images (transform.py:215-226): the largest resized image, each side rounded up to a multiple of `size_divisible`."""
    stride = float(size_divisible)
    return (int(math.ceil(float(max(s[0] for s in sizes)) / stride) * stride),
            int(math.ceil(float(max(s[1] for s in sizes)) / stride) * stride))


IngestPlan = collections.namedtuple("IngestPlan", "sizes pad offsets nbytes first_tile tiles")


def plan_ingest(shapes, min_size, max_size, size_divisible=32, fixed_size=None):
    """Sizes and layout of one `ingest` call, on the host alone.  shapes: [(H, W)] of the uint8 images; min_size: the min side for all
    images, or one per image (the training draws).
        sizes       [(h, w)] of every resized image (`resized_size`, or `fixed_size`)
        pad         (pad_h, pad_w) of the batch
        offsets     byte offset of every image in the packed buffer (running sums of 3 * H * W), nbytes their total
        first_tile  index of every image's first tile of the mi355det_ingest_u8 launch, tiles their total"""
    n = len(shapes)
    mins = list(min_size) if isinstance(min_size, (list, tuple)) else [min_size] * n
    if len(mins) != n:
        raise ValueError(f"plan_ingest: {len(mins)} min sizes for {n} images")
    if fixed_size is not None:
        sizes = [(int(fixed_size[1]), int(fixed_size[0]))] * n
    else:
        sizes = [resized_size(int(h), int(w), float(mn), float(max_size)) for (h, w), mn in zip(shapes, mins)]
    ph, pw = padded_size(sizes, size_divisible)
    per_image = -(-ph // INGEST_TILE_H) * -(-pw // INGEST_TILE_W)
    offsets, total = _packed_layout(shapes)
    return IngestPlan(sizes, (ph, pw), offsets, total, [i * per_image for i in range(n)], n * per_image)


def _packed_layout(shapes):
    """Byte offset of every [H, W, 3] image in the packed buffer, and their total."""
    offsets, total = [], 0
    for h, w in shapes:
        offsets.append(total)
        total += 3 * int(h) * int(w)
    return offsets, total


def resize_keypoints(keypoints, original_size, new_size):
    """transform.py:260-275: x and y scaled by the float32 ratios new / original, v untouched (a float32 multiply per coordinate)."""
    ratio_h, ratio_w = (np.float32(s) / np.float32(o) for s, o in zip(new_size, original_size))
    out = keypoints.clone()
    out[..., 0] *= float(ratio_w)
    out[..., 1] *= float(ratio_h)
    return out


def _checked_ingest_arguments(images, targets, flips, keypoints=False):
    """The refusals of `ingest`, all on the host and ahead of any launch.  Returns the images as tensors, the targets as copied dicts (the
    caller's dicts and tensors are not modified) and one bool per image."""
    images = [torch.as_tensor(i) for i in images]
    n = len(images)
    if n == 0:
        raise ValueError("ingest: images is empty")
    for img in images:
        if img.dtype != torch.uint8:
            raise TypeError(f"ingest: expected uint8 images of shape [H, W, 3], but found type {img.dtype}")
        if img.dim() != 3 or img.shape[-1] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
            raise ValueError("ingest: images is expected to be a list of uint8 tensors of shape [H, W, 3], got {}".format(tuple(img.shape)))
    if any(img.device != images[0].device for img in images):
        raise ValueError("ingest: the images are either all on the CPU or all on one device")
    flips = [False] * n if flips is None else [bool(f) for f in flips]
    if len(flips) != n:
        raise ValueError(f"ingest: {len(flips)} flips for {n} images")
    if targets is not None:
        if len(targets) != n:
            raise ValueError(f"ingest: {len(targets)} targets for {n} images")
        targets = [dict(t) for t in targets]
        for t, img in zip(targets, images):
            if "keypoints" in t and not keypoints:
                raise ValueError("ingest: targets with keypoints are not supported (there is no keypoint branch on this path)")
            if "keypoints" in t:
                kp = t["keypoints"]
                if kp.dim() != 3 or kp.shape[-1] != 3 or not kp.is_floating_point():
                    raise ValueError("ingest: expected target keypoints to be a float tensor of shape [G, K, 3], got {}".format(tuple(kp.shape)))
            if "boxes" in t and (t["boxes"].dim() != 2 or t["boxes"].shape[-1] != 4):
                raise ValueError("Expected target boxes to be a tensor of shape [N, 4], got {:}.".format(tuple(t["boxes"].shape)))
            if "masks" in t and (t["masks"].dim() != 3 or tuple(t["masks"].shape[-2:]) != tuple(img.shape[:2])):
                raise ValueError("ingest: masks of shape {} for an image of {}".format(tuple(t["masks"].shape), tuple(img.shape[:2])))
    return images, targets, flips


def _augment_tables(augment, shapes, targets):
    """The refusals and the tables of `ingest(augment=...)`, on the host and ahead of any launch.  augment: one record per image with the
    fields of `transforms.AugmentParams`.  Returns the windows [(h, w)] (the images the resize sees), the mi355det_ingest_aug_image table
    without its offset, out_h / out_w and first_tile columns, and the mi355det_photo_image table of the images that have ops (offsets and
    blocks from the packed layout of `shapes`)."""
    n = len(shapes)
    augment = list(augment)
    if len(augment) != n:
        raise ValueError(f"ingest: {len(augment)} augment records for {n} images")
    if targets is not None and any("masks" in t for t in targets):
        raise ValueError("ingest: targets with masks are not supported together with augment (the reference's IoU crop does not touch them)")
    windows, table, photo, offset, block = [], (IngestAugImage * n)(), [], 0, 0
    for i, (p, (h, w)) in enumerate(zip(augment, shapes)):
        canvas_h, canvas_w, left, top, fill = p.zoom if p.zoom is not None else (h, w, 0, 0, (0, 0, 0))
        if left < 0 or top < 0 or top + h > canvas_h or left + w > canvas_w:
            raise ValueError(f"ingest: image {i}: the zoom-out canvas {canvas_h} x {canvas_w} does not hold the {h} x {w} image at ({top}, {left})")
        if len(fill) != 3 or any(int(f) != f or not 0 <= f <= 255 for f in fill):
            raise ValueError(f"ingest: image {i}: the fill is three bytes, got {fill}")
        crop_left, crop_top, crop_w, crop_h = p.crop if p.crop is not None else (0, 0, canvas_w, canvas_h)
        if crop_w < 1 or crop_h < 1 or crop_left < 0 or crop_top < 0 or crop_top + crop_h > canvas_h or crop_left + crop_w > canvas_w:
            raise ValueError(f"ingest: image {i}: the crop {p.crop} is empty or lies outside its {canvas_h} x {canvas_w} canvas")
        windows.append((int(crop_h), int(crop_w)))
        table[i] = IngestAugImage(0, h, w, canvas_h, canvas_w, top, left, crop_top, crop_left, crop_h, crop_w, 0, 0, int(bool(p.flip)), 0,
                                  int(fill[0]) | int(fill[1]) << 8 | int(fill[2]) << 16, 0)
        ops, perm = tuple(p.ops), (0, 1, 2) if p.permutation is None else tuple(int(c) for c in p.permutation)
        if sorted(perm) != [0, 1, 2]:
            raise ValueError(f"ingest: image {i}: {p.permutation} is no permutation of the three channels")
        if len(ops) > PHOTO_MAX_OPS or sum(name == "contrast" for name, _f in ops) > 1:
            raise ValueError(f"ingest: image {i}: at most {PHOTO_MAX_OPS} photometric ops, one contrast among them")
        if ops or perm != (0, 1, 2):
            codes, factors = [], []
            for name, f in ops:
                if name not in PHOTO_OPS:
                    raise ValueError(f'ingest: image {i}: unknown photometric op "{name}"')
                if name == "hue":
                    if not -0.5 <= f <= 0.5:
                        raise ValueError(f"ingest: image {i}: hue factor {f} is not in [-0.5, 0.5]")
                    f = int(float(f) * 255) & 255        # adjust_hue's np.uint8(hue_factor * 255), which H is shifted by modulo 256
                elif not 0 <= f < math.inf:
                    raise ValueError(f"ingest: image {i}: {name} factor {f} is negative or not finite")
                codes.append(PHOTO_OPS[name])
                factors.append(float(f))
            pad = PHOTO_MAX_OPS - len(ops)
            photo.append(PhotoImage(offset, h * w, block, len(ops), (ctypes.c_int32 * PHOTO_MAX_OPS)(*codes, *[0] * pad),
                                    (ctypes.c_float * PHOTO_MAX_OPS)(*factors, *[0.0] * pad), (ctypes.c_int32 * 3)(*perm), 0))
            block += -(-h * w // PHOTO_BLOCK_PIXELS)
        offset += 3 * h * w
    if targets is not None:
        for i, (t, (wh, ww)) in enumerate(zip(targets, windows)):
            if "boxes" in t and t["boxes"].numel() and (float(t["boxes"][:, 0::2].max()) > ww or float(t["boxes"][:, 1::2].max()) > wh):
                raise ValueError(f"ingest: image {i}: boxes outside the {wh} x {ww} window: with augment, the targets are those `draw` returned")
    return windows, table, (PhotoImage * len(photo))(*photo)


class _Staging:
    """Pinned host buffers of `ingest` for one device: the packed pixels, and the image table followed by the box offsets.  An upload from
    them is asynchronous, so `acquire` waits for the event recorded behind the previous call's copies before the buffers are written again."""

    def __init__(self):
        self.pixels = self.meta = self.event = None

    def acquire(self, nbytes, nmeta):
        if self.event is not None:
            self.event.synchronize()
        if self.pixels is None or self.pixels.numel() < nbytes:
            self.pixels = torch.empty(max(nbytes, 1), dtype=torch.uint8, pin_memory=True)
        if self.meta is None or self.meta.numel() < nmeta:
            self.meta = torch.empty(nmeta, dtype=torch.uint8, pin_memory=True)
        return self.pixels, self.meta

    def release(self):
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()


class GeneralizedRCNNTransform(torch.nn.Module):
    def __init__(self, min_size, max_size, image_mean, image_std, size_divisible=32, fixed_size=None, keypoints=False):
        super().__init__()
        self.keypoints = keypoints          # True for a model with a keypoint branch (KeypointRCNN): `ingest` then takes targets with keypoints
        self.min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
        self.max_size = max_size
        self.image_mean, self.image_std = image_mean, image_std
        self.size_divisible = size_divisible
        self.fixed_size = fixed_size
        self._stats = {}
        self._staging = {}

    def torch_choice(self, k):
        """transform.py:137-145 (same RNG draw as the reference)."""
        return k[int(torch.empty(1).uniform_(0.0, float(len(k))).item())]

    def _mean_std(self, device):
        if device not in self._stats:
            self._stats[device] = (torch.tensor(self.image_mean, dtype=torch.float32, device=device),
                                   torch.tensor(self.image_std, dtype=torch.float32, device=device))
        return self._stats[device]

    def forward(self, images, targets=None):
        images = list(images)
        if targets is not None:
            targets = [dict(t) for t in targets]          # copy, as the reference does, so the caller's dicts are not modified
        sizes = []
        for img in images:
            if img.dim() != 3:
                raise ValueError("images is expected to be a list of 3d tensors of shape [C, H, W], got {}".format(img.shape))
            if not img.is_floating_point():
                raise TypeError(f"Expected input images to be of floating type (in range [0, 1]), but found type {img.dtype} instead")
            h, w = int(img.shape[-2]), int(img.shape[-1])
            if self.fixed_size is not None:
                sizes.append((int(self.fixed_size[1]), int(self.fixed_size[0])))
            else:
                size = float(self.torch_choice(self.min_size)) if self.training else float(self.min_size[-1])
                sizes.append(resized_size(h, w, size, float(self.max_size)))
        ph, pw = padded_size(sizes, self.size_divisible)
        dev = images[0].device
        c = int(images[0].shape[0])
        mean, std = self._mean_std(dev)
        batch = torch.empty((len(images), c, ph, pw), dtype=torch.float32, device=dev)
        L = lib()
        for i, (img, (oh, ow)) in enumerate(zip(images, sizes)):
            src = img.float().contiguous()
            check(L.mi355det_resize_bilinear(ptr(src), c, c, int(img.shape[-2]), int(img.shape[-1]), ptr(mean), ptr(std), ptr(batch[i]), oh, ow, ph, pw,
                                             stream_ptr()), "resize_bilinear")
            if targets is not None and targets[i] is not None and "boxes" in targets[i]:
                targets[i]["boxes"] = resize_boxes(targets[i]["boxes"], (int(img.shape[-2]), int(img.shape[-1])), (oh, ow))
            if targets is not None and targets[i] is not None and "masks" in targets[i]:      # transform.py:54-60 (nearest, uint8)
                targets[i]["masks"] = mask_resize_nearest(targets[i]["masks"], (oh, ow))
            if targets is not None and targets[i] is not None and "keypoints" in targets[i]:  # transform.py:169-172
                targets[i]["keypoints"] = resize_keypoints(targets[i]["keypoints"], (int(img.shape[-2]), int(img.shape[-1])), (oh, ow))
        return ImageList(batch, sizes), targets

    def ingest(self, images, targets=None, flips=None, device=None, augment=None):
        """The route for images as a decoder hands them over: a list of uint8 [H, W, 3] tensors (or numpy arrays) of any sizes, all on the
        CPU or all on one device, and one horizontal-flip flag per image (detection/transforms.py:30-44; `presets.DetectionPresetTrain.draw`).
        Returns what `forward` returns for the flipped float images `img.permute(2, 0, 1).float().div(255)` and their flipped targets, bit
        for bit, from one image launch (mi355det_ingest_u8) and one box launch (mi355det_flip_resize_boxes) per batch; the ImageList
        carries `original_image_sizes`.  CPU images are packed into a pinned buffer and go up in one copy (to `device`, default the current
        one).  Targets are copied: `boxes` and `masks` are transformed, other keys pass through.  `keypoints` (float [G, K, 3]) are refused
        by a transform built without `keypoints=True` (a model without a keypoint branch); KeypointRCNN's transform flips them
        (detection/transforms.py:10-19: the COCO person index permutation, x = width - x, rows with v == 0 zeroed) and resizes them
        (transform.py:260-275), all keypoints of the batch in one launch beside the box launch (mi355det_flip_resize_keypoints).

        augment: the records of `transforms.SSDAugmentation.draw`, one per image, with the targets that `draw` returned and `flips` None
        (the flip is in the records).  The photometric ops run on the packed bytes (mi355det_photometric_u8), zoom-out, crop and flip
        inside the image launch (mi355det_ingest_aug_u8), the boxes as before with the window's width: the same bits as `forward` on the
        images that the reference's PIL transforms give.  Sizes and `original_image_sizes` are the windows': the images the model sees."""
        if augment is not None and flips is not None:
            raise ValueError("ingest: with augment the flips are in its records, flips must be None")
        images, targets, flips = _checked_ingest_arguments(images, targets, flips, self.keypoints)
        if augment is not None and targets is not None and any("keypoints" in t for t in targets):
            raise ValueError("ingest: targets with keypoints are not supported together with augment (the ssd / ssdlite policies do not move them)")
        n = len(images)
        src_dev = images[0].device
        shapes = [(int(img.shape[0]), int(img.shape[1])) for img in images]
        windows, aug_table, photo_table = shapes, None, None
        if augment is not None:
            windows, aug_table, photo_table = _augment_tables(augment, shapes, targets)
            flips = [bool(p.flip) for p in augment]
        if self.fixed_size is None and self.training:
            mins = [float(self.torch_choice(self.min_size)) for _ in images]       # one draw per image, in order, as `forward`
        else:
            mins = float(self.min_size[-1])
        plan = plan_ingest(windows, mins, float(self.max_size), self.size_divisible, self.fixed_size)
        offsets, nbytes = (plan.offsets, plan.nbytes) if augment is None else _packed_layout(shapes)      # the sources', not the windows'
        if src_dev.type != "cpu":
            dev = src_dev
        else:
            dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())

        table = (IngestImage * n)()              # of the windows: the whole images without augment
        for i, ((h, w), (oh, ow)) in enumerate(zip(windows, plan.sizes)):
            table[i] = IngestImage(offsets[i], h, w, oh, ow, int(flips[i]), plan.first_tile[i])
            if augment is not None:
                aug_table[i].offset, aug_table[i].out_h, aug_table[i].out_w, aug_table[i].first_tile = offsets[i], oh, ow, plan.first_tile[i]
        with_boxes = [i for i in range(n) if targets is not None and "boxes" in targets[i]]
        box_offsets = np.zeros(n + 1, dtype=np.int64)
        for i in with_boxes:
            box_offsets[i + 1] = targets[i]["boxes"].shape[0]
        np.cumsum(box_offsets, out=box_offsets)
        with_kp = [i for i in range(n) if targets is not None and "keypoints" in targets[i]]
        kp_offsets = np.zeros(n + 1, dtype=np.int64)
        for i in with_kp:
            kp_offsets[i + 1] = targets[i]["keypoints"].shape[0]
            if flips[i] and targets[i]["keypoints"].shape[1] != 17:
                raise ValueError("ingest: the flip of keypoints is the COCO person permutation of 17 keypoints (detection/transforms.py:10-19), "
                                 "got {}".format(int(targets[i]["keypoints"].shape[1])))
            if targets[i]["keypoints"].shape[1] != targets[with_kp[0]]["keypoints"].shape[1]:
                raise ValueError("ingest: every image must have the same number of keypoints per instance")
        np.cumsum(kp_offsets, out=kp_offsets)
        ntable = ctypes.sizeof(table)
        nbox = ntable + box_offsets.nbytes
        naug = nmeta = nbox + (kp_offsets.nbytes if with_kp else 0)      # the augment tables follow: every size is a multiple of 8
        if augment is not None:
            nphoto = naug + ctypes.sizeof(aug_table)
            nmeta = nphoto + ctypes.sizeof(photo_table)
        with torch.cuda.device(dev):
            stage = self._staging.setdefault(dev, _Staging())
            pixels, meta = stage.acquire(nbytes if src_dev.type == "cpu" else 0, nmeta)
            meta[:ntable].copy_(torch.from_numpy(np.frombuffer(table, dtype=np.uint8)))
            meta[ntable:nbox].copy_(torch.from_numpy(box_offsets.view(np.uint8)))
            if with_kp:
                meta[nbox:naug].copy_(torch.from_numpy(kp_offsets.view(np.uint8)))
            if augment is not None:
                meta[naug:nphoto].copy_(torch.from_numpy(np.frombuffer(aug_table, dtype=np.uint8)))
                if len(photo_table):
                    meta[nphoto:nmeta].copy_(torch.from_numpy(np.frombuffer(photo_table, dtype=np.uint8)))
            if src_dev.type == "cpu":
                for img, off, (h, w) in zip(images, offsets, shapes):
                    pixels[off:off + 3 * h * w].view(h, w, 3).copy_(img)
                packed = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                packed.copy_(pixels[:nbytes], non_blocking=True)
            else:
                packed = torch.cat([img.reshape(-1) for img in images])
            meta_dev = torch.empty(nmeta, dtype=torch.uint8, device=dev)
            meta_dev.copy_(meta[:nmeta], non_blocking=True)
            stage.release()
            table_dev = ctypes.c_void_p(meta_dev.data_ptr())
            mean, std = self._mean_std(dev)
            ph, pw = plan.pad
            batch = torch.empty((n, 3, ph, pw), dtype=torch.float32, device=dev)
            L = lib()
            if augment is None:
                check(L.mi355det_ingest_u8(ptr(packed), nbytes, ctypes.cast(table, ctypes.c_void_p), table_dev, n, ptr(mean), ptr(std), ptr(batch),
                                           ph, pw, stream_ptr()), "ingest_u8")
            else:
                if len(photo_table):
                    sums = torch.empty(len(photo_table), dtype=torch.int64, device=dev)
                    check(L.mi355det_photometric_u8(ptr(packed), nbytes, ctypes.cast(photo_table, ctypes.c_void_p),
                                                    ctypes.c_void_p(meta_dev.data_ptr() + nphoto), len(photo_table), ptr(sums),
                                                    stream_ptr()), "photometric_u8")
                check(L.mi355det_ingest_aug_u8(ptr(packed), nbytes, ctypes.cast(aug_table, ctypes.c_void_p),
                                               ctypes.c_void_p(meta_dev.data_ptr() + naug), n, ptr(mean), ptr(std), ptr(batch), ph, pw,
                                               stream_ptr()), "ingest_aug_u8")
            if with_boxes:
                boxes = [targets[i]["boxes"].to(torch.float32) for i in with_boxes]
                if any(b.device != boxes[0].device for b in boxes):
                    boxes = [b.to(dev) for b in boxes]
                boxes = torch.cat(boxes).to(dev).contiguous()
                out = torch.empty_like(boxes)
                check(L.mi355det_flip_resize_boxes(ptr(boxes), ptr(out), boxes.shape[0], ctypes.c_void_p(meta_dev.data_ptr() + ntable), table_dev, n,
                                                   stream_ptr()), "flip_resize_boxes")
                for i, b in zip(with_boxes, out.split([int(targets[i]["boxes"].shape[0]) for i in with_boxes])):
                    targets[i]["boxes"] = b
            if with_kp:
                kps = [targets[i]["keypoints"].to(torch.float32).to(dev) for i in with_kp]
                kps = torch.cat(kps).contiguous()
                out = torch.empty_like(kps)
                check(L.mi355det_flip_resize_keypoints(ptr(kps), ptr(out), kps.shape[0], kps.shape[1], ctypes.c_void_p(meta_dev.data_ptr() + nbox),
                                                       ctypes.cast(table, ctypes.c_void_p), table_dev, n, stream_ptr()), "flip_resize_keypoints")
                for i, k in zip(with_kp, out.split([int(targets[i]["keypoints"].shape[0]) for i in with_kp])):
                    targets[i]["keypoints"] = k
            if targets is not None:
                from ..ops import mask_resize_nearest as _resize
                for i, t in enumerate(targets):
                    if "masks" in t:
                        t["masks"] = _resize(t["masks"].to(dev), plan.sizes[i], flip=flips[i])
        return ImageList(batch, plan.sizes, windows), targets

    def postprocess(self, result, image_shapes, original_image_sizes, mask_format="dense"):
        """transform.py:228-247 (boxes, masks and keypoints when the result has them).  mask_format "dense" is the
        reference's [D, 1, H0, W0] float masks; "rle" gives their `> 0.5` run lengths (an RLEBatch) at the original image size instead."""
        if mask_format not in ("dense", "rle"):
            raise ValueError("mask_format must be 'dense' or 'rle'")
        if self.training:
            return result
        for i, (pred, im_s, o_im_s) in enumerate(zip(result, image_shapes, original_image_sizes)):
            boxes = resize_boxes(pred["boxes"], im_s, o_im_s)
            result[i]["boxes"] = boxes
            if "masks" in pred:
                if mask_format == "dense":
                    result[i]["masks"] = paste_masks(pred["masks"], boxes, o_im_s)
                else:              # `paste_masks(...) > 0.5` as run lengths, without the full-size masks
                    from ..ops import mask_rle_paste
                    result[i]["masks"] = mask_rle_paste(pred["masks"], boxes, o_im_s)
            if "keypoints" in pred:
                result[i]["keypoints"] = resize_keypoints(pred["keypoints"], im_s, o_im_s)
        return result


def interpolate_bilinear(imgs, size):
    """F.interpolate(imgs, size=size, mode='bilinear', align_corners=False) of a batch [N,C,H,W] (YOLO multi-scale training,
    yolo/procedures/train_one_epoch.py:64-69)."""
    n, c, h, w = imgs.shape
    oh, ow = (size, size) if isinstance(size, int) else (int(size[0]), int(size[1]))
    src = imgs.float().contiguous()
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=imgs.device)
    check(lib().mi355det_resize_bilinear(ptr(src), n * c, c, h, w, None, None, ptr(out), oh, ow, oh, ow, stream_ptr()), "resize_bilinear")
    return out
