"""Mirror of torchvision_models/detection/coco_utils.py:33-108: COCO polygon annotations -> the `masks` a Mask R-CNN trains from, without
pycocotools.  The polygons are rasterised on the device (`polygons.polygons_to_rle`: frPyObjects + merge) and decoded there
(`ops.mask_rle_decode`), so `target["masks"]` is a uint8 [N, H, W] tensor ON THE DEVICE; the other fields are host tensors as in the
reference, whose training loop moves the whole target to the device anyway."""
import torch

from .. import ops
from ..polygons import polygons_to_rle


def convert_coco_poly_to_mask(segmentations, height, width, device=None):
    """coco_utils.py:33-47: one uint8 [H, W] mask per annotation (the union of its polygons), stacked; zeros((0, H, W)) for none."""
    segmentations = list(segmentations)
    if not segmentations:
        return torch.zeros((0, int(height), int(width)), dtype=torch.uint8, device="cuda" if device is None else device)
    return ops.mask_rle_decode(polygons_to_rle(segmentations, height, width, device))


def _image_size(image):
    """(w, h) of a PIL image (its .size) or of a [..., H, W] tensor."""
    if torch.is_tensor(image):
        return int(image.shape[-1]), int(image.shape[-2])
    return image.size


class ConvertCocoPolysToMask(object):
    """coco_utils.py:50-108: drops crowds, converts the boxes to clamped [x0, y0, x1, y1], rasterises the polygons, keeps the annotations
    whose box is not empty."""

    def __init__(self, device=None):
        self.device = device

    def __call__(self, image, target):
        w, h = _image_size(image)

        image_id = torch.tensor([target["image_id"]])

        anno = target["annotations"]
        try:
            anno = [obj for obj in anno if obj["iscrowd"] == 0]
        except KeyError:
            pass

        boxes = torch.as_tensor([obj["bbox"] for obj in anno], dtype=torch.float32).reshape(-1, 4)
        boxes[:, 2:] += boxes[:, :2]
        boxes[:, 0::2].clamp_(min=0, max=w)
        boxes[:, 1::2].clamp_(min=0, max=h)

        classes = torch.tensor([obj["category_id"] for obj in anno], dtype=torch.int64)

        masks = convert_coco_poly_to_mask([obj["segmentation"] for obj in anno], h, w, self.device)

        keypoints = None
        if anno and "keypoints" in anno[0]:
            keypoints = torch.as_tensor([obj["keypoints"] for obj in anno], dtype=torch.float32)
            num_keypoints = keypoints.shape[0]
            if num_keypoints:
                keypoints = keypoints.view(num_keypoints, -1, 3)

        keep = (boxes[:, 3] > boxes[:, 1]) & (boxes[:, 2] > boxes[:, 0])
        boxes = boxes[keep]
        classes = classes[keep]
        masks = masks[keep.to(masks.device)]
        if keypoints is not None:
            keypoints = keypoints[keep]

        out = {"boxes": boxes, "labels": classes, "masks": masks, "image_id": image_id}
        if keypoints is not None:
            out["keypoints"] = keypoints

        # for conversion to coco api
        out["area"] = torch.tensor([obj["area"] for obj in anno])
        try:
            out["iscrowd"] = torch.tensor([obj["iscrowd"] for obj in anno])
        except KeyError:
            out["iscrowd"] = torch.tensor([0 for obj in anno])
        return image, out
