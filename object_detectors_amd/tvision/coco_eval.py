"""Mirror of the detection-to-COCO formatting of torchvision_models/detection/coco_eval.py (:83-105 prepare_for_coco_detection,
:107-140 prepare_for_coco_segmentation, :169-171 convert_to_xywh): the wire format handed to pycocotools / lvis."""
import torch

from .._lib import check, lib, ptr, stream_ptr


def convert_to_xywh(boxes):
    """coco_eval.py:169-171."""
    k = int(boxes.shape[0])
    b = boxes.float().contiguous()
    out = torch.empty((k, 4), dtype=torch.float32, device=b.device)
    check(lib().mi355det_coco_rows(ptr(b), 4, None, None, 0, k, 1.0, 1.0, 1.0, 0, 2, ptr(out), None, None, stream_ptr()), "coco_rows")
    return out


def prepare_for_coco_detection(predictions):
    """coco_eval.py:83-105: {image_id: {'boxes' [k,4] xyxy, 'scores' [k], 'labels' [k]}} -> list of result dicts."""
    coco_results = []
    for original_id, prediction in predictions.items():
        if len(prediction) == 0:
            continue
        boxes = convert_to_xywh(prediction["boxes"]).tolist()
        scores = prediction["scores"].tolist()
        labels = prediction["labels"].tolist()
        coco_results.extend([{"image_id": original_id, "category_id": labels[k], "bbox": box, "score": scores[k]} for k, box in enumerate(boxes)])
    return coco_results


def prepare_for_coco_segmentation(predictions):
    """coco_eval.py:107-140: {image_id: {'scores' [k], 'labels' [k], 'masks'}} -> list of result dicts whose 'segmentation' is the compressed
    run-length encoding pycocotools' mask.encode would give for `masks > 0.5`.  'masks' is the reference's dense [k, 1, H, W] float tensor
    (encoded by mi355det_mask_rle_count / _emit) or the RLEBatch of MaskRCNN(mask_format="rle")."""
    from ..ops import mask_rle_dense
    from ..rle import RLEBatch
    coco_results = []
    for original_id, prediction in predictions.items():
        if len(prediction) == 0:
            continue
        scores = prediction["scores"].tolist()
        labels = prediction["labels"].tolist()
        masks = prediction["masks"]
        rles = (masks if isinstance(masks, RLEBatch) else mask_rle_dense(masks, 0.5)).to_coco()
        coco_results.extend([{"image_id": original_id, "category_id": labels[k], "segmentation": rle, "score": scores[k]}
                             for k, rle in enumerate(rles)])
    return coco_results
