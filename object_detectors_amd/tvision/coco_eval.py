"""Mirror of torchvision_models/detection/coco_eval.py: the detection-to-COCO formatting (:83-105 prepare_for_coco_detection, :107-140
prepare_for_coco_segmentation, :142-166 prepare_for_coco_keypoint, :169-171 convert_to_xywh) and CocoEvaluator (:20-81), which scores the detections with the device
evaluator of object_detectors_amd/cocoeval.py instead of pycocotools."""
import json

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


def prepare_for_coco_keypoint(predictions):
    """coco_eval.py:142-166: {image_id: {'scores' [k], 'labels' [k], 'keypoints' [k, K, 3]}} -> list of result dicts with the reference's
    four fields; 'keypoints' is each detection's flat x, y, v list."""
    coco_results = []
    for original_id, prediction in predictions.items():
        if len(prediction) == 0:
            continue
        scores = prediction["scores"].tolist()
        labels = prediction["labels"].tolist()
        keypoints = prediction["keypoints"].flatten(start_dim=1).tolist()
        coco_results.extend([{"image_id": original_id, "category_id": labels[k], "keypoints": keypoint, "score": scores[k]}
                             for k, keypoint in enumerate(keypoints)])
    return coco_results


def get_iou_types(model):
    """detection/engine.py:58-67 (_get_iou_types): what `evaluate` scores for a model - boxes, masks for MaskRCNN, keypoints for KeypointRCNN."""
    from .keypoint_rcnn import KeypointRCNN
    from .mask_rcnn import MaskRCNN
    model = getattr(model, "module", model)
    iou_types = ["bbox"]
    if isinstance(model, MaskRCNN):
        iou_types.append("segm")
    if isinstance(model, KeypointRCNN):
        iou_types.append("keypoints")
    return iou_types


class CocoEvaluator:
    """coco_eval.py:20-81 on top of cocoeval.COCOEval.  update() only stores the predictions (tensors stay where they are; dense masks become
    run lengths at once); evaluation runs in accumulate(), over everything stored, so nothing is copied to the host per batch.  The result
    rows of prepare_for_coco_* are built only by save_detections()."""

    def __init__(self, coco_gt, iou_types):
        from ..cocoeval import COCOEval, load_dataset
        if not isinstance(iou_types, (list, tuple)):
            raise TypeError("CocoEvaluator: iou_types must be a list or tuple")
        for t in iou_types:
            if t not in ("bbox", "segm", "boundary", "keypoints"):
                raise ValueError("Unknown iou type {}".format(t))
        self.coco_gt = load_dataset(coco_gt)
        self.iou_types = list(iou_types)
        self.coco_eval = {t: COCOEval(self.coco_gt, t) for t in self.iou_types}       # keypoints: refused for a data set without any
        self.img_ids = []
        self.predictions = {}                                  # image id -> its prediction, the first one seen

    def update(self, predictions):
        from ..ops import mask_rle_dense
        from ..rle import RLEBatch
        for image_id, prediction in predictions.items():
            if len(prediction) == 0:
                continue
            self.img_ids.append(image_id)
            if image_id in self.predictions:
                continue
            kept = {k: prediction[k].detach() for k in ("boxes", "scores", "labels") if k in prediction}
            if "segm" in self.iou_types or "boundary" in self.iou_types:
                masks = prediction["masks"]
                kept["masks"] = masks if isinstance(masks, RLEBatch) else mask_rle_dense(masks, 0.5)
            if "keypoints" in self.iou_types:
                kept["keypoints"] = prediction["keypoints"].detach()
            self.predictions[image_id] = kept

    def synchronize_between_processes(self):
        """Every rank ends with the detections of all ranks, in rank order; of an image seen on several ranks the first occurrence stays."""
        import torch.distributed as dist
        from ..rle import RLEBatch
        if not (dist.is_available() and dist.is_initialized()):
            return

        def host(v):
            if isinstance(v, RLEBatch):
                return RLEBatch(v.size, v.counts.cpu(), v.offsets, None if v.area is None else v.area.cpu(),
                                None if v.bbox is None else v.bbox.cpu())
            return v.cpu()
        mine = [(image_id, {k: host(v) for k, v in p.items()}) for image_id, p in self.predictions.items()]
        gathered = [None] * dist.get_world_size()
        dist.all_gather_object(gathered, (list(self.img_ids), mine))
        own, self.img_ids, self.predictions = self.predictions, [], {}
        for rank, (img_ids, preds) in enumerate(gathered):
            self.img_ids.extend(img_ids)
            for image_id, p in preds:
                if image_id not in self.predictions:
                    self.predictions[image_id] = own[image_id] if rank == dist.get_rank() else p

    def accumulate(self):
        for iou_type, ev in self.coco_eval.items():
            ev.reset()
            for image_id, p in self.predictions.items():
                dev = ev.device
                if iou_type == "bbox":
                    ev.add(image_id, p["labels"], p["scores"], boxes=convert_to_xywh(p["boxes"].to(dev)))
                elif iou_type == "keypoints":
                    ev.add(image_id, p["labels"], p["scores"], keypoints=p["keypoints"])
                else:
                    ev.add(image_id, p["labels"], p["scores"], masks=p["masks"])
            ev.evaluate()
            ev.accumulate()

    def summarize(self):
        for iou_type, ev in self.coco_eval.items():
            print("IoU metric: {}".format(iou_type))
            ev.summarize()

    def prepare(self, predictions, iou_type):
        if iou_type == "bbox":
            return prepare_for_coco_detection(predictions)
        if iou_type in ("segm", "boundary"):                   # boundary IoU reads the same masks
            return prepare_for_coco_segmentation(predictions)
        if iou_type == "keypoints":
            return prepare_for_coco_keypoint(predictions)
        raise ValueError("Unknown iou type {}".format(iou_type))

    def save_detections(self, path):
        rows = []
        for iou_type in self.iou_types:
            rows.extend(self.prepare(self.predictions, iou_type))
        with open(path, "w") as f:
            json.dump(rows, f, indent=4)
