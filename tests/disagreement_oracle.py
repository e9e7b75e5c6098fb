"""The reference's notebooks/get_disagreement.py:62-100 in its literal form: a Python loop over the images with CPU torch float64, box_iou
restated from its definition, `.max(axis=0)`, the `try / except IndexError` and the sets, in the notebook's order.  Slow and obvious: the
reference the device comparison (object_detectors_amd/compare.py, csrc/compare_kernels.hip) is compared against bit for bit
(tests/test_gpu_compare.py) and that tests/test_oracle_disagreement.py pins with hand-checked cases.  Not imported by the product.

Inputs are plain Python: a COCO dataset dict (`images`, `annotations`) and two lists of result dicts (`image_id`, `category_id`, `score`,
`bbox`); model 0 is the notebook's baseline.  The per-image lists keep dataset / input order, as COCO.getAnnIds gives them."""
import itertools

import numpy as np
import torch


def box_iou(boxes1, boxes2):
    """[N, 4] against [M, 4] boxes [x1, y1, x2, y2] -> [N, M], as torchvision.ops.boxes.box_iou defines it."""
    area1, area2 = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]) for b in (boxes1, boxes2))
    lt, rb = torch.max(boxes1[:, None, :2], boxes2[:, :2]), torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def convert_gt_to_numpy(input_list):
    res = np.array([list(itertools.chain(il["bbox"], [float(il["category_id"])])) for il in input_list])
    res[:, 2:4] += res[:, 0:2]                       # an empty list: a 1-D array, IndexError
    return res


def convert_dt_to_numpy(input_list):
    res = np.array([list(itertools.chain(il["bbox"], [il["score"], float(il["category_id"])])) for il in input_list])
    res[:, 2:4] += res[:, 0:2]
    return res


def best_match(det_ann, gt_ann):
    """det_ann [D, 6] (x1, y1, x2, y2, score, label), gt_ann [G, 5] -> (best IoU [G], best detection [G]); IndexError for D == 0."""
    iou = box_iou(det_ann[:, :4], gt_ann[:, :4])
    return iou.max(axis=0)[0], iou.max(axis=0)[1]


def right_instances(det_ann, gt_ann, iou_true_positives):
    """The notebook's lines 74-80 and 93 for one model -> (the ground truths it gets right, best IoU [G], best detection [G])."""
    iou_values, iou_indices = best_match(det_ann, gt_ann)
    mask = iou_values >= iou_true_positives
    if det_ann[iou_indices[mask]].shape[0] == 0:
        correct = []
    else:
        correct = gt_ann[:, 4][mask] == (det_ann[iou_indices[mask]][:, 5])
    gt = torch.arange(gt_ann.shape[0])
    return gt[mask][correct].tolist(), iou_values, iou_indices


def disagreement(dataset, results0, results1, iou_threshold=0.5, confidence=0.0):
    """-> {"yes_yes", "yes_no", "no_yes", "no_no", "total", "missed", "images": {image id: per model (right instances, best IoU, best index)}
    for the images that were counted}."""
    img_ids = [im["id"] for im in dataset["images"]]
    by_img = lambda rows: {i: [r for r in rows if r["image_id"] == i] for i in img_ids}
    gts, base, det1 = by_img(dataset.get("annotations", [])), by_img(results0), by_img(results1)
    yes_yes = no_yes = yes_no = no_no = missed = total_val_instances = 0
    images = {}
    for img_id in img_ids:
        try:
            gt_ann = torch.tensor(convert_gt_to_numpy(gts[img_id]))
            base_ann = convert_dt_to_numpy(base[img_id])
            det1_ann = convert_dt_to_numpy(det1[img_id])
            det1_ann = torch.tensor(det1_ann[det1_ann[:, 4] > confidence])
            base_ann = torch.tensor(base_ann[base_ann[:, 4] > confidence])
            side1 = right_instances(base_ann, gt_ann, iou_threshold)
            side2 = right_instances(det1_ann, gt_ann, iou_threshold)
            lista1, lista2 = side1[0], side2[0]
            total_val_instances += gt_ann.shape[0]
            yes_no += len(set(lista1) - set(lista2))
            no_yes += len(set(lista2) - set(lista1))
            yes_yes += len(set(lista1) & set(lista2))
            no_no += len(set(torch.arange(gt_ann.shape[0]).tolist()) - (set(lista1) | set(lista2)))
            images[img_id] = (side1, side2)
        except IndexError:
            missed += 1
    return {"yes_yes": yes_yes, "yes_no": yes_no, "no_yes": no_yes, "no_no": no_no, "total": total_val_instances, "missed": missed,
            "images": images}
