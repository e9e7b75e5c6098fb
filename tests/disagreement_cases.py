"""Inputs shared by tests/test_oracle_disagreement.py (CPU) and tests/test_gpu_compare.py: hand-checked cases with their expected tables,
the lane / chunk boundary case and a seeded random case.  Plain Python dicts, as tests/disagreement_oracle.py takes them."""
import numpy as np


def _ann(image_id, bbox, label):
    return {"image_id": image_id, "bbox": [float(v) for v in bbox], "category_id": int(label)}


def _det(image_id, bbox, label, score):
    return {"image_id": image_id, "bbox": [float(v) for v in bbox], "category_id": int(label), "score": float(score)}


def _dataset(image_ids, anns):
    return {"images": [{"id": i} for i in image_ids], "categories": [{"id": c} for c in range(1, 6)],
            "annotations": [dict(a, id=j + 1) for j, a in enumerate(anns)]}


def _table(yes_yes=0, yes_no=0, no_yes=0, no_no=0, missed=0):
    return {"yes_yes": yes_yes, "yes_no": yes_no, "no_yes": no_yes, "no_no": no_no, "total": yes_yes + yes_no + no_yes + no_no, "missed": missed}


COUNT_KEYS = ("yes_yes", "yes_no", "no_yes", "no_no", "total", "missed")
BOX = [10, 10, 20, 20]
FAR = [200, 200, 5, 5]


def hand_cases():
    """[(name, dataset, results of model 0, results of model 1, iou_threshold, confidence, expected counts)], each worked out by hand."""
    cases = []
    # model 0 finds the instance with the right label, model 1 finds it with the wrong one
    cases.append(("wrong_label", _dataset([7], [_ann(7, BOX, 3)]), [_det(7, BOX, 3, .9)], [_det(7, BOX, 4, .9)], .5, 0., _table(yes_no=1)))
    # the same box twice with different labels: both reach IoU 1, the lower index decides
    cases.append(("tie", _dataset([7], [_ann(7, BOX, 1)]), [_det(7, BOX, 2, .9), _det(7, BOX, 1, .8)],
                  [_det(7, BOX, 1, .9), _det(7, BOX, 2, .8)], .5, 0., _table(no_yes=1)))
    # a zero-area ground truth and a zero-area detection apart from each other: union 0, IoU 0 / 0 = NaN, which beats the 0 of the detection
    # that covers the point.  At threshold 0 that 0 would have been enough (model 1, which lacks the zero-area detection, gets it right).
    point, cover = [5, 5, 0, 0], [0, 0, 10, 10]
    cases.append(("nan_column", _dataset([7], [_ann(7, point, 1), _ann(7, cover, 1)]),
                  [_det(7, cover, 1, .9), _det(7, [80, 80, 0, 0], 1, .8)], [_det(7, cover, 1, .9)], 0., 0., _table(yes_yes=1, no_yes=1)))
    # a score equal to the confidence is dropped (strict >); the far detection keeps the image counted for model 0
    cases.append(("score_equals_confidence", _dataset([7], [_ann(7, BOX, 2)]), [_det(7, BOX, 2, .3), _det(7, FAR, 2, .9)],
                  [_det(7, BOX, 2, .31)], .5, .3, _table(no_yes=1)))
    # image 9 has an annotation but no detection of model 1: missed, absent from the total.  Image 4 counts.
    cases.append(("no_detections_of_one_model", _dataset([9, 4], [_ann(9, BOX, 1), _ann(4, BOX, 1)]),
                  [_det(9, BOX, 1, .9), _det(4, BOX, 1, .9)], [_det(4, BOX, 1, .9)], .5, 0., _table(yes_yes=1, missed=1)))
    # image 9 has detections of both models and no annotation: missed.  Image 4: both models wrong (no overlap).
    cases.append(("no_annotations", _dataset([9, 4], [_ann(4, BOX, 1)]), [_det(9, BOX, 1, .9), _det(4, FAR, 1, .9)],
                  [_det(9, BOX, 1, .9), _det(4, FAR, 1, .9)], .5, 0., _table(no_no=1, missed=1)))
    return cases


def boundary_case():
    """Detection counts per image of 0, 1, 63, 64, 65 and 130 (model 1 gets them in reverse image order), ground-truth counts of 1, 4, 5 and
    9; in the 130-detection images the best box is duplicated at indices 3 and 70 (a tie across chunks of 64) and another at 64 and 65
    (across lanes of the second chunk), each time with the right label at the higher index only, and a third at 5 and
    128 (the higher index on the lower lane) with the right label at the lower index.
    -> dataset, results of model 0, results of model 1."""
    rng = np.random.RandomState(5)
    det_counts, gt_counts = [0, 1, 63, 64, 65, 130, 130, 2], [1, 4, 5, 9, 1, 9, 5, 4]
    image_ids = [31, 2, 17, 5, 40, 11, 23, 8]
    anns, res = [], ([], [])
    for n, img in enumerate(image_ids):
        gts = [np.concatenate([rng.randint(0, 50, 2) * 4.0, rng.randint(2, 12, 2) * 4.0]) for _ in range(gt_counts[n])]
        labels = rng.randint(1, 6, gt_counts[n])
        anns += [_ann(img, b, l) for b, l in zip(gts, labels)]
        for model in range(2):
            nd = det_counts[n] if model == 0 else det_counts[len(det_counts) - 1 - n]
            dets = []
            for d in range(nd):
                g = rng.randint(0, len(gts))
                jit = gts[g] + np.concatenate([rng.randint(-2, 3, 2) * 2.0, rng.randint(0, 3, 2) * 2.0]) + 1.0      # never the exact box
                dets.append(_det(img, jit, labels[g] if rng.rand() < .6 else 1 + (labels[g] % 5), rng.rand() * .9 + .05))
            if nd == 130:
                wrong = lambda l: 1 + (l % 5)
                dets[3], dets[70] = _det(img, gts[0], wrong(labels[0]), .5), _det(img, gts[0], labels[0], .6)
                last = len(gts) - 1
                dets[65], dets[64] = _det(img, gts[last], labels[last], .5), _det(img, gts[last], wrong(labels[last]), .6)
                dets[5], dets[128] = _det(img, gts[1], labels[1], .5), _det(img, gts[1], wrong(labels[1]), .6)       # 128 is lane 0 again
            res[model].extend(dets)
    return _dataset(image_ids, anns), res[0], res[1]


def random_case(seed, images=40):
    """About `images` images, half with integer-valued boxes on a grid of 4 (zero widths and heights occur, exact copies of ground truths
    occur: ties, IoU 1, NaN columns), half with fractional boxes; labels from 5 categories; some scores exactly 0.3.
    -> dataset, results of model 0, results of model 1."""
    rng = np.random.RandomState(seed)
    image_ids = [int(v) for v in rng.permutation(np.arange(1, 3 * images))[:images]]
    anns, res = [], ([], [])
    for n, img in enumerate(image_ids):
        grid = n % 2 == 0
        ng = 0 if rng.rand() < .05 else rng.randint(1, 8)

        def box():
            if grid:
                return np.concatenate([4.0 * rng.randint(0, 8, 2), 4.0 * rng.randint(0, 6, 2)])
            return np.concatenate([rng.rand(2) * 40, rng.rand(2) * 30 + .5])
        gts, labels = [box() for _ in range(ng)], rng.randint(1, 6, ng)
        anns += [_ann(img, b, l) for b, l in zip(gts, labels)]
        for model in range(2):
            nd = 0 if rng.rand() < .05 else rng.randint(1, 14)
            for _ in range(nd):
                if ng and rng.rand() < .65:
                    g = rng.randint(0, ng)
                    if grid and rng.rand() < .5:
                        b = gts[g]
                    elif grid:
                        b = gts[g] + np.concatenate([4.0 * rng.randint(-1, 2, 2), 4.0 * rng.randint(0, 2, 2)])
                    else:
                        b = gts[g] * (1 + rng.randn(4) * .06)
                    label = labels[g] if rng.rand() < .7 else rng.randint(1, 6)
                else:
                    b, label = box(), rng.randint(1, 6)
                score = .3 if rng.rand() < .1 else rng.rand()
                res[model].append(_det(img, b, label, score))
    # detections arrive image-interleaved, not grouped
    for model in range(2):
        order = rng.permutation(len(res[model]))
        res[model][:] = [res[model][j] for j in order]
    return _dataset(image_ids, anns), res[0], res[1]


RANDOM_SEED = 0
