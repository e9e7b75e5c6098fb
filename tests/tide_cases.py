"""Inputs for the error breakdown tests: hand cases with their expectations written out, and a seeded generator.

A hand case is {"dataset", "results", "kinds" (one name or None per result, in list order), "partners" (annotation id or None per result),
"missed" (annotation ids)} and, where the prices were worked out, "levels": {state: one entry per category}, the precision curve of the
category in that state: None (no counted ground truth, a -1 cell), a number (the same precision at all 101 recall thresholds) or
(n, first, rest) (the first n thresholds at `first`, the others at `rest`).  States not listed equal "base".

With one ground truth per category the curve is flat: recall is 0 or 1, so every threshold reads the envelope's value at the true positive,
1 / (false positives before it + 1 + 2^-52), or 0 when the ground truth is never found."""
import numpy as np

ONE = 1.0 / (1.0 + 2.0 ** -52)          # tp / (fp + tp + eps) with tp = 1, fp = 0
HALF = 1.0 / (2.0 + 2.0 ** -52)         # one false positive ahead of the true positive: 2 + 2^-52 rounds to 2
A1 = [0., 0., 10., 10.]
FAR = [100., 100., 10., 10.]


def _ann(aid, img, cat, box, crowd=0):
    return {"id": aid, "image_id": img, "category_id": cat, "bbox": list(box), "area": float(box[2] * box[3]), "iscrowd": crowd}


def _det(img, cat, box, score):
    return {"image_id": img, "category_id": cat, "bbox": list(box), "score": score}


def _case(cats, anns, results, kinds, partners, missed, levels=None):
    images = sorted(set([a["image_id"] for a in anns] + [r["image_id"] for r in results]))
    return {"dataset": {"images": [{"id": i} for i in images], "categories": [{"id": c} for c in cats], "annotations": anns},
            "results": results, "kinds": kinds, "partners": partners, "missed": missed, "levels": levels}


def hand_cases():
    c = {}
    # ---- one per kind.  Category 2 always holds one ground truth far away with its true positive (score .8)
    far, far_tp = _ann(2, 1, 2, FAR), _det(1, 2, FAR, .8)
    # Loc: IoU 40 / 100 with the free ground truth of its own category
    c["loc"] = _case([1, 2], [_ann(1, 1, 1, A1), far], [_det(1, 1, [0, 0, 10, 4], .9), far_tp], ["Loc", None], [1, None], [],
                     {"base": [0., ONE], "Loc": [ONE, ONE], "FN": [None, ONE]})
    # Cls: the box of the category-1 ground truth under label 2, ahead of category 2's true positive
    c["cls"] = _case([1, 2], [_ann(1, 1, 1, A1), far], [_det(1, 2, A1, .9), far_tp], ["Cls", None], [1, None], [],
                     {"base": [0., HALF], "Cls": [ONE, ONE], "FP": [0., ONE], "FN": [None, HALF]})
    # Both: IoU .4 with a ground truth of another category only; that ground truth is explained by nothing: Miss
    c["both"] = _case([1, 2], [_ann(1, 1, 1, A1), far], [_det(1, 2, [0, 0, 10, 4], .9), far_tp], ["Both", None], [None, None], [1],
                      {"base": [0., HALF], "Both": [0., ONE], "FP": [0., ONE], "Miss": [None, HALF], "FN": [None, HALF]})
    # Dupe: a second detection (IoU .8) of a taken ground truth, between the two true positives of its category (two images): recall .5 is
    # reached at precision ONE (51 thresholds, 0 .. 0.5), recall 1 at 2 / (3 + 2^-52) = 2 / 3 with the duplicate; without it recall 1 is
    # reached at 2 / (2 + 2^-52) = 1.0, which the envelope carries back over ONE to every threshold
    c["dupe"] = _case([1], [_ann(1, 1, 1, A1), _ann(2, 2, 1, A1)], [_det(1, 1, A1, .9), _det(1, 1, [0, 0, 10, 8], .5), _det(2, 1, A1, .3)],
                      [None, "Dupe", None], [None, None, None], [],
                      {"base": [(51, ONE, 2.0 / 3.0)], "Dupe": [1.0], "FP": [1.0]})
    # Bkg: overlaps nothing
    c["bkg"] = _case([1], [_ann(1, 1, 1, A1)], [_det(1, 1, [200, 200, 10, 10], .9), _det(1, 1, A1, .8)], ["Bkg", None], [None, None], [],
                     {"base": [HALF], "Bkg": [ONE], "FP": [ONE]})
    # Miss: a ground truth without any detection near it
    c["miss"] = _case([1, 2], [_ann(1, 1, 1, A1), far], [far_tp], [None], [None], [1],
                      {"base": [0., ONE], "Miss": [None, ONE], "FN": [None, ONE]})
    # ---- the order of the tests
    # s = .9 (a taken ground truth of its own category) and o = 80 / 90 (a free one of another) both reach fg: Cls, not Dupe
    c["cls_before_dupe"] = _case([1, 2], [_ann(1, 1, 1, A1), _ann(2, 1, 2, [0, 0, 10, 8])], [_det(1, 1, A1, .9), _det(1, 1, [0, 0, 10, 9], .5)],
                                 [None, "Cls"], [None, 2], [],
                                 {"base": [ONE, 0.], "Cls": [ONE, ONE], "FN": [ONE, None]})
    # s = 10 / (10 + 100 - 10) = 0.1 = bg exactly: Loc
    c["s_equals_bg"] = _case([1], [_ann(1, 1, 1, A1)], [_det(1, 1, [0, 0, 10, 1], .9)], ["Loc"], [1], [], {"base": [0.], "Loc": [ONE], "FN": [None]})
    # s = 0 < bg and o = 0.1 = bg exactly: max(s, o) <= bg, Bkg
    c["max_equals_bg"] = _case([1, 2], [_ann(1, 1, 1, FAR), _ann(2, 1, 2, A1)], [_det(1, 1, [0, 0, 10, 1], .9)], ["Bkg"], [None], [1, 2],
                               {"base": [0., 0.], "Miss": [None, None], "FN": [None, None]})
    # ---- claims
    # two Loc detections on one free ground truth: the higher score claims it although it was added later; the loser still explains it
    c["loc_conflict"] = _case([1], [_ann(1, 1, 1, A1)], [_det(1, 1, [0, 0, 10, 4], .6), _det(1, 1, [0, 0, 10, 4.5], .9)], ["Loc", "Loc"], [1, 1], [],
                              {"base": [0.], "Loc": [ONE], "FN": [None]})
    c["loc_conflict"]["loc_winner"] = 1
    # equal scores: the one added first claims it
    c["loc_tie"] = _case([1], [_ann(1, 1, 1, A1)], [_det(1, 1, [0, 0, 10, 4], .7), _det(1, 1, [0, 0, 10, 4.5], .7)], ["Loc", "Loc"], [1, 1], [],
                         {"base": [0.], "Loc": [ONE], "FN": [None]})
    c["loc_tie"]["loc_winner"] = 0
    # a Cls detection whose partner is taken: dropped by the Cls fix, which then prices like dropping it
    c["cls_partner_used"] = _case([1, 2], [_ann(1, 1, 1, A1), far], [_det(1, 1, A1, .95), _det(1, 2, A1, .9), far_tp], [None, "Cls", None],
                                  [None, 1, None], [], {"base": [ONE, HALF], "Cls": [ONE, ONE], "FP": [ONE, ONE]})
    # two Cls detections of different categories on one free partner: the higher score moves, the other is dropped
    c["cls_conflict"] = _case([1, 2, 3], [_ann(1, 1, 1, A1)], [_det(1, 2, A1, .5), _det(1, 3, A1, .7)], ["Cls", "Cls"], [1, 1], [],
                              {"base": [0., None, None], "Cls": [ONE, None, None], "FN": [None, None, None]})
    c["cls_conflict"]["cls_winner"] = 1
    c["cls_tie"] = _case([1, 2, 3], [_ann(1, 1, 1, A1)], [_det(1, 3, A1, .5), _det(1, 2, A1, .5)], ["Cls", "Cls"], [1, 1], [],
                         {"base": [0., None, None], "Cls": [ONE, None, None], "FN": [None, None, None]})
    c["cls_tie"]["cls_winner"] = 0
    # ---- a crowd is invisible: the label-2 detection on it is Bkg (visible it would be Cls), the label-1 detection is matched to it and ignored
    c["crowd"] = _case([1, 2], [_ann(1, 1, 1, A1, crowd=1), far], [_det(1, 2, A1, .9), _det(1, 1, A1, .85), far_tp], ["Bkg", None, None],
                       [None, None, None], [], {"base": [None, HALF], "Bkg": [None, ONE], "FP": [None, ONE]})
    return c


def level_curve(level):
    """One category's entry of "levels" -> its 101 precision values."""
    if level is None:
        return np.full(101, -1.0)
    if isinstance(level, tuple):
        n, first, rest = level
        return np.asarray([first] * n + [rest] * (101 - n), np.float64)
    return np.full(101, float(level))


def expected_ap(levels):
    """The AP50 of one state from its per-category curves: the mean of the valid cells of precision [101, K]."""
    p = np.stack([level_curve(v) for v in levels], 1)
    p = p[p > -1]
    return np.float64(-1) if p.size == 0 else np.mean(p)


def generate(seed, num_images=40, num_cats=12, lvis=False):
    """A seeded data set in which every kind occurs: detections are made by jittering, relabelling, duplicating and dropping ground-truth
    boxes, plus boxes anywhere.  No two ground-truth boxes of an image are identical and no (image, category) gets more than 100 detections,
    moved ones included (an image gets far fewer than 100 in all).  Scores are rounded to two decimals, so ties occur.  Some results carry
    an unknown image or category.  -> (dataset, results)."""
    rng = np.random.RandomState(seed)
    cat_ids = [3 + 2 * k for k in range(num_cats)]
    img_ids = [int(v) for v in rng.permutation(np.arange(1, 4 * num_images))[:num_images]]
    anns, results, images = [], [], []
    other = lambda cat: cat_ids[(cat_ids.index(cat) + 1 + rng.randint(0, num_cats - 1)) % num_cats]
    score = lambda: float(np.round(rng.rand(), 2))
    for img in img_ids:
        seen, present = set(), set()
        for _ in range(int(rng.choice([0, 1, 2, 3, 5, 8, 12]))):
            cat = cat_ids[int(rng.randint(0, num_cats) ** 2 // num_cats)]              # long-tailed
            box = np.concatenate([rng.rand(2) * 300, rng.uniform(20, 120, 2)])
            assert tuple(box) not in seen
            seen.add(tuple(box))
            present.add(cat)
            ann = _ann(len(anns) + 1, img, cat, box.tolist(), crowd=int(not lvis and rng.rand() < .08))
            if lvis:
                ann["ignore"] = int(rng.rand() < .1)
            anns.append(ann)
            tight = lambda: (box * (1 + rng.randn(4) * .03)).tolist()
            loose = lambda: (box + np.asarray([box[2] * rng.uniform(.4, .8) * rng.choice([-1, 1]), 0, 0, 0])).tolist()
            what = rng.choice(["tp", "loc", "cls", "both", "dupe", "miss"], p=[.3, .17, .15, .1, .13, .15])
            if what == "tp":
                results.append(_det(img, cat, tight(), score()))
            elif what == "loc":
                results.extend(_det(img, cat, loose(), score()) for _ in range(rng.randint(1, 3)))
            elif what == "cls":
                results.extend(_det(img, other(cat), tight(), score()) for _ in range(rng.randint(1, 3)))
            elif what == "both":
                results.append(_det(img, other(cat), loose(), score()))
            elif what == "dupe":
                results.extend(_det(img, cat, tight(), score()) for _ in range(rng.randint(2, 4)))
        for _ in range(rng.randint(0, 4)):
            box = np.concatenate([rng.rand(2) * 600, rng.uniform(10, 100, 2)])
            results.append(_det(img, cat_ids[rng.randint(0, num_cats)], box.tolist(), score()))
        if rng.rand() < .1:
            results.append(_det(img, 4, [0., 0., 50., 50.], score()))                  # a category the ground truth does not list
        im = {"id": img}
        if lvis:
            absent = [c for c in cat_ids if c not in present]
            im["neg_category_ids"] = [c for c in absent if rng.rand() < .5]
            im["not_exhaustive_category_ids"] = [c for c in cat_ids if rng.rand() < .15]
        images.append(im)
    results.append(_det(10 ** 6, cat_ids[0], [0., 0., 50., 50.], .99))                 # an image the ground truth does not list
    order = rng.permutation(len(results))
    results = [results[j] for j in order]
    cats = [{"id": c, "frequency": "rcf"[k % 3]} if lvis else {"id": c} for k, c in enumerate(cat_ids)]
    return {"images": images, "categories": cats, "annotations": anns}, results
