"""The device error breakdown (object_detectors_amd/tide.py, csrc/tide_kernels.hip) against its literal form (tests/tide_oracle.py) with ==:
kinds, partners, the two overlaps as bit patterns, the flag arrays of every fix and the prices.  Same-category overlaps are also the bits the
evaluator's own IoU pass wrote.  The shapes are the smallest at which the kernels can go wrong: empty images, 1 / 63 / 64 / 65 / 130 false
positives on an image (lane striding and its tail), 63 / 64 / 65 counted ground truths (the staging chunk is 64), nothing but true positives
(idle lanes), ties."""
import io

import numpy as np
import pytest
import torch

from tests import tide_cases, tide_oracle
from tests.tide_cases import _ann, _det

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CHUNK = 64                                                        # TIDE_CHUNK of csrc/tide_kernels.hip
HAND = tide_cases.hand_cases()
EV_ARRAYS = ("iou", "iou_offsets", "dt_offsets", "gt_offsets", "dt_match", "dt_ignore", "gt_match", "gt_ignore", "dt_score", "dt_boxes", "dt_index",
             "dt_rank", "cat_dt_offsets", "cat_gt_offsets", "dt_image", "gt_image")


def evaluated(dataset, results, lvis=False):
    if lvis:
        from object_detectors_amd.lviseval import LVISEval
        return LVISEval(dataset, results, device=DEV).evaluate()
    from object_detectors_amd.cocoeval import COCOEval
    ev = COCOEval(dataset, "bbox", device=DEV)
    ev.add_results(results)
    return ev.evaluate()


def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def check(dataset, results, lvis=False):
    """Evaluate, break down, compare everything with the literal form.  -> (evaluator, breakdown, result dict, the literal form)."""
    from object_detectors_amd.tide import ErrorBreakdown
    an = tide_oracle.analyse(dataset, results, lvis=lvis)
    ev = evaluated(dataset, results, lvis)
    before = {k: getattr(ev, k).clone() for k in EV_ARRAYS}
    b = ErrorBreakdown(ev)
    res = b.run()
    host = lambda t: t.cpu().numpy()
    nd, ng = len(an["dt_items"]), len(an["gt_items"])
    assert (ev.num_dt, ev.num_gt) == (nd, ng)
    assert np.array_equal(host(b.kind), an["kind"]) and np.array_equal(host(b.partner), an["partner"])
    assert np.array_equal(host(b.missed), an["missed"])
    assert np.array_equal(bits(host(b.best_same)), bits(an["best_same"])) and np.array_equal(bits(host(b.best_other)), bits(an["best_other"]))
    assert np.array_equal(host(b.fix_dt_match).reshape(8, nd) != 0, an["fix_dt_match"] != 0)
    assert np.array_equal(host(b.fix_dt_ignore).reshape(8, nd), an["fix_dt_ignore"])
    assert np.array_equal(host(b.fix_gt_ignore), an["fix_gt_ignore"])
    assert np.array_equal(host(b.cls_cat), an["cls_cat"]) and np.array_equal(host(b.cls_match) != 0, an["cls_match"] != 0)
    assert np.array_equal(host(b.cls_ignore), an["cls_ignore"])
    for key in ("counts", "counts_per_category", "ap_fixed", "dap", "ap_per_category", "dap_per_category", "dap_per_frequency"):
        if key in an or key in res:
            print(key, np.asarray(res[key]).tolist(), np.asarray(an[key]).tolist())
            np.testing.assert_array_equal(res[key], an[key])      # ==, with NaN (a price without a counted ground truth) equal to NaN
            assert np.asarray(res[key]).dtype == np.asarray(an[key]).dtype
    assert res["ap_base"] == an["ap_base"]
    assert res["counts"][:5].sum() == res["counts"][6]
    # same-category overlaps are the evaluator's own: iou[iou_offsets[group] + d * G + g] of the detection's group
    dt_off, gt_off, iou_off, iou = (host(getattr(ev, k)) for k in ("dt_offsets", "gt_offsets", "iou_offsets", "iou"))
    same, partner, kind = host(b.best_same), host(b.partner), host(b.kind)
    seen = 0
    for d in np.flatnonzero(kind == tide_oracle.LOC):
        j = int(np.searchsorted(dt_off, d, side="right")) - 1
        G = int(gt_off[j + 1] - gt_off[j])
        g = int(partner[d]) - int(gt_off[j])
        assert 0 <= g < G
        assert bits(same[d:d + 1])[0] == bits(iou[int(iou_off[j]) + (d - int(dt_off[j])) * G + g: int(iou_off[j]) + (d - int(dt_off[j])) * G + g + 1])[0]
        seen += 1
    # the evaluator is only read
    for k, v in before.items():
        assert torch.equal(getattr(ev, k), v), k
    # AP50 of the base state is the evaluator's own
    ev.accumulate()
    own = ev.summarize()["AP50"] if lvis else ev.summarize(file=io.StringIO())[1]
    assert res["ap_base"] == own
    return ev, b, res, an, seen


# ---- the hand cases, with their written-out expectations checked on the device result itself
@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_case(name):
    case = HAND[name]
    _ev, b, res, an, _seen = check(case["dataset"], case["results"])
    slot = {id(r): d for d, r in enumerate(an["dt_items"])}
    names = (None,) + tide_oracle.KINDS[:5]
    kind, partner = b.kind.cpu().numpy(), b.partner.cpu().numpy()
    for j, r in enumerate(case["results"]):
        assert names[kind[slot[id(r)]]] == case["kinds"][j]
        p = partner[slot[id(r)]]
        assert (None if p < 0 else an["gt_items"][int(p)]["id"]) == case["partners"][j]
    levels = case["levels"]
    assert res["ap_base"] == tide_cases.expected_ap(levels["base"])
    for j, fix in enumerate(tide_oracle.FIXES):
        assert res["ap_fixed"][j] == tide_cases.expected_ap(levels.get(fix, levels["base"])), fix


def test_every_ground_truth_of_a_category_missed():
    _ev, _b, res, _an, _seen = check(HAND["max_equals_bg"]["dataset"], HAND["max_equals_bg"]["results"])
    miss, fn = tide_oracle.FIXES.index("Miss") + 1, tide_oracle.FIXES.index("FN") + 1
    assert (res["ap_per_category"][:, [miss, fn]] == -1).all() and (res["ap_per_category"][:, 0] == 0).all()
    assert np.isnan(res["dap"][[miss - 1, fn - 1]]).all() and np.isnan(res["dap_per_category"][:, [miss - 1, fn - 1]]).all()


# ---- empty things
def test_empty_images_and_empty_evaluator():
    anns = [_ann(1, 2, 1, [0, 0, 10, 10]), _ann(2, 2, 2, [30, 0, 10, 10]), _ann(3, 4, 1, [0, 0, 10, 10])]
    results = [_det(2, 1, [0, 0, 10, 4], .9), _det(3, 2, [0, 0, 10, 10], .8), _det(3, 1, [5, 5, 10, 10], .8)]
    dataset = {"images": [{"id": i} for i in (1, 2, 3, 4, 5)], "categories": [{"id": 1}, {"id": 2}], "annotations": anns}
    _ev, _b, res, _an, _seen = check(dataset, results)            # image 1, 5: neither; 3: detections only; 4: ground truth only
    assert res["counts"].tolist() == [0, 1, 0, 0, 2, 2, 3]
    for empty in ({"images": [{"id": 1}], "categories": [{"id": 1}], "annotations": []}, {"images": [], "categories": [], "annotations": []}):
        _ev, b, res, _an, _seen = check(empty, [_det(1, 7, [0, 0, 1, 1], .5)])
        assert res["counts"].tolist() == [0] * 7 and res["ap_base"] == -1 and np.isnan(res["dap"]).all()
        assert b.kind.shape == (0,) and b.missed.shape == (0,)


# ---- lane striding: 1, 63, 64, 65 and 130 false positives on one image each, of every kind, with true positives in between
def _crowded_image(img, rng, num_fp, num_gt, cats):
    anns, results = [], []
    for n in range(num_gt):
        box = [40. * (n % 13) + float(rng.rand()), 40. * (n // 13) + float(rng.rand()), 30., 30.]
        anns.append(_ann(0, img, cats[n % len(cats)], box, crowd=int(n % 11 == 10)))
        if n % 3 == 0:
            results.append(_det(img, cats[n % len(cats)], box, float(np.round(rng.rand(), 2))))            # a true positive
    exact = [n for n in range(num_gt) if n % 3 == 0 and n % 11 != 10]            # the ground truths that have their true positive
    for n in range(num_fp):                                       # each of these ends up a false positive: the image holds num_fp exactly
        what = n % 5                                              # loose, nowhere, duplicate, relabelled, loose and relabelled
        a = anns[exact[rng.randint(0, len(exact))] if what == 2 else rng.randint(0, num_gt)]
        box = np.asarray(a["bbox"])
        if what in (0, 4):
            box = box + [18, 0, 0, 0]
        elif what == 1:
            box = np.asarray([1000. + 40 * n, 1000., 20., 20.])
        cat = a["category_id"] if what in (0, 1, 2) else cats[(cats.index(a["category_id"]) + 1) % len(cats)]
        results.append(_det(img, cat, (box + rng.rand(4) * (0 if what == 2 else 2)).tolist(), float(np.round(rng.rand(), 2))))
    return anns, results


def _assemble(parts, cats):
    anns = [a for p in parts for a in p[0]]
    for n, a in enumerate(anns):
        a["id"] = n + 1
    results = [r for p in parts for r in p[1]]
    images = sorted(set(a["image_id"] for a in anns) | set(r["image_id"] for r in results))
    return {"images": [{"id": i} for i in images], "categories": [{"id": c} for c in cats], "annotations": anns}, results


def test_lane_striding():
    rng, cats = np.random.RandomState(5), [1, 2, 3]
    dataset, results = _assemble([_crowded_image(10 + n, rng, n, 9, cats) for n in (1, 63, 64, 65, 130)], cats)
    ev, b, res, _an, seen = check(dataset, results)
    per_image = torch.bincount(ev.dt_image.to(torch.int64)[b.kind != 0], minlength=5).tolist()
    print(per_image, res["counts"].tolist(), seen)
    assert per_image == [1, 63, 64, 65, 130] and (res["counts"][:5] > 0).all() and seen > 0


def test_ground_truth_chunks():
    """63, 64 and 65 counted ground truths on an image (with uncounted ones in between, which the staging squeezes out), the last image with
    more than 64 detections as well, so that the chunks are staged again for the second batch of lanes."""
    rng, cats = np.random.RandomState(6), [1, 2, 3, 4]
    parts = []
    for img, counted, num_fp in ((1, CHUNK - 1, 20), (2, CHUNK, 20), (3, CHUNK + 1, 130)):
        total = counted
        while sum(1 for n in range(total) if n % 11 != 10) < counted:
            total += 1
        parts.append(_crowded_image(img, rng, num_fp, total, cats))
        assert sum(1 for a in parts[-1][0] if not a["iscrowd"]) == counted
    dataset, results = _assemble(parts, cats)
    _ev, _b, res, _an, seen = check(dataset, results)
    assert (res["counts"][:5] > 0).all() and seen > 0


def test_all_true_positives():
    rng, cats = np.random.RandomState(7), [1, 2]
    anns, _ = _crowded_image(1, rng, 0, 70, cats)
    anns = [dict(a, iscrowd=0) for a in anns]
    results = [_det(1, a["category_id"], a["bbox"], float(np.round(rng.rand(), 2))) for a in anns]
    dataset, results = _assemble([(anns, results)], cats)
    _ev, b, res, _an, _seen = check(dataset, results)
    assert res["counts"].tolist() == [0] * 7 and int(b.kind.sum()) == 0 and (res["dap"] == 0).all() and res["ap_base"] == 1.0


def test_ties():
    """Equal overlaps: the lowest slot is the partner, in the own category and in the others.  Equal scores: the detection added first claims."""
    left, right = [0., 0., 10., 10.], [20., 0., 10., 10.]
    between = [5., 0., 20., 10.]                                  # IoU 50 / 250 with both
    anns = [_ann(1, 1, 2, right), _ann(2, 1, 2, left), _ann(3, 2, 1, left), _ann(4, 2, 3, right)]
    results = [_det(1, 2, between, .5), _det(1, 2, between, .5), _det(2, 2, between, .4), _det(2, 2, [0, 0, 10, 9], .5), _det(2, 3, [0, 0, 10, 9], .5)]
    dataset = {"images": [{"id": 1}, {"id": 2}], "categories": [{"id": 1}, {"id": 2}, {"id": 3}], "annotations": anns}
    _ev, b, _res, an, _seen = check(dataset, results)
    slot = {id(r): d for d, r in enumerate(an["dt_items"])}
    partner_id = lambda j: an["gt_items"][int(b.partner[slot[id(results[j])]])]["id"]
    assert partner_id(0) == 1 and partner_id(1) == 1             # annotation 1 holds the lower slot of the two
    assert b.best_same[slot[id(results[0])]].item() == 0.2
    assert b.kind[slot[id(results[2])]].item() == tide_oracle.BOTH and b.best_other[slot[id(results[2])]].item() == 0.2
    match = b.fix_dt_match[1, 0].cpu().numpy()
    assert match[slot[id(results[0])]] == 1 and match[slot[id(results[1])]] == 0
    cls = b.cls_match.cpu().numpy()
    assert cls[slot[id(results[3])]] == 1 and cls[slot[id(results[4])]] == 0          # both Cls on annotation 3, equal scores


# ---- generated cases
@pytest.mark.parametrize("seed", (21, 22, 23))
def test_generated(seed):
    dataset, results = tide_cases.generate(seed, num_images=40, num_cats=12)
    ev, _b, res, _an, seen = check(dataset, results)
    assert ev.num_dt < len(results)                               # the results of an unknown image or category stay dropped
    assert (res["counts"] > 0).all() and seen > 0


def test_lvis():
    dataset, results = tide_cases.generate(31, num_images=30, num_cats=12, lvis=True)
    assert any(im["neg_category_ids"] for im in dataset["images"]) and any(im["not_exhaustive_category_ids"] for im in dataset["images"])
    assert any(a["ignore"] for a in dataset["annotations"])
    _ev, _b, res, _an, seen = check(dataset, results, lvis=True)
    assert res["dap_per_frequency"].shape == (3, 8) and (res["counts"] > 0).all() and seen > 0


def test_two_runs_are_the_same_bits():
    from object_detectors_amd.tide import ErrorBreakdown
    dataset, results = tide_cases.generate(22, num_images=40, num_cats=12)
    ev = evaluated(dataset, results)
    runs = []
    for _ in range(2):
        b = ErrorBreakdown(ev)
        res = b.run()
        runs.append(([getattr(b, k).clone() for k in ("kind", "partner", "best_same", "best_other", "missed", "fix_dt_match", "fix_dt_ignore",
                                                        "fix_gt_ignore", "cls_cat", "cls_match", "cls_ignore")], res))
    for x, y in zip(runs[0][0], runs[1][0]):
        assert torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x, y.view(torch.int64) if y.dtype == torch.float64 else y)
    for key in ("ap_fixed", "dap", "ap_per_category", "counts"):
        assert np.array_equal(bits(runs[0][1][key]) if runs[0][1][key].dtype == np.float64 else runs[0][1][key],
                              bits(runs[1][1][key]) if runs[1][1][key].dtype == np.float64 else runs[1][1][key])


def test_report_prints_the_table():
    from object_detectors_amd.tide import ErrorBreakdown
    case = HAND["both"]
    b = ErrorBreakdown(evaluated(case["dataset"], case["results"]))
    b.run()
    out = io.StringIO()
    b.report(file=out)
    lines = out.getvalue().splitlines()
    assert lines[0].endswith("AP50 = 25.00") and lines[4].split() == ["Both", "1", "25.00"] and "do not add up" in lines[-1]
