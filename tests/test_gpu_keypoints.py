"""COCO keypoint evaluation on the device (COCOEval(gt, "keypoints"): csrc/oks_kernels.hip, mi355det_keypoints_match, the unchanged
accumulate) against the literal host form tests/oks_oracle.py, on the seeded sets of tests/keypoint_cases.py: K = 17 with COCO's sigmas and
K = 3 with custom ones.  The host form is computed once per set and shared."""
import io

import numpy as np
import pytest
import torch

from tests import keypoint_cases as kc
from tests import oks_oracle as ko

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CASE_NAMES = sorted(kc.CASES)


def _flatten(ev):
    """The groups of the host form in the device's slot layout: category-major, image second."""
    keys = sorted(ev["groups"])
    groups = [ev["groups"][k] for k in keys]
    I = len(ev["img_ids"])
    cat = lambda name, axis, dtype: np.concatenate([g[name] for g in groups], axis).astype(dtype)
    return {"keys": np.asarray([k * I + i for k, i in keys], np.int64), "iou": np.concatenate([g["iou"].reshape(-1) for g in groups]),
            "dt_offsets": np.cumsum([0] + [len(g["dt"]) for g in groups]), "gt_offsets": np.cumsum([0] + [len(g["gt"]) for g in groups]),
            "dt_match": cat("dt_match", 2, np.int32), "dt_ignore": cat("dt_ignore", 2, np.uint8), "gt_match": cat("gt_match", 2, np.int32),
            "gt_ignore": cat("gt_ignore", 1, np.uint8)}


def _run(dataset, rows, sigmas):
    from object_detectors_amd.cocoeval import COCOEval
    e = COCOEval(dataset, "keypoints", sigmas=sigmas)
    e.add_results(rows)
    return e.evaluate().accumulate()


@pytest.fixture(scope="module")
def sets():
    out = {}
    for name, (K, sigmas, seed) in kc.CASES.items():
        dataset, rows = kc.build(K, seed)
        ev = ko.evaluate(dataset, rows, sigmas)
        precision, recall, scores = ko.accumulate(ev)
        out[name] = {"K": K, "sigmas": sigmas, "dataset": dataset, "rows": rows, "ev": ev, "flat": _flatten(ev), "precision": precision,
                     "recall": recall, "scores": scores, "stats": ko.summarize(precision, recall), "device": _run(dataset, rows, sigmas)}
    return out


@pytest.mark.parametrize("name", CASE_NAMES)
def test_oks_buffer(sets, name):
    """The similarity buffer against the host form within 1e-13 absolute.  The bound is derived, not measured.  Both sides compute the
    argument of every exp with the same correctly rounded float64 operations in the same order, so the arguments are identical.  Each of
    the two exp results (math.exp, the device library's) lies within 1 ulp of the true value, a value <= 1: they differ by at most 2^-52.
    The terms are added in the same order on both sides; with K <= 17 every partial sum is below 32, so an addition rounds by at most
    2^-49 on either side.  The two sums therefore differ by at most 17 * 2^-52 + 17 * 2 * 2^-49 < 6.5e-14, the division by n >= 1 does
    not enlarge that and rounds once more on either side (2^-53 each): below 1e-13.  Where every term is exp(0) the sum and the quotient
    are exact on both sides: those values are compared bit for bit."""
    s = sets[name]
    e, flat = s["device"], s["flat"]
    assert ko.separation_violations(s["ev"]) == []
    host = lambda t: t.cpu().numpy()
    assert np.array_equal(host(e.group_keys), flat["keys"])
    assert np.array_equal(host(e.dt_offsets), flat["dt_offsets"]) and np.array_equal(host(e.gt_offsets), flat["gt_offsets"])
    got = host(e.iou)
    assert got.dtype == np.float64 and got.shape == flat["iou"].shape
    diff = np.abs(got - flat["iou"])
    print(f"{name}: {got.size} similarities, largest difference from the host form {diff.max():.3e}")
    assert diff.max() <= 1e-13
    exact = flat["iou"] == 1.0
    assert exact.sum() >= 2 and np.array_equal(got[exact], flat["iou"][exact])
    assert ((flat["iou"] > 0.05) & (flat["iou"] < 0.95)).sum() > 20 and (flat["iou"] == 0).any()
    again = _run(s["dataset"], s["rows"], s["sigmas"])
    assert torch.equal(again.iou, e.iou) and host(again.iou).tobytes() == got.tobytes()
    assert torch.equal(again.dt_match, e.dt_match) and again.precision.tobytes() == e.precision.tobytes()


@pytest.mark.parametrize("name", CASE_NAMES)
def test_match_tables_and_stats_equal_the_host_form(sets, name):
    """Equal, not close: with the similarities within 1e-13 and (asserted first) no value within 1e-9 of a threshold and no two unequal
    values of a row within 1e-9 of each other, every comparison of the match comes out the same on both sides; the rest is integers and
    the quotients of coco_accumulate."""
    s = sets[name]
    e, flat = s["device"], s["flat"]
    assert ko.separation_violations(s["ev"]) == []
    host = lambda t: t.cpu().numpy()
    for field in ("dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        got = host(getattr(e, field))
        assert got.dtype == flat[field].dtype and np.array_equal(got, flat[field]), field
    assert e.precision.shape == (10, 101, 2, 3, 1) and e.recall.shape == (10, 2, 3, 1)
    for field in ("precision", "recall", "scores"):
        got = getattr(e, field)
        assert got.dtype == np.float64 and got.shape == s[field].shape and np.array_equal(got, s[field]), field
    out = io.StringIO()
    stats = e.summarize(file=out)
    assert stats.shape == (10,) and np.array_equal(stats, s["stats"]) and np.array_equal(e.stats, s["stats"])
    lines = out.getvalue().splitlines()
    assert len(lines) == 10 and all("maxDets= 20" in line for line in lines)
    assert lines[0] == f" Average Precision  (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = {stats[0]:0.3f}"
    assert lines[9] == f" Average Recall     (AR) @[ IoU=0.50:0.95 | area= large | maxDets= 20 ] = {stats[9]:0.3f}"
    assert [line[1:18].strip() for line in lines] == ["Average Precision"] * 5 + ["Average Recall"] * 5
    assert ["IoU=0.50 " in line for line in lines] == [False, True, False, False, False] * 2
    per_cat = e.summarize_per_category()
    assert per_cat.shape == (2, 10) and np.array_equal(per_cat[:, 0], [ko._mean(s["precision"][:, :, k, 0, 0]) for k in range(2)])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_bootstrap_with_unit_weights_reproduces_stats(sets, name):
    s = sets[name]
    e = s["device"]
    boot = e.bootstrap(np.ones((2, len(e.img_ids)), np.int64))
    assert boot.shape == (2, 10) and np.array_equal(boot[0], boot[1])
    # the same cells summed in another order (evalcore.cell_mean): at most 10 * 101 * 2 values <= 1, a relative error of the sum of at most
    # 2020 * 2^-53 = 2.3e-13 on either side
    assert np.abs(boot[0] - s["stats"]).max() <= 1e-12 and np.array_equal(boot[0] == -1, s["stats"] == -1)


def _predictions(rows, K):
    """The result rows as Keypoint R-CNN hands them over: per image xyxy boxes, scores, labels and keypoints [n, K, 3]."""
    preds = {}
    for img in sorted(set(r["image_id"] for r in rows)):
        mine = [r for r in rows if r["image_id"] == img]
        kp = torch.tensor([r["keypoints"] for r in mine], dtype=torch.float64, device=DEV).reshape(-1, K, 3)
        lo, hi = kp[:, :, :2].min(1).values, kp[:, :, :2].max(1).values
        preds[img] = {"boxes": torch.cat([lo, hi], 1).float(), "scores": torch.tensor([r["score"] for r in mine], dtype=torch.float64, device=DEV),
                      "labels": torch.tensor([r["category_id"] for r in mine], dtype=torch.int64, device=DEV), "keypoints": kp}
    return preds


@pytest.mark.parametrize("name", CASE_NAMES)
def test_add_with_tensors_equals_add_results(sets, name):
    from object_detectors_amd.cocoeval import COCOEval
    s = sets[name]
    rows_first = s["device"]
    e = COCOEval(s["dataset"], "keypoints", sigmas=s["sigmas"])
    xy_only = COCOEval(s["dataset"], "keypoints", sigmas=s["sigmas"])
    for img, p in _predictions(s["rows"], s["K"]).items():
        e.add(img, p["labels"], p["scores"], keypoints=p["keypoints"])
        xy_only.add(img, p["labels"], p["scores"], keypoints=p["keypoints"][:, :, :2])
    for ev in (e, xy_only):
        ev.evaluate().accumulate()
        assert ev.num_added == len(s["rows"])
        # another order of addition permutes nothing that is kept: scores are distinct, so the slots are the same
        assert torch.equal(ev.iou, rows_first.iou) and torch.equal(ev.dt_match, rows_first.dt_match)
        assert ev.precision.tobytes() == rows_first.precision.tobytes() and ev.scores.tobytes() == rows_first.scores.tobytes()
        assert np.array_equal(ev.summarize(file=io.StringIO()), s["stats"])


def test_coco_evaluator_with_bbox_and_keypoints(sets, tmp_path):
    import json
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    s = sets["coco17"]
    preds = _predictions(s["rows"], s["K"])
    both, boxes_only = CocoEvaluator(s["dataset"], ["bbox", "keypoints"]), CocoEvaluator(s["dataset"], ["bbox"])
    ids = list(preds)
    both.update({i: preds[i] for i in ids[:2]})
    both.update({i: preds[i] for i in ids[2:]})
    boxes_only.update(preds)
    for ev in (both, boxes_only):
        ev.synchronize_between_processes()              # no process group: a no-op
        ev.accumulate()
        ev.summarize()
    assert np.array_equal(both.coco_eval["keypoints"].stats, s["stats"])
    assert both.coco_eval["bbox"].stats.shape == (12,) and (both.coco_eval["bbox"].stats > 0).any()
    assert np.array_equal(both.coco_eval["bbox"].stats, boxes_only.coco_eval["bbox"].stats)
    both.save_detections(tmp_path / "rows.json")
    saved = json.loads((tmp_path / "rows.json").read_text())
    assert len(saved) == 2 * len(s["rows"]) and sum("keypoints" in r for r in saved) == len(s["rows"])
    assert np.array_equal(ko.stats(s["dataset"], [r for r in saved if "keypoints" in r]), s["stats"])      # float64 survives json


def test_single_pairs_through_the_op():
    """ops.coco_oks on one group against the hand-checked values of tests/test_oracle_oks.py (within the 1e-13 of test_oks_buffer), and
    K = 64, the largest the entry takes.  There the bound of test_oks_buffer's derivation is wider: partial sums below 64 round by at most
    2^-48 on either side, 64 * 2^-52 + 64 * 2 * 2^-48 < 4.7e-13."""
    import math
    from object_detectors_amd import ops
    t = lambda v, *shape: torch.tensor(v, dtype=torch.float64, device=DEV).reshape(*shape)
    off = lambda n: torch.tensor([0, n], dtype=torch.int64, device=DEV)
    dt = t([104.0, 100.0, 55.0, 66.0, 100.0, 100.0, 1e6, -1e6], 2, 2, 2)
    gt = t([100.0, 100.0, 2, 0.0, 0.0, 0], 1, 2, 3)
    got = ops.coco_oks(off(2), off(1), off(2), 2, dt, gt, t([90, 90, 20, 20], 1, 4), t([8.0], 1), t([1.0, 1.0], 2)).cpu().tolist()
    assert abs(got[0] - math.exp(-1.0)) <= 1e-13 and got[1] == 1.0
    blank = t([0.0] * 6, 1, 2, 3)
    dt = t([-10.0, 50.0, 20.0, 30.0, 20.0, 30.0, 53.0, 12.0], 2, 2, 2)
    got = ops.coco_oks(off(2), off(1), off(2), 2, dt, blank, t([10, 10, 20, 20], 1, 4), t([4.5], 1), t([1.0, 1.0], 2)).cpu().tolist()
    assert got[0] == 1.0 and abs(got[1] - (1.0 + math.exp(-1.0)) / 2) <= 1e-13
    rng = np.random.RandomState(64)
    K, D, G = 64, 5, 11
    gk = np.concatenate([rng.rand(G, K, 2) * 100, rng.randint(0, 3, (G, K, 1))], 2)
    dk = gk[rng.randint(0, G, D), :, :2] + rng.randn(D, K, 2) * 3
    box, area, sig = np.tile([0.0, 0.0, 100.0, 100.0], (G, 1)), 2000 + 6000 * rng.rand(G), 0.03 + 0.1 * rng.rand(K)
    want = np.asarray([[ko.oks_pair(dk[d].reshape(-1), gk[g].reshape(-1), box[g], area[g], ko.variances(sig)) for g in range(G)] for d in range(D)])
    got = ops.coco_oks(off(D), off(G), off(D * G), D * G, t(dk, D, K, 2), t(gk, G, K, 3), t(box, G, 4), t(area, G), t((sig * 2) ** 2, K))
    assert np.abs(got.cpu().numpy().reshape(D, G) - want).max() <= 4.7e-13
    with pytest.raises(ValueError):
        ops.coco_oks(off(D), off(G), off(D * G), D * G, t(dk, D, K, 2), t(gk, G, K, 3), t(box, G, 4), t(area, G), t((sig[:5] * 2) ** 2, 5))
