"""The device model comparison (object_detectors_amd/compare.py, csrc/compare_kernels.hip) against the literal per-image loop
(tests/disagreement_oracle.py).  Both sides do the same correctly rounded float64 operations in the same order, so best_iou is compared as
bit patterns and best_index, correct and the six counts with ==."""
import numpy as np
import pytest
import torch

from tests import disagreement_cases as dc
from tests import disagreement_oracle as do

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
HAND = dc.hand_cases()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _by_image(rows, image_ids):
    return {i: [r for r in rows if r["image_id"] == i] for i in image_ids}


def _top(rows, image_ids, max_dets):
    """Each image's rows in descending score order (stable), cut to max_dets: what the front end keeps with max_dets given."""
    per = _by_image(rows, image_ids)
    return [r for i in image_ids for r in sorted(per[i], key=lambda r: -r["score"])[:max_dets]]


def _expected(d, dataset, res, thr, conf):
    """best_iou / best_index / correct [2, G] in the slot order of `d`, each (image, model) through the literal form on its own."""
    image_ids = [im["id"] for im in dataset["images"]]
    anns = dataset["annotations"]
    slot_of = {int(pos): s for s, pos in enumerate(d.gt_index)}
    G = len(anns)
    iou, idx, ok = np.zeros((2, G)), -np.ones((2, G), np.int32), np.zeros((2, G), np.uint8)
    for img in image_ids:
        pos = [j for j, a in enumerate(anns) if a["image_id"] == img]
        if not pos:
            continue
        slots = [slot_of[j] for j in pos]
        gt_ann = torch.tensor(do.convert_gt_to_numpy([anns[j] for j in pos]))
        for model in range(2):
            rows = [r for r in res[model] if r["image_id"] == img and r["score"] > conf]
            if not rows:
                continue                                  # -1 / 0 / 0
            right, values, indices = do.right_instances(torch.tensor(do.convert_dt_to_numpy(rows)), gt_ann, thr)
            iou[model, slots], idx[model, slots] = values.numpy(), indices.numpy()
            ok[model, [slots[g] for g in right]] = 1
    return iou, idx, ok


def _check(dataset, res0, res1, thr, conf, max_dets=None, fed=None):
    """Runs the front end on (res0, res1) and compares everything with the literal form fed with `fed` (default: the same lists)."""
    from object_detectors_amd.compare import Disagreement
    d = Disagreement(dataset, device=DEV, max_dets=max_dets)
    d.add_results(0, res0)
    d.add_results(1, res1)
    got = d.run(thr, conf)
    fed = (res0, res1) if fed is None else fed
    want = do.disagreement(dataset, fed[0], fed[1], thr, conf)
    iou, idx, ok = _expected(d, dataset, fed, thr, conf)
    assert d.best_iou.dtype == torch.float64 and d.best_index.dtype == torch.int32 and got["correct"].dtype == torch.uint8
    assert tuple(d.best_iou.shape) == tuple(d.best_index.shape) == tuple(got["correct"].shape) == (2, len(dataset["annotations"]))
    got_iou = d.best_iou.cpu().numpy()
    print("best_iou: differing bit patterns", int((_bits(got_iou) != _bits(iou)).sum()), "of", iou.size, "| NaN on the device",
          int(np.isnan(got_iou).sum()), "in the literal form", int(np.isnan(iou).sum()))
    assert np.array_equal(_bits(got_iou), _bits(iou))
    assert np.array_equal(d.best_index.cpu().numpy(), idx)
    assert np.array_equal(got["correct"].cpu().numpy(), ok)
    assert {k: got[k] for k in dc.COUNT_KEYS} == {k: want[k] for k in dc.COUNT_KEYS}
    return d, got, want


# ---------------------------------------------------------------------------------------------------------------- (a) hand cases
@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_case(case):
    _name, dataset, res0, res1, thr, conf, table = case
    _d, got, _want = _check(dataset, res0, res1, thr, conf)
    assert {k: got[k] for k in dc.COUNT_KEYS} == table


# ---------------------------------------------------------------------------------------------------------------- (b) lanes and chunks
def test_lane_and_chunk_boundaries():
    dataset, res0, res1 = dc.boundary_case()
    per0 = _by_image(res0, [im["id"] for im in dataset["images"]])
    assert sorted(len(v) for v in per0.values()) == [0, 1, 2, 63, 64, 65, 130, 130]
    d, got, want = _check(dataset, res0, res1, .5, 0.)
    assert want["missed"] == 2 and min(want[k] for k in ("yes_yes", "yes_no", "no_yes", "no_no")) > 0
    # the planted ties: the lower index wins at 3 / 70 and at 64 / 65 (wrong label there), and at 5 / 128 (right label there)
    for img in (11, 23):
        first = [j for j, a in enumerate(dataset["annotations"]) if a["image_id"] == img]
        slot = {int(pos): s for s, pos in enumerate(d.gt_index)}
        model = 0
        index, right = d.best_index[model].cpu().numpy(), got["correct"][model].cpu().numpy()
        assert index[slot[first[0]]] == 3 and not right[slot[first[0]]]
        assert index[slot[first[-1]]] == 64 and not right[slot[first[-1]]]
        assert index[slot[first[1]]] == 5 and right[slot[first[1]]]


# ---------------------------------------------------------------------------------------------------------------- (c) seeded random case
@pytest.fixture(scope="module")
def random_case():
    return dc.random_case(dc.RANDOM_SEED)


@pytest.mark.parametrize("thr", [.5, .75])
def test_random_case(random_case, thr):
    dataset, res0, res1 = random_case
    want = do.disagreement(dataset, res0, res1, thr, .3)
    # the literal form alone says that the case is not vacuous
    assert min(want[k] for k in ("yes_yes", "yes_no", "no_yes", "no_no")) > 0
    assert any(bool(torch.isnan(side[1]).any()) for sides in want["images"].values() for side in sides)
    assert want["missed"] <= len(dataset["images"]) // 4
    assert any(r["score"] == .3 for r in res0 + res1)
    d, got, _want = _check(dataset, res0, res1, thr, .3)
    first = (d.best_iou.clone(), d.best_index.clone(), got["correct"].clone(), {k: got[k] for k in dc.COUNT_KEYS})
    again = d.run(thr, .3)                                  # without re-adding; the same bits
    assert torch.equal(first[0].view(torch.int64), d.best_iou.view(torch.int64)) and torch.equal(first[1], d.best_index)
    assert torch.equal(first[2], again["correct"]) and first[3] == {k: again[k] for k in dc.COUNT_KEYS}


def test_run_again_with_other_thresholds(random_case):
    from object_detectors_amd.compare import Disagreement
    dataset, res0, res1 = random_case
    d = Disagreement(dataset, device=DEV)
    d.add_results(0, res0)
    d.add_results(1, res1)
    for thr, conf in ((.5, .3), (.75, 0.), (.5, .3)):
        got, want = d.run(thr, conf), do.disagreement(dataset, res0, res1, thr, conf)
        assert {k: got[k] for k in dc.COUNT_KEYS} == {k: want[k] for k in dc.COUNT_KEYS}


# ---------------------------------------------------------------------------------------------------------------- (d) max_dets
def test_max_dets(random_case):
    dataset, res0, res1 = random_case
    ids = [im["id"] for im in dataset["images"]]
    fed = (_top(res0, ids, 3), _top(res1, ids, 3))
    assert len(fed[0]) < len(res0) and len(fed[1]) < len(res1)
    _d, got, _want = _check(dataset, res0, res1, .5, .3, max_dets=3, fed=fed)
    plain = do.disagreement(dataset, res0, res1, .5, .3)
    assert {k: got[k] for k in dc.COUNT_KEYS} != {k: plain[k] for k in dc.COUNT_KEYS}       # the cut matters on this case


# ---------------------------------------------------------------------------------------------------------------- (e) unknown images
def test_unknown_image_ids_change_nothing(random_case):
    dataset, res0, res1 = random_case
    stray = [dict(res0[j], image_id=10 ** 6 + j) for j in range(5)]
    d0, got0, _ = _check(dataset, res0, res1, .5, .3)
    d1, got1, _ = _check(dataset, stray + res0, res1[:7] + stray + res1[7:], .5, .3, fed=(res0, res1))
    assert torch.equal(d0.best_iou.view(torch.int64), d1.best_iou.view(torch.int64)) and torch.equal(got0["correct"], got1["correct"])
    assert d1.num_added == [len(res0) + 5, len(res1) + 5]


# ---------------------------------------------------------------------------------------------------------------- (f) add == add_results
def test_add_with_device_tensors(random_case):
    from object_detectors_amd.compare import Disagreement
    dataset, res0, res1 = random_case
    ref, want, _ = _check(dataset, res0, res1, .5, .3)
    d = Disagreement(dataset, device=DEV)
    cols = lambda rows: (torch.tensor([r["image_id"] for r in rows], device=DEV), torch.tensor([r["category_id"] for r in rows], device=DEV),
                         torch.tensor([r["score"] for r in rows], dtype=torch.float64, device=DEV),
                         torch.tensor([r["bbox"] for r in rows], dtype=torch.float64, device=DEV).reshape(-1, 4))
    d.add(0, *cols(res0))                                    # one call, an image id per detection
    per1 = _by_image(res1, [im["id"] for im in dataset["images"]])
    per1[10 ** 6] = [dict(res1[0], image_id=10 ** 6)]                      # an image the ground truth does not know
    for img, rows in per1.items():                                         # one call per image, a scalar image id; input order within an image
        _ids, cat, score, box = cols(rows)
        d.add(1, img, cat, score, box)
    got = d.run(.5, .3)
    assert torch.equal(ref.best_iou.view(torch.int64), d.best_iou.view(torch.int64)) and torch.equal(ref.best_index, d.best_index)
    assert torch.equal(want["correct"], got["correct"]) and {k: got[k] for k in dc.COUNT_KEYS} == {k: want[k] for k in dc.COUNT_KEYS}


def test_float32_detections_are_widened_exactly(random_case):
    from object_detectors_amd.compare import Disagreement
    dataset, res0, res1 = random_case
    f32 = lambda rows: [dict(r, bbox=[float(np.float32(v)) for v in r["bbox"]], score=float(np.float32(r["score"]))) for r in rows]
    ref, want, _ = _check(dataset, f32(res0), f32(res1), .5, .3)
    d = Disagreement(dataset, device=DEV)
    for model, rows in enumerate((res0, res1)):
        d.add(model, torch.tensor([r["image_id"] for r in rows], device=DEV), torch.tensor([r["category_id"] for r in rows], device=DEV),
              torch.tensor([r["score"] for r in rows], dtype=torch.float32, device=DEV),
              torch.tensor([r["bbox"] for r in rows], dtype=torch.float32, device=DEV))
    got = d.run(.5, .3)
    assert torch.equal(ref.best_iou.view(torch.int64), d.best_iou.view(torch.int64)) and torch.equal(want["correct"], got["correct"])


def test_empty_sides():
    from object_detectors_amd.compare import Disagreement
    dataset = HAND[0][1]
    d = Disagreement(dataset, device=DEV)
    got = d.run()
    assert {k: got[k] for k in dc.COUNT_KEYS} == {"yes_yes": 0, "yes_no": 0, "no_yes": 0, "no_no": 0, "total": 0, "missed": 1}
    assert d.best_index.cpu().tolist() == [[-1], [-1]] and d.best_iou.cpu().tolist() == [[0.], [0.]] and got["correct"].cpu().tolist() == [[0], [0]]
    none = Disagreement({"images": [{"id": 1}], "categories": [], "annotations": []}, device=DEV)
    none.add_results(0, HAND[0][2])
    got = none.run()
    assert tuple(got["correct"].shape) == (2, 0) and got["total"] == 0 and got["missed"] == 1
