"""COCOEval.summarize_per_category() against the numpy restatement of the rules (tests/cocoeval_oracle.py) run on one category at a time,
which is what the reference's notebooks/get_map.py does with pycocotools (params.catIds = [cat]).  Exact comparison: the per-category
slice holds the same numbers in the same order as a one-category evaluation, and np.mean sums them the same way."""
import io

import numpy as np
import pytest
import torch

from tests import cocoeval_oracle as co

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
CAT_IDS = [5, 2, 9]                               # 9 has no ground truth in the small area range
IMG_IDS = [42, 3, 17, 8, 99, 23]


@pytest.fixture(scope="module")
def small_set():
    rng = np.random.RandomState(3)
    anns, results = [], []
    for img in IMG_IDS:
        for _ in range(rng.randint(2, 7)):
            cat = CAT_IDS[rng.randint(0, 3)]
            side = rng.uniform(40, 120, 2) if cat == 9 else np.exp(rng.uniform(np.log(6), np.log(150), 2))
            box = np.concatenate([rng.rand(2) * 200, side])
            anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": box.tolist(), "area": float(box[2] * box[3]),
                         "iscrowd": int(rng.rand() < .1)})
            for _ in range(rng.randint(0, 4)):    # detections near it, sometimes under another category
                jit = box * (1 + rng.randn(4) * .1)
                jit[2:] = np.maximum(jit[2:], 1.0)
                results.append({"image_id": img, "category_id": cat if rng.rand() < .8 else CAT_IDS[rng.randint(0, 3)], "bbox": jit.tolist(),
                                "score": float(rng.rand())})
        for _ in range(rng.randint(0, 5)):
            box = np.concatenate([rng.rand(2) * 200, rng.uniform(4, 100, 2)])
            results.append({"image_id": img, "category_id": CAT_IDS[rng.randint(0, 3)], "bbox": box.tolist(), "score": float(rng.rand())})
    dataset = {"images": [{"id": i} for i in IMG_IDS], "categories": [{"id": c} for c in CAT_IDS], "annotations": anns}
    assert not any(a["category_id"] == 9 and a["area"] <= 32 ** 2 for a in anns) and any(a["category_id"] == 9 for a in anns)
    assert any(a["category_id"] != 9 and a["area"] < 32 ** 2 for a in anns)
    return dataset, results


@pytest.fixture(scope="module")
def evaluated(small_set):
    from object_detectors_amd.cocoeval import COCOEval
    dataset, results = small_set
    e = COCOEval(dataset, "bbox", device=DEV)
    e.add_results(results)
    return e.evaluate().accumulate()


def test_rows_equal_one_category_evaluations(small_set, evaluated):
    dataset, results = small_set
    got = evaluated.summarize_per_category()
    assert got.shape == (3, 12) and got.dtype == np.float64
    for k, cat in enumerate(evaluated.cat_ids):
        # the restatement takes its categories from the dataset: with one category listed it drops the annotations and results of the others
        want = co.stats(dict(dataset, categories=[{"id": cat}]), results)
        print(cat, got[k].tolist(), want.tolist())
        assert np.array_equal(got[k], want)
    k9 = evaluated.cat_ids.index(9)
    assert got[k9, 3] == -1 and got[k9, 9] == -1 and got[k9, 0] > -1          # no small ground truth: APs and ARs are -1
    assert (got[[k for k in range(3) if k != k9]][:, 3] > -1).all()
    assert len(set(got[:, 0].tolist())) == 3                                  # the categories differ: the rows are not one number repeated


def test_full_summary_is_untouched(small_set, evaluated):
    dataset, results = small_set
    stats = evaluated.summarize(file=io.StringIO())
    kept = stats.copy()
    assert np.array_equal(kept, co.stats(dataset, results))
    evaluated.summarize_per_category()
    assert evaluated.stats is stats and np.array_equal(evaluated.stats, kept)


def test_table_from_evaluators(evaluated):
    from object_detectors_amd import compare
    per = evaluated.summarize_per_category()
    t = compare.per_category_table({"a": evaluated}, metric_columns=(0, 1))
    assert t["columns"] == ["AP", "AP50"] and t["a"]["AP"] == per[:, 0].tolist() and t["a"]["AP50"] == per[:, 1].tolist()
