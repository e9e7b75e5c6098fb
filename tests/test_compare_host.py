"""Host side of the model comparison (object_detectors_amd/compare.py, COCOEval.summarize_per_category): McNemar's test, the report text,
the per-category table on hand-made arrays and the argument checks.  CPU only: nothing here launches a kernel."""
import io
import math

import numpy as np
import pytest
import torch

from object_detectors_amd import compare
from object_detectors_amd.cocoeval import COCOEval

DATASET = {"images": [{"id": 1}, {"id": 2}], "categories": [{"id": 3}, {"id": 5}, {"id": 8}],
           "annotations": [{"id": 1, "image_id": 1, "category_id": 3, "bbox": [0., 0., 4., 4.], "area": 16., "iscrowd": 0}]}


def test_mcnemar_against_chi2():
    """The survival function of chi-square with one degree of freedom.  The bar: erfc and chi2.sf are both accurate to a few ulp of the
    result, and the argument sqrt(s / 2) carries one rounding that the tail amplifies by about s (d ln erfc(sqrt(s/2)) / d ln s ~ s / 2 for
    large s): over this grid s stays below 3000, so 1e-11 leaves a factor of about 20 over the 5.3e-13 measured with this libm.
    Below the normal range (p < 2.2e-308, s above about 1410) a double is spaced 4.9e-324 apart whatever its size, so no relative bound can
    hold there (chi2.sf gives 0 where erfc still gives 3.5e-323); there both sides only have to agree that p is below the normal range."""
    from scipy.stats import chi2
    grid = sorted(set(list(range(0, 40)) + [50, 64, 99, 100, 250, 500, 999, 1000, 1500, 2000, 2999, 3000]))
    worst = 0.0
    for b in grid:
        for c in grid:
            if b + c == 0:
                continue
            stat, p = compare.mcnemar(b, c)
            assert stat == (abs(b - c) - 1) ** 2 / (b + c)
            want = float(chi2.sf(stat, 1))
            if want < 2.3e-308:                                  # subnormal or zero: see the docstring
                assert 0.0 <= p < 2.3e-308, (b, c, p, want)
                continue
            worst = max(worst, abs(p - want) / want)
            assert math.isclose(p, want, rel_tol=1e-11), (b, c, p, want)
    print("worst relative difference", worst)


def test_mcnemar_fixed_values():
    assert compare.mcnemar(0, 0) == (0.0, 1.0)                   # the documented deviation: the bare formula is 0 / 0
    stat, p = compare.mcnemar(10, 20)
    assert stat == 81 / 30
    assert p == math.erfc(math.sqrt(81 / 60)) and abs(p - 0.100348) < 1e-6
    assert compare.mcnemar(20, 10) == (stat, p)
    assert compare.mcnemar(1, 0) == (0.0, 1.0)                    # |b - c| - 1 = 0
    with pytest.raises(ValueError):
        compare.mcnemar(-1, 3)


def _with_result(table):
    d = compare.Disagreement(DATASET, device="cpu")
    d.result = dict(table, iou_threshold=0.5, confidence=0.0)
    return d


def test_report_text():
    d = _with_result({"yes_yes": 120, "yes_no": 10, "no_yes": 20, "no_no": 7})
    out = io.StringIO()
    stat, p = d.report(alpha=0.05, file=out)
    assert (stat, p) == compare.mcnemar(10, 20)
    assert out.getvalue().splitlines() == [
        "+------------+----------+------------+",
        "|  IoU@0.5   | Correct2 | Incorrect2 |",
        "+------------+----------+------------+",
        "|  Correct1  |   120    |     10     |",
        "| Incorrect1 |    20    |     7      |",
        "+------------+----------+------------+",
        "McNemar's test:",
        "statistic=2.7000, p-value=0.1003",
        "Same proportions of errors (fail to reject H0)"]
    out = io.StringIO()
    d.report(alpha=0.2, file=out)
    assert out.getvalue().splitlines()[-1] == "Different proportions of errors (reject H0)"
    with pytest.raises(RuntimeError):
        compare.Disagreement(DATASET, device="cpu").report()


def _hand_evaluator():
    """precision [10, 101, 3, 4, 3] / recall [10, 3, 4, 3] filled by hand: category 0 constant per threshold, category 1 with -1 in the small
    range, category 2 all -1."""
    e = COCOEval(DATASET, device="cpu")
    p, r = -np.ones((10, 101, 3, 4, 3)), -np.ones((10, 3, 4, 3))
    p[:, :, 0] = np.linspace(1.0, 0.1, 10)[:, None, None, None]          # AP = mean = 0.55, AP50 = 1.0, AP75 = 0.5
    r[:, 0] = 0.25
    p[:, :, 1] = 0.5
    p[:, :, 1, 1] = -1
    r[:, 1] = np.asarray([0.125, 0.25, 0.375])[None, None, :]
    r[:, 1, 1] = -1
    e.precision, e.recall = p, r
    return e


def test_summarize_per_category_by_hand():
    e = _hand_evaluator()
    s = e.summarize_per_category()
    assert s.shape == (3, 12) and s.dtype == np.float64
    assert s[0, 0] == np.mean(np.repeat(np.linspace(1.0, 0.1, 10), 101)) and s[0, 1] == 1.0 and s[0, 2] == np.linspace(1.0, 0.1, 10)[5]
    assert (s[0, 6:] == 0.25).all()
    assert s[1].tolist() == [.5, .5, .5, -1, .5, .5, .125, .25, .375, -1, .375, .375]
    assert (s[2] == -1).all()
    assert e.stats is None                                       # nothing summarised, nothing printed
    with pytest.raises(RuntimeError):
        COCOEval(DATASET, device="cpu").summarize_per_category()


def test_per_category_table():
    e = _hand_evaluator()
    t = compare.per_category_table({"base": e, "other": e}, metric_columns=(1, 3, 8))
    assert t["columns"] == ["AP50", "APs", "AR100"]
    ap0 = float(np.mean(np.repeat(np.linspace(1.0, 0.1, 10), 101)))
    assert t["base"] == {"AP50": [1.0, .5, -1.0], "APs": [ap0, -1.0, -1.0], "AR100": [.25, .375, -1.0]}       # the chosen columns, not stats[0..2]
    assert t["other"] == t["base"]
    assert compare.per_category_table({"base": e})["columns"] == ["AP"]
    import json
    json.dumps(t)
    with pytest.raises(ValueError):
        compare.per_category_table({"base": e}, metric_columns=(12,))


def test_box_disagreement_refuses_cpu_tensors():
    from object_detectors_amd import ops
    off = torch.zeros(2, dtype=torch.int64)
    side = (off, torch.zeros((0, 4), dtype=torch.float64), torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.box_disagreement(off, torch.zeros((0, 4), dtype=torch.float64), torch.zeros(0, dtype=torch.int64), side, side, 0.5)


def test_add_refuses_bad_arguments():
    d = compare.Disagreement(DATASET, device="cpu")
    box = torch.zeros((2, 4))
    for model in (2, -1, None, True, "0"):
        with pytest.raises(ValueError):
            d.add(model, 1, torch.tensor([3, 3]), torch.tensor([.5, .6]), box)
        with pytest.raises(ValueError):
            d.add_results(model, [])
    with pytest.raises(ValueError):
        d.add(0, 1, torch.tensor([3, 3]), torch.tensor([.5]), box)
    with pytest.raises(ValueError):
        d.add(1, 1, torch.tensor([3, 3]), torch.tensor([.5, .6]), box[:1])
    with pytest.raises(ValueError):
        d.add(1, torch.tensor([1, 2, 1]), torch.tensor([3, 3]), torch.tensor([.5, .6]), box)
    assert d.num_added == [0, 0]
    with pytest.raises(ValueError):
        compare.Disagreement(DATASET, device="cpu", max_dets=0)


def test_c_entry_refuses_bad_arguments():
    """MI355DET_EINVAL (-1) for a negative image count and for missing offset tables with images; both return before any launch."""
    import ctypes
    from object_detectors_amd import _lib
    L = _lib.lib()
    nul = ctypes.c_void_p(None)
    tail = (0.5, nul, nul, nul, nul)
    assert L.mi355det_box_disagreement(-1, nul, 0, nul, nul, nul, 0, nul, nul, nul, 0, nul, nul, *tail) == -1
    assert b"box_disagreement" in L.mi355det_last_error()
    assert L.mi355det_box_disagreement(3, nul, 0, nul, nul, nul, 0, nul, nul, nul, 0, nul, nul, *tail) == -1
    assert L.mi355det_box_disagreement(0, nul, 0, nul, nul, nul, 0, nul, nul, nul, 0, nul, nul, *tail) == 0          # no images: nothing to do
    assert L.mi355det_box_disagreement(0, nul, -1, nul, nul, nul, 0, nul, nul, nul, 0, nul, nul, *tail) == -1
