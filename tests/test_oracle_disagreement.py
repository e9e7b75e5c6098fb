"""Hand-checked cases that pin tests/disagreement_oracle.py, the literal form of the reference's notebooks/get_disagreement.py that the device
comparison is measured against (tests/test_gpu_compare.py).  CPU only."""
import pytest
import torch

from tests import disagreement_cases as dc
from tests import disagreement_oracle as do

CASES = dc.hand_cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_case(case):
    _name, dataset, res0, res1, thr, conf, want = case
    got = do.disagreement(dataset, res0, res1, thr, conf)
    assert {k: got[k] for k in dc.COUNT_KEYS} == want


def test_box_iou_by_hand():
    a = torch.tensor([[0., 0., 10., 10.], [5., 5., 5., 5.]], dtype=torch.float64)        # [x1, y1, x2, y2]; the second has no area
    b = torch.tensor([[0., 0., 10., 5.], [20., 20., 30., 30.], [80., 80., 80., 80.]], dtype=torch.float64)
    iou = do.box_iou(a, b)
    assert iou[0, 0] == 0.5 and iou[0, 1] == 0.0 and iou[0, 2] == 0.0 and iou[1, 0] == 0.0
    assert torch.isnan(iou[1, 2])                  # two zero areas apart from each other: 0 / 0
    # the area is (x2 - x1) * (y2 - y1) of the corner form, which is not always w * h
    x, w = 0.1, 0.2
    assert (x + w) - x != w


def test_tie_takes_the_lower_index():
    _name, dataset, res0, res1, thr, conf, _want = CASES[1]
    (right0, iou0, idx0), (right1, iou1, idx1) = do.disagreement(dataset, res0, res1, thr, conf)["images"][7]
    assert iou0.tolist() == [1.0] and iou1.tolist() == [1.0] and idx0.tolist() == [0] and idx1.tolist() == [0]
    assert right0 == [] and right1 == [0]


def test_nan_beats_every_number():
    _name, dataset, res0, res1, thr, conf, _want = CASES[2]
    (right0, iou0, idx0), (right1, iou1, idx1) = do.disagreement(dataset, res0, res1, thr, conf)["images"][7]
    assert torch.isnan(iou0[0]) and idx0.tolist() == [1, 0] and right0 == [1]          # the point: NaN from detection 1, so it is wrong
    assert iou1.tolist() == [0.0, 1.0] and right1 == [0, 1]                             # without that detection 0 >= 0 is enough
    # torch.max along dim 0: NaN wins, and among equals or among NaNs the first
    nan = float("nan")
    m = torch.tensor([[.5, nan, .2], [.5, .3, nan], [.1, nan, .9]], dtype=torch.float64).max(dim=0)
    assert m.indices.tolist() == [0, 0, 1]


def test_empty_sides_raise_index_error():
    gt = torch.tensor(do.convert_gt_to_numpy([{"bbox": [0., 0., 4., 4.], "category_id": 1}]))
    with pytest.raises(IndexError):
        do.convert_dt_to_numpy([])
    with pytest.raises(IndexError):
        do.convert_gt_to_numpy([])
    with pytest.raises(IndexError):
        do.best_match(torch.zeros((0, 6), dtype=torch.float64), gt)                     # every detection filtered by the confidence
