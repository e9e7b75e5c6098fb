"""Host side of the error breakdown (object_detectors_amd/tide.py): what ErrorBreakdown refuses, the report text on a hand-made result and
the argument checks of the two C entries.  CPU only: nothing here launches a kernel."""
import ctypes
import io

import numpy as np
import pytest
import torch

from object_detectors_amd import tide
from object_detectors_amd.cocoeval import COCOEval

DATASET = {"images": [{"id": 1}, {"id": 2}], "categories": [{"id": 3}, {"id": 5}],
           "annotations": [{"id": 1, "image_id": 1, "category_id": 3, "bbox": [0., 0., 4., 4.], "area": 16., "iscrowd": 0}]}


def test_refuses_an_evaluator_that_was_not_evaluated():
    with pytest.raises(RuntimeError):
        tide.ErrorBreakdown(COCOEval(DATASET, device="cpu"))


def test_refuses_segm():
    with pytest.raises(NotImplementedError):
        tide.ErrorBreakdown(COCOEval(DATASET, "segm", device="cpu"))


def test_refuses_a_threshold_the_evaluator_did_not_use():
    ev = COCOEval(DATASET, device="cpu")
    ev.iou = torch.zeros(0, dtype=torch.float64)                  # stands for evaluate(): the threshold is looked up before anything is read
    b = tide.ErrorBreakdown(ev)
    for fg in (0.525, 0.3, 1.0):
        with pytest.raises(ValueError):
            b.run(fg=fg)
    with pytest.raises(RuntimeError):
        b.report()


def test_ops_refuse_cpu_tensors():
    from object_detectors_amd import ops
    i64 = torch.zeros(1, dtype=torch.int64)
    view = (i64, i64[:0], i64, i64[:0])
    none = lambda dt, *shape: torch.zeros((0,) + shape, dtype=dt)
    with pytest.raises(ValueError):
        ops.tide_classify(view, none(torch.float64, 4), none(torch.int32), none(torch.uint8), none(torch.float64, 4), none(torch.int32),
                          none(torch.uint8), none(torch.uint8))
    with pytest.raises(ValueError):
        ops.tide_fixes(view, none(torch.int32), none(torch.uint8), none(torch.int32), none(torch.int32), none(torch.uint8), none(torch.uint8),
                       none(torch.uint8), none(torch.int64), none(torch.uint8))


def test_report_text():
    ev = COCOEval(DATASET, device="cpu")
    ev.iou = torch.zeros(0, dtype=torch.float64)
    b = tide.ErrorBreakdown(ev)
    dap = np.asarray([.125, .0625, 0., .03125, .25, np.nan, .5, .375])
    b.result = {"fg": .5, "bg": .1, "ap_base": .4375, "counts": np.asarray([3, 2, 0, 1, 7, 4, 13], np.int64), "dap": dap,
                "dap_per_category": np.stack([dap, dap * 2])}
    out = io.StringIO()
    b.report(file=out, per_category=True)
    lines = out.getvalue().splitlines()
    assert lines[0] == "Error breakdown at IoU 0.50 (background below 0.10): AP50 = 43.75"
    assert lines[2].split() == ["Cls", "3", "12.50"] and lines[7].split() == ["Miss", "4", "nan"]
    assert lines[8].split() == ["FP", "13", "50.00"] and lines[9].split() == ["FN", "37.50"]
    assert "do not add up" in lines[10]
    assert lines[11].split() == ["category"] + list(tide.FIXES) and lines[13].split()[:3] == ["5", "25.00", "12.50"]


NUL = ctypes.c_void_p(None)
PTR = ctypes.c_void_p(64)                                         # never dereferenced: every call below returns before a launch


def _classify(L, images, nd, ng, fg=.5, bg=.1, view=PTR, operand=PTR):
    return L.mi355det_tide_classify(images, view, view, nd, view, view, ng, *([operand] * 7), fg, bg, *([operand] * 5), NUL)


def _fixes(L, images, nd, ng, view=PTR, operand=PTR):
    return L.mi355det_tide_fixes(images, view, view, nd, view, view, ng, *([operand] * 15), NUL)


def test_c_entries_refuse_bad_arguments():
    """MI355DET_EINVAL (-1) for negative sizes, missing operands and bad thresholds; no images, or no slots at all, is nothing to do (0).
    All of it returns before any launch."""
    from object_detectors_amd import _lib
    L = _lib.lib()
    for call, name in ((_classify, b"tide_classify"), (_fixes, b"tide_fixes")):
        for sizes in ((-1, 0, 0), (2, -1, 0), (2, 0, -1)):
            assert call(L, *sizes) == -1
            assert name in L.mi355det_last_error()
        assert call(L, 3, 5, 5, view=NUL) == -1                    # images, but no view of them
        assert call(L, 3, 5, 0, operand=NUL) == -1                 # detections without their arrays
        assert call(L, 3, 0, 5, operand=NUL) == -1                 # ground truths without theirs
        assert call(L, 0, 5, 5, view=NUL, operand=NUL) == 0        # no images: nothing to do
        assert call(L, 3, 0, 0, view=NUL, operand=NUL) == 0        # no slots at all
    for fg, bg in ((.5, .5), (.1, .5), (.5, 0.), (.5, -.1), (1.5, .1), (0., 0.), (float("nan"), .1), (.5, float("nan"))):
        assert _classify(L, 0, 0, 0, fg=fg, bg=bg) == -1, (fg, bg)
        assert b"threshold" in L.mi355det_last_error()
    assert _classify(L, 0, 0, 0, fg=1.0, bg=.1) == 0               # (0, 1] includes 1
