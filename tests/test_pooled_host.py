"""Host side of AP-fixed and AP-pool: what mi355det_pooled_accumulate refuses (before any launch, so null and host pointers do), the new
arguments of LVISEval / LVISSegmEval, and the default arguments leaving every key as it was.  CPU only."""
import ctypes as C

import pytest

DATASET = {"images": [{"id": 1, "neg_category_ids": [], "not_exhaustive_category_ids": [], "height": 8, "width": 8}],
           "categories": [{"id": 1, "frequency": "f"}], "annotations": []}


def _call(P=0, S=1, T=10, A=4, R=101, num_dt=0, offsets=(0, 0), operand=True, missing=None, ws_bytes=None):
    """Every pointer is one host buffer that is never dereferenced but the host copy of the offsets; `missing` names the operand passed as null."""
    from object_detectors_amd import _lib
    L = _lib.lib()
    buf = (C.c_int64 * 8)()
    p = C.cast(buf, C.c_void_p) if operand else None
    host = (C.c_int64 * len(offsets))(*offsets)
    need = int(L.mi355det_pooled_accumulate_workspace(max(P, 0), S, T, A))
    args = dict(pool_order=p, P=P, pool_offsets=p, host=C.cast(host, C.c_void_p), S=S, npig=p, num_dt=num_dt, dt_score=p, dt_match=p, dt_ignore=p, T=T,
                A=A, rec_thrs=p, R=R, precision=p, recall=p, scores=p, workspace=p, ws_bytes=need if ws_bytes is None else ws_bytes, stream=None)
    if missing:
        args[missing] = None
    return L.mi355det_pooled_accumulate(*args.values())


def _last_error():
    from object_detectors_amd import _lib
    return _lib.lib().mi355det_last_error().decode()


@pytest.mark.parametrize("kw, text", [
    (dict(P=-1), "negative"), (dict(num_dt=-1), "negative"),
    (dict(S=0, offsets=(0,)), "positive"), (dict(T=0), "positive"), (dict(A=0), "positive"), (dict(R=0), "positive"),
    (dict(T=10, A=7), "64"), (dict(T=65, A=1), "64"), (dict(R=4097), "4096"),
    (dict(missing="pool_offsets"), "missing"), (dict(missing="host"), "missing"), (dict(missing="npig"), "missing"),
    (dict(missing="rec_thrs"), "missing"), (dict(missing="precision"), "missing"), (dict(missing="recall"), "missing"),
    (dict(missing="scores"), "missing"), (dict(missing="workspace"), "missing"),
    (dict(P=5, offsets=(0, 5), missing="pool_order"), "missing"), (dict(P=5, offsets=(0, 5), num_dt=3, missing="dt_score"), "missing"),
    (dict(P=5, offsets=(0, 5), num_dt=3, missing="dt_match"), "missing"), (dict(P=5, offsets=(0, 5), num_dt=3, missing="dt_ignore"), "missing"),
    (dict(P=5, S=2, offsets=(0, 4, 3)), "non-decreasing"), (dict(P=5, offsets=(-1, 3)), "non-decreasing"), (dict(P=5, offsets=(0, 6)), "past"),
    (dict(P=5, offsets=(0, 5), ws_bytes=64), "workspace"), (dict(ws_bytes=0), "workspace"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_entry_refuses_before_any_launch(kw, text):
    assert _call(**kw) == -1                                       # MI355DET_EINVAL
    assert "pooled_accumulate" in _last_error() and text in _last_error()


def test_workspace_size_and_tile():
    from object_detectors_amd import _lib, ops
    L = _lib.lib()
    tile = ops.pooled_tile()
    assert tile == L.mi355det_pooled_tile() and tile >= 64 and tile % 64 == 0
    size = lambda P, S=4, T=10, A=4: int(L.mi355det_pooled_accumulate_workspace(P, S, T, A))
    assert size(0) > 0 and size(0) % 16 == 0
    assert size(10 * tile) - size(9 * tile) >= 16 * tile           # 16 bytes per position, and the tile tables
    assert size(-1) == 0 and size(5, S=0) == 0 and size(5, T=10, A=7) == 0


def test_op_refuses_cpu_tensors():
    import torch
    from object_detectors_amd import ops
    z = lambda dt, *shape: torch.zeros(shape, dtype=dt)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.pooled_accumulate(z(torch.int64, 0), z(torch.int64, 2), z(torch.int64, 1, 4), z(torch.float64, 0), z(torch.int32, 4, 10, 0),
                              z(torch.uint8, 4, 10, 0), z(torch.float64, 101))


@pytest.mark.parametrize("kw", [dict(max_dets=0), dict(max_dets=-2), dict(max_dets=300.0), dict(max_dets="300"), dict(max_dets=True),
                                dict(max_dets_per_cat=0), dict(max_dets_per_cat=-1), dict(max_dets_per_cat=10000.0), dict(max_dets_per_cat=False)],
                         ids=lambda kw: "-".join(f"{k}={v!r}" for k, v in kw.items()))
def test_evaluators_refuse_bad_cuts(kw):
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    with pytest.raises(ValueError, match="max_dets"):
        LVISEval(DATASET, **kw)
    with pytest.raises(ValueError, match="max_dets"):
        LVISSegmEval(DATASET, **kw)


def test_default_arguments_leave_the_keys():
    from object_detectors_amd import lviseval
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    keys = ("AP", "AP50", "AP75", "APs", "APm", "APl", "APr", "APc", "APf", "AR@300", "ARs@300", "ARm@300", "ARl@300")
    assert lviseval.RESULT_KEYS == keys and LVISEval.stat_names == keys
    for e in (LVISEval(DATASET), LVISSegmEval(DATASET), LVISEval(DATASET, None, "bbox", None, 300, None)):
        assert e.stat_names == keys and e.max_dets == 300 and e.max_dets_per_cat is None


def test_cut_arguments_name_the_keys():
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    for e in (LVISEval(DATASET, max_dets=None), LVISEval(DATASET, max_dets=-1), LVISSegmEval(DATASET, max_dets=None)):
        assert e.max_dets == -1 and e.stat_names[9:] == ("AR@-1", "ARs@-1", "ARm@-1", "ARl@-1") and e.stat_names[:9] == LVISEval.stat_names[:9]
    assert LVISEval(DATASET, max_dets=50).stat_names[9] == "AR@50"
    for e in (LVISEval.fixed(DATASET), LVISSegmEval.fixed(DATASET, iou_type="boundary")):
        assert e.max_dets == -1 and e.max_dets_per_cat == 10000 and e.stat_names[9] == "AR@-1"
    assert type(LVISSegmEval.fixed(DATASET)) is LVISSegmEval


def test_pooled_needs_evaluate_first():
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISEval
    for e in (LVISEval(DATASET), COCOEval(DATASET)):
        with pytest.raises(RuntimeError, match="evaluate"):
            e.accumulate_pooled()
        with pytest.raises(RuntimeError, match="accumulate_pooled"):
            e.summarize_pooled()
    assert [n for n, _c in LVISEval(DATASET).default_pools()] == ["", "r", "c", "f"] and [n for n, _c in COCOEval(DATASET).default_pools()] == [""]
