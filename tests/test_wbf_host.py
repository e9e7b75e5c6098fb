"""Weighted boxes fusion without a launch: what the front end (object_detectors_amd/ensemble.py), ops.wbf_fuse and the C entry point
mi355det_wbf_fuse refuse, and the empty result.  CPU only."""
import ctypes

import pytest
import torch

IMAGES = [1, 2, 3]


def _wbf(**kw):
    from object_detectors_amd.ensemble import WeightedBoxesFusion
    return WeightedBoxesFusion(IMAGES, device="cpu", **kw)


@pytest.mark.parametrize("weights", [(1, 0), (1, -2), (float("inf"), 1), (float("nan"),), ()])
def test_weights_must_be_positive(weights):
    with pytest.raises(ValueError, match="weight"):
        _wbf(weights=weights)


def test_one_weight_per_model():
    from object_detectors_amd.ensemble import fuse_results
    with pytest.raises(ValueError, match="one weight per model"):
        fuse_results([[], [], []], IMAGES, weights=(1, 1), device="cpu")
    with pytest.raises(ValueError, match="one weight per model"):
        _wbf(weights=(1, 1)).add_results(2, [])


@pytest.mark.parametrize("thr", [-.01, 1.0, 1.5, float("nan")])
def test_iou_thr_range(thr):
    with pytest.raises(ValueError, match="iou_thr"):
        _wbf(iou_thr=thr)


@pytest.mark.parametrize("conf_type", ["box_and_model_avg", "absent_model_aware_avg", "AVG", None])
def test_unknown_conf_type(conf_type):
    with pytest.raises(ValueError, match="conf_type"):
        _wbf(conf_type=conf_type)


@pytest.mark.parametrize("model", [-1, 2, 1.0, True, None])
def test_model_index_out_of_range(model):
    f = _wbf(weights=(1, 1))
    with pytest.raises(ValueError, match="model"):
        f.add_results(model, [])
    with pytest.raises(ValueError, match="model"):
        f.add(model, 1, [1], [.5], [[0, 0, 1, 1]])


def test_models_are_counted_without_weights():
    f = _wbf()
    assert f.num_models == 1 and f.weights == [1.0]
    f.add_results(2, [])
    assert f.num_models == 3 and f.weights == [1.0, 1.0, 1.0] and f.weight_sum == 3.0 and f.weight_max == 1.0
    assert _wbf(weights=(2, 1, .5)).weight_sum == 3.5


def test_images_from_a_ground_truth():
    from object_detectors_amd.ensemble import WeightedBoxesFusion
    gt = {"images": [{"id": 7}, {"id": 3}], "categories": [{"id": 1}], "annotations": []}
    assert WeightedBoxesFusion(gt, device="cpu").img_ids == [3, 7]
    assert WeightedBoxesFusion(torch.tensor([5, 2, 5]), device="cpu").img_ids == [2, 5]
    with pytest.raises(ValueError):
        WeightedBoxesFusion({"no": "images"}, device="cpu")


def test_run_before_anything_is_added():
    from object_detectors_amd.ensemble import DROP_REASONS
    f = _wbf(weights=(1, 1))
    f.add_results(0, [])
    r = f.run()
    for key, dtype in (("image_index", torch.int64), ("image_id", torch.int64), ("category_id", torch.int64), ("score", torch.float64),
                       ("members", torch.int32), ("cluster_of", torch.int64)):
        assert r[key].dtype == dtype and tuple(r[key].shape) == (0,)
    assert r["box"].dtype == torch.float64 and tuple(r["box"].shape) == (0, 4)
    assert r["dropped"] == dict.fromkeys(DROP_REASONS, 0) and len(DROP_REASONS) == 5
    assert f.to_results() == []


def test_op_refuses_cpu_tensors():
    from object_detectors_amd import ops
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.wbf_fuse(torch.zeros(2, dtype=torch.int64), torch.zeros(1, 4, dtype=torch.float64), torch.ones(1, dtype=torch.float64))


# ---- the C entry point: every refusal comes before any launch, so null device pointers do
def _call(num_groups=0, num_boxes=0, iou_thr=.55, conf_type=0, weight_sum=1.0, weight_max=1.0, operand=None):
    from object_detectors_amd import _lib
    p = ctypes.c_void_p(operand)
    return _lib.lib().mi355det_wbf_fuse(p, num_groups, num_boxes, p, p, iou_thr, conf_type, weight_sum, weight_max, p, p, p, p, p, p, None)


def test_entry_accepts_nothing_to_do():
    assert _call() == 0
    assert _call(conf_type=1, iou_thr=0.0, weight_sum=3.5, weight_max=2.0) == 0


@pytest.mark.parametrize("kw", [dict(num_groups=-1), dict(num_boxes=-1), dict(iou_thr=-.01), dict(iou_thr=1.0), dict(iou_thr=float("nan")),
                                dict(conf_type=2), dict(conf_type=-1), dict(weight_sum=0.0), dict(weight_sum=float("inf")),
                                dict(weight_sum=float("nan")), dict(weight_max=0.0), dict(weight_max=-1.0), dict(weight_max=float("inf")),
                                dict(num_groups=1, num_boxes=1), dict(num_groups=1)], ids=lambda kw: "-".join(f"{k}={v}" for k, v in kw.items()))
def test_entry_refuses(kw):
    from object_detectors_amd import _lib
    assert _call(**kw) == -1                                        # MI355DET_EINVAL
    assert b"wbf_fuse" in _lib.lib().mi355det_last_error()


def test_lds_cluster_count_is_exported():
    from object_detectors_amd import ops
    n = ops.wbf_lds_clusters()
    assert 64 < n and n * 40 <= 64 * 1024 // 2                      # past one lane stride; two workgroups' worth stays under 64 KB
