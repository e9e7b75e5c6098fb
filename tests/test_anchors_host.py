"""The host side of object_detectors_amd/anchors.py: list handling, anchor layouts, and every refusal that needs no device.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from object_detectors_amd import anchors as A  # noqa: E402
from tests.test_oracle_kmeans import dataset  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "anchors_lvis.json")


def test_extend_anchors_reproduces_the_recorded_lvis_list():
    """The reference's lvis.yaml = its three found centres per scale in front of the stock three."""
    rec = json.load(open(GOLDEN))
    assert rec["stock"] == A.STOCK_ANCHORS
    found = [scale[:3] for scale in rec["lvis"]]
    assert A.extend_anchors(rec["stock"], found) == rec["lvis"]
    assert [len(s) for s in A.extend_anchors(rec["stock"], found)] == [6, 6, 6]
    with pytest.raises(ValueError):
        A.extend_anchors(rec["stock"], found[:2])
    # the first recorded pair is width * 416, height * 416 of a centre of the large band: area > 0.1
    w, h = rec["lvis"][0][0]
    assert (w / 416) * (h / 416) > 0.1 and (rec["lvis"][2][0][0] / 416) * (rec["lvis"][2][0][1] / 416) < 0.01


def test_split_anchors_orders_by_descending_area_and_splits_evenly():
    c = [[0.1, 0.1], [0.5, 0.5], [0.2, 0.1], [0.9, 0.8], [0.05, 0.05], [0.1, 0.2]]       # areas .01 .25 .02 .72 .0025 .02: a tie keeps its order
    got = A.split_anchors(c, 100, 3)
    assert got == [[[90.0, 80.0], [50.0, 50.0]], [[20.0, 10.0], [10.0, 20.0]], [[10.0, 10.0], [5.0, 5.0]]]
    assert A.split_anchors(c, 100, 1) == [got[0] + got[1] + got[2]]
    with pytest.raises(ValueError):
        A.split_anchors(c[:5], 100, 3)
    with pytest.raises(ValueError):
        A.iou_anchors({"features": None}, "coco", 416, k=8, scales=3)
    with pytest.raises(ValueError):
        A.iou_anchors({"features": None}, "coco", 416, k=9, metric="euclid")
    with pytest.raises(ValueError):
        A.reference_anchors({"features": None}, "coco", 416, metric="iou")


def test_box_arrays_walks_the_images():
    a = A.box_arrays(dataset(), "coco")
    assert a["n_images"] == 2 and a["image_size"].tolist() == [[10, 10], [100, 200]]          # sorted ids: 3, 7
    assert a["box_wh"].shape == (10, 2) and a["box_wh"].dtype == np.float64 and a["image_index"].dtype == np.int32
    assert a["image_index"].tolist() == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1]                      # the annotation of image 99 is gone
    assert a["box_wh"][4].tolist() == [12.5, 16.0]
    with pytest.raises(ValueError):
        A.box_arrays({"images": [{"id": 1, "width": 4, "height": 4}], "annotations": [{"image_id": 2, "bbox": [0, 0, 1, 1]}]})
    with pytest.raises(ValueError):
        A.box_arrays(dataset(), "voc")


def test_dataset_arrays_is_unchanged_by_the_shared_walk():
    from object_detectors_amd import dataset_stats
    d = dataset()
    d["categories"] = [{"id": 1, "name": "a"}]
    a = dataset_stats.dataset_arrays(d, "coco")
    assert a["image_index"].tolist() == [1, 0, 1, 1, 1, 1, 1, 1, 1, 1] and a["category_index"].tolist() == [1] * 10
    assert a["n_images"] == 2 and a["n_categories"] == 2
    d["images"] = []
    with pytest.raises(ValueError):
        dataset_stats.dataset_arrays(d, "coco")


def test_seeded_rows_draws_problem_major_from_one_generator():
    rows = A.seeded_rows([5, 7], 2, 3, seed=5)
    g = torch.Generator().manual_seed(5)
    want = torch.stack([torch.stack([torch.randperm(n, generator=g)[:2] for _ in range(3)]) for n in (5, 7)])
    assert torch.equal(rows, want) and tuple(rows.shape) == (2, 3, 2)


def test_refusals_that_need_no_device():
    X = torch.rand(20, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        A.kmeans(X, 3)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        A.assign(X, X[:3])
    with pytest.raises(ValueError, match="CUDA/HIP"):
        A.fitness(X, A.STOCK_ANCHORS)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        A.box_features(A.box_arrays(dataset()), device="cpu")


class FakeDevice(torch.Tensor):
    """A CPU tensor that says it lives on the device: reaches the refusals behind the device check without one."""

    @property
    def is_cuda(self):
        return True


def fake(t):
    return t.as_subclass(FakeDevice)


def test_refusals_behind_the_device_check():
    X = fake(torch.rand(20, 2, dtype=torch.float64))
    with pytest.raises(ValueError, match="float64"):
        A.kmeans(fake(torch.rand(20, 2)), 3)
    with pytest.raises(ValueError, match="float64"):
        A.kmeans(fake(torch.rand(20, dtype=torch.float64)), 3)
    with pytest.raises(ValueError, match="features"):
        A.kmeans(fake(torch.rand(20, 5, dtype=torch.float64)), 3)
    with pytest.raises(ValueError, match="no points"):
        A.kmeans(fake(torch.rand(0, 2, dtype=torch.float64)), 3)
    with pytest.raises(ValueError, match="F = 2"):
        A.kmeans(fake(torch.rand(20, 4, dtype=torch.float64)), 3, metric="iou")
    with pytest.raises(ValueError, match="metric"):
        A.kmeans(X, 3, metric="cosine")
    for k in (0, -1, A.MAX_K + 1):
        with pytest.raises(ValueError, match="k <="):
            A.kmeans(X, k)
    with pytest.raises(ValueError, match="n_init"):
        A.kmeans(X, 3, n_init=A.MAX_RESTARTS + 1)
    with pytest.raises(ValueError, match="n_init"):
        A.kmeans(X, 3, n_init=0)
    with pytest.raises(ValueError, match="problems"):
        A.kmeans(X, 3, problem=fake(torch.zeros(20, dtype=torch.int8)), n_problems=A.MAX_PROBLEMS + 1)
    with pytest.raises(ValueError, match="problem index per point"):
        A.kmeans(X, 3, n_problems=2)
    with pytest.raises(ValueError, match="problem index per point"):
        A.kmeans(X, 3, problem=fake(torch.zeros(19, dtype=torch.int8)), n_problems=2)
    with pytest.raises(ValueError, match="positive"):
        A.kmeans(X, 3, max_iter=0)
    for shape in ((1, 2, 3, 3), (2, 2, 3, 2), (1, 2, 4, 2), (2, 3, 2), (1, A.MAX_RESTARTS + 1, 3, 2)):
        with pytest.raises(ValueError, match="init"):
            A.kmeans(X, 3, init=torch.zeros(shape, dtype=torch.float64))
    with pytest.raises(ValueError, match="init"):
        A.kmeans(X, 3, init=torch.zeros((1, 2, 3, 2), dtype=torch.float32))
    with pytest.raises(ValueError, match="centres"):
        A.assign(X, fake(torch.zeros(A.MAX_ASSIGN_K + 1, 2, dtype=torch.float64)))
    with pytest.raises(ValueError, match="centres"):
        A.assign(X, fake(torch.zeros(3, 4, dtype=torch.float64)))
    with pytest.raises(ValueError, match="anchors"):
        A.fitness(X, np.ones((A.MAX_ASSIGN_K + 1, 2)))
    with pytest.raises(ValueError, match="positive"):
        A.fitness(X, [[[1, 2], [0, 3]]])


def test_the_restated_limits_are_the_library_s():
    """The limits the host refuses by are the ones the LDS layout of csrc/kmeans_kernels.hip was sized for, and admit the issue's
    P = 3, R = 16, k = 16, F = 4 together."""
    from object_detectors_amd import build
    build.build()
    lim = A.limits()
    assert (lim["problems"], lim["restarts"], lim["k"], lim["features"], lim["assign_k"]) == (A.MAX_PROBLEMS, A.MAX_RESTARTS, A.MAX_K,
                                                                                             A.MAX_FEATURES, A.MAX_ASSIGN_K)
    assert lim["problems"] >= 3 and lim["restarts"] >= 16 and lim["k"] >= 16 and lim["features"] >= 4
    from object_detectors_amd import _lib
    L = _lib.lib()
    B = lim["points_per_workgroup"]
    assert L.mi355det_kmeans_workspace(B + 1, 3, 16, 16, 4) == 3 * 16 * (16 * 4 + 1) * 2 * 8 +(16 * (B + 1) + 7) // 8 * 8 + (3 * 16 * 16 + 2 * 48) * 4
    for bad in ((0, 1, 1, 1, 1), (10, 5, 1, 1, 1), (10, 1, 17, 1, 1), (10, 1, 1, 17, 1), (10, 1, 1, 1, 5), (2 ** 31, 1, 1, 1, 1)):
        assert L.mi355det_kmeans_workspace(*bad) == 0
    # the C entries refuse null pointers and exceeded limits through mi355det_last_error, before any launch
    assert L.mi355det_kmeans_passes(None, None, 10, 1, 1, 1, 2, 0, 300, 1, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"missing operand" in L.mi355det_last_error()
    assert L.mi355det_kmeans_passes(None, None, 10, 1, 1, 17, 2, 0, 300, 1, None, None, None, None, None, None, None, None, 0, None) == -1
    assert b"limits" in L.mi355det_last_error()
    assert L.mi355det_kmeans_assign(None, None, 10, 1, 3, 4, 1, None, None, None, None) == -1            # iou with F = 4
    assert L.mi355det_box_features(None, None, None, 10, 1, None, None, None, None) == -1
    assert L.mi355det_kmeans_check(None, None, 10, 1, 2, 0, None, None) == -1
    assert L.mi355det_kmeans_begin(10, 1, 1, 1, 2, None, None, None, 0, None) == -1


def test_make_anchors_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_anchors.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--extend-defaults" in r.stdout and "--inp-dim" in r.stdout
