"""Host side of the polygon path (object_detectors_amd/polygons.py, ops.poly_rle, tvision/coco_utils.py): every refusal is a ValueError
raised before the library or the device is touched, dataset_to_rle passes non-polygon segmentations through, and the new entry points are
declared and bound.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SQUARE = [1, 1, 9, 1, 9, 9, 1, 9]
ENTRY_POINTS = ["mi355det_poly_points_count", "mi355det_poly_points_emit", "mi355det_poly_events", "mi355det_poly_runs_count",
                "mi355det_poly_runs_emit", "mi355det_rle_decode"]


@pytest.fixture()
def no_device(monkeypatch):
    """Any use of the library or of a device tensor fails the test with something that is not a ValueError."""
    from object_detectors_amd import _lib, ops

    def touched(*a, **k):
        raise AssertionError("the device was reached before the input was refused")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(ops, "lib", touched)
    monkeypatch.setattr(torch.Tensor, "to", touched)
    monkeypatch.setattr(torch.Tensor, "cuda", touched)


BAD_SEGMENTATIONS = [
    ("a 4-number box", [[1, 1, 5, 5]]),
    ("a flat 4-number box", [1, 1, 5, 5]),
    ("one point", [SQUARE, [1, 1]]),
    ("odd number of coordinates", [[1, 1, 9, 1, 9, 9, 1]]),
    ("nan", [[1, 1, 9, 1, float("nan"), 9]]),
    ("inf", [[1, 1, 9, 1, float("inf"), 9]]),
    ("too large", [[1, 1, 9, 1, 9, float(1 << 24)]]),
    ("too small", [[1, 1, 9, 1, 9, -float(1 << 24)]]),
    ("a string coordinate", [[1, 1, 9, 1, 9, "9"]]),
    ("a nested polygon", [[[1, 1], [9, 1], [9, 9]]]),
    ("run lengths", {"size": [12, 12], "counts": [144]}),
    ("an empty polygon", [[]]),
]


@pytest.mark.parametrize("name,seg", BAD_SEGMENTATIONS, ids=[b[0] for b in BAD_SEGMENTATIONS])
def test_bad_segmentations_are_refused_on_the_host(no_device, name, seg):
    from object_detectors_amd import polygons
    from object_detectors_amd.tvision import coco_utils
    with pytest.raises(ValueError):
        polygons.polygons_to_rle([SQUARE, seg], 12, 12)
    with pytest.raises(ValueError):
        polygons.segmentations_to_rle([seg], [(12, 12)])
    with pytest.raises(ValueError):
        coco_utils.convert_coco_poly_to_mask([seg], 12, 12)


@pytest.mark.parametrize("h,w", [(0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15), (2.5, 4), (True, 4)])
def test_bad_sizes_are_refused_on_the_host(no_device, h, w):
    from object_detectors_amd import polygons
    with pytest.raises(ValueError):
        polygons.polygons_to_rle([SQUARE], h, w)
    with pytest.raises(ValueError):
        polygons.segmentations_to_rle([SQUARE], [(h, w)])


def test_largest_coordinate_and_size_pass_the_host_checks():
    from object_detectors_amd import polygons
    big = float((1 << 24) - 1)
    xy, po, ao, sz = polygons.flatten([[[0, 0, big, 0, -big, big]], SQUARE, []], [(1 << 15, (1 << 16) - 1), (3, 3), (1, 1)])
    assert xy.dtype == np.float64 and xy.shape == (14,) and po.tolist() == [0, 3, 7] and ao.tolist() == [0, 1, 2, 2]
    assert sz.dtype == np.int32 and sz.tolist() == [[1 << 15, (1 << 16) - 1], [3, 3], [1, 1]]


def test_one_size_per_segmentation(no_device):
    from object_detectors_amd import polygons
    with pytest.raises(ValueError):
        polygons.segmentations_to_rle([SQUARE, SQUARE], [(12, 12)])


def _tables():
    return dict(xy=np.asarray(SQUARE + SQUARE[:6], np.float64), poly_offsets=[0, 4, 7], ann_offsets=[0, 1, 2], sizes=[[12, 12], [12, 12]])


@pytest.mark.parametrize("change", [
    dict(poly_offsets=[0, 5, 7]),                          # a polygon of 2 points
    dict(poly_offsets=[1, 4, 7]),
    dict(poly_offsets=[0, 4, 8]),                          # more points than xy holds
    dict(ann_offsets=[0, 2, 1]),
    dict(ann_offsets=[0, 1, 3]),
    dict(ann_offsets=[0, 1]),                              # a polygon without an annotation
    dict(sizes=[[12, 12]]),
    dict(sizes=[[12, 12], [0, 12]]),
    dict(sizes=[[12, 12], [1 << 16, 1 << 15]]),
    dict(xy=np.asarray(SQUARE + [1, 1, float("nan"), 1, 9, 9], np.float64)),
    dict(xy=np.asarray(SQUARE + [1, 1, float(1 << 24), 1, 9, 9], np.float64)),
])
def test_ops_poly_rle_refuses_bad_tables_on_the_host(no_device, change):
    from object_detectors_amd import ops
    with pytest.raises(ValueError):
        ops.poly_rle(**{**_tables(), **change})


def test_mask_rle_decode_refuses_host_counts(no_device):
    from object_detectors_amd import ops
    with pytest.raises(ValueError):
        ops.mask_rle_decode(torch.tensor([144], dtype=torch.int32), [0, 1], (12, 12))
    with pytest.raises(ValueError):
        ops.mask_rle_decode(torch.tensor([144], dtype=torch.int32))


def test_dataset_to_rle_passes_other_segmentations_through(no_device):
    """Run lengths (count list or string), bitmaps and annotations without a segmentation stay the same objects; without a polygon nothing
    is converted, so nothing reaches the device."""
    from object_detectors_amd import polygons
    bitmap = np.zeros((4, 6), np.uint8)
    anns = [{"id": 1, "image_id": 7, "category_id": 1, "segmentation": {"size": [4, 6], "counts": [3, 2, 19]}},
            {"id": 2, "image_id": 7, "category_id": 1, "segmentation": {"size": [4, 6], "counts": "32c0"}},
            {"id": 3, "image_id": 7, "category_id": 1, "segmentation": bitmap},
            {"id": 4, "image_id": 7, "category_id": 1, "bbox": [0, 0, 2, 2]}]
    ds = {"images": [{"id": 7, "height": 4, "width": 6}], "categories": [{"id": 1}], "annotations": anns, "info": {"year": 2017}}
    out = polygons.dataset_to_rle(ds)
    assert out is not ds and out["annotations"] is not anns and set(out) == set(ds)
    assert out["images"] is ds["images"] and out["categories"] is ds["categories"] and out["info"] is ds["info"]
    assert len(out["annotations"]) == 4 and all(a is b for a, b in zip(out["annotations"], anns))
    assert out["annotations"][2]["segmentation"] is bitmap


def test_dataset_to_rle_refuses_on_the_host(no_device):
    from object_detectors_amd import polygons
    ds = {"images": [{"id": 7, "height": 12, "width": 12}], "categories": [{"id": 1}],
          "annotations": [{"id": 1, "image_id": 8, "category_id": 1, "segmentation": [SQUARE]}]}
    with pytest.raises(ValueError):
        polygons.dataset_to_rle(ds)                        # the annotation's image is missing
    ds["annotations"][0].update(image_id=7, segmentation=[[1, 1, 5, 5]])
    with pytest.raises(ValueError):
        polygons.dataset_to_rle(ds)                        # a 4-number box
    with pytest.raises(ValueError):
        polygons.dataset_to_rle([1, 2])


def test_is_polygon_segmentation():
    from object_detectors_amd.polygons import is_polygon_segmentation as isp
    assert isp([]) and isp([SQUARE]) and isp(SQUARE) and isp(((1.5, 2, 3, 4, 5, 6),))
    assert not isp({"size": [1, 1], "counts": [1]}) and not isp(np.zeros((2, 2))) and not isp(None) and not isp("abc")


def test_entry_points_are_declared_and_bound():
    from object_detectors_amd import _lib, build
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355det.h")).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.PROTOTYPES, name
    assert any(src == "poly_kernels.hip" and "-ffp-contract=off" in flags for src, flags in build.SOURCES)
    L = _lib.lib()
    for name in ENTRY_POINTS:
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """Status -1 (MI355DET_EINVAL) from the argument checks, which run before any HIP call."""
    from object_detectors_amd import _lib
    L = _lib.lib()
    assert L.mi355det_poly_points_count(None, None, None, None, -1, 0, None, None) == -1
    assert L.mi355det_poly_points_count(None, None, None, None, 1, 0, None, None) == -1
    assert L.mi355det_poly_points_emit(None, None, None, None, 0, 0, None, 5, None, 4, None) == -1
    assert L.mi355det_poly_runs_emit(None, None, None, None, None, None, 0, -1, None, 0, None, 0, None, None, None) == -1
    assert L.mi355det_rle_decode(None, None, 1, 0, 4, None, None) == -1
    assert L.mi355det_rle_decode(None, None, 1, 1 << 16, 1 << 15, None, None) == -1
    assert L.mi355det_rle_decode(None, None, 1, 4, 4, None, None) == -1
    assert b"rle_decode" in L.mi355det_last_error()
    assert L.mi355det_rle_decode(None, None, 0, 4, 4, None, None) == 0
    assert L.mi355det_poly_points_count(None, None, None, None, 0, 0, None, None) == 0
    # what the emit pass says of the numbers read back from the count pass, word for word; refused calls touch no pointer
    fake = C.c_void_p(4096)
    emit = lambda total=5, counts=fake, cap=5: \
        L.mi355det_poly_runs_emit(fake, fake, fake, fake, fake, fake, 2, 3, fake, total, counts, cap, None, None, None)
    for kw, text in ((dict(cap=4), "poly_runs_emit: capacity 4 is smaller than the 5 counts"),
                     (dict(total=2), "poly_runs_emit: total_runs 2 is below one count per annotation"),
                     (dict(counts=None), "poly_runs_emit: missing operand")):
        assert emit(**kw) == -1, kw
        assert L.mi355det_last_error().decode() == text


def test_shims_register_coco_utils():
    from object_detectors_amd import shims
    assert "coco_utils" in shims._TVISION
    from object_detectors_amd.tvision import coco_utils
    assert callable(coco_utils.convert_coco_poly_to_mask) and callable(coco_utils.ConvertCocoPolysToMask())
