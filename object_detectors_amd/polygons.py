"""COCO / LVIS polygon ground truth as run lengths, made on the device (csrc/poly_kernels.hip through `ops.poly_rle`).

A `segmentation` of a COCO annotation is a list of polygons `[[x0, y0, x1, y1, ...], ...]`; its mask is the union of the polygons' masks,
each rasterised by the rule of pycocotools `rleFrPoly` (include/mi355det.h, "Polygon ground truth as COCO run-length encodings").  What
pycocotools spells `merge(frPyObjects(segmentation, h, w))`, and torchvision_models/detection/coco_utils.py:33-47 `decode(...).any(dim=2)`.

    polygons_to_rle(segmentations, h, w)         one image: an RLEBatch, one mask per annotation
    segmentations_to_rle(segmentations, sizes)   annotations of images of different sizes in one call
    dataset_to_rle(dataset)                      a dataset dict whose polygon segmentations are replaced by {"size", "counts"}

    COCOEval(dataset_to_rle(json.load(open("instances_val2017.json"))), "segm")

Accepted input: a list of polygons or one flat polygon; each polygon an even number of coordinates, at least 6; every coordinate finite with
|c| < 2^24; h, w >= 1 and h*w < 2^31.  Anything else is a ValueError raised on the host before any launch.  An empty list is the all-zero
mask.  Deviation from pycocotools: frPyObjects reads a flat list of 4 numbers as a box [x, y, w, h]; here it is refused like any other
polygon of fewer than 3 points."""
from collections import namedtuple

import numpy as np

from .rle import RLEBatch

MAX_COORD = float(1 << 24)

PolygonRLE = namedtuple("PolygonRLE", "counts offsets area bbox sizes")
PolygonRLE.__doc__ = """The run lengths of n annotations in the concatenated form of RLEBatch: counts int32, area int64 [n] and bbox int32
[n, 4] on the device, offsets a host list [n + 1], sizes int32 [n, 2] = [h, w] on the host."""


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


def is_polygon_segmentation(seg):
    """A list of polygons or one flat polygon (also the empty list), as opposed to run lengths (a dict) or a bitmap (an array)."""
    return isinstance(seg, (list, tuple)) and (len(seg) == 0 or isinstance(seg[0], (list, tuple)) or _is_number(seg[0]))


def _parts(seg, where):
    """One segmentation -> its polygons as flat float64 arrays, validated."""
    if not isinstance(seg, (list, tuple)):
        raise ValueError(f"{where}: a segmentation must be a list of polygons or one flat polygon, not {type(seg).__name__}")
    polys = [seg] if len(seg) and _is_number(seg[0]) else list(seg)
    out = []
    for poly in polys:
        arr = np.asarray(poly) if isinstance(poly, (list, tuple, np.ndarray)) else None
        if arr is None or arr.ndim != 1 or (arr.size and arr.dtype.kind not in "iuf"):     # strings, booleans, nested lists, None
            raise ValueError(f"{where}: a polygon must be a flat list of numbers")
        if arr.size % 2 or arr.size < 6:
            raise ValueError(f"{where}: a polygon needs an even number of coordinates, at least 6 (got {arr.size}; a 4-number box is not "
                             "a polygon here)")
        arr = arr.astype(np.float64)
        if not (np.isfinite(arr) & (np.abs(arr) < MAX_COORD)).all():
            raise ValueError(f"{where}: every coordinate must be finite with |c| < 2^24")
        out.append(arr)
    return out


def _size(h, w, where):
    if isinstance(h, bool) or isinstance(w, bool) or not isinstance(h, (int, np.integer)) or not isinstance(w, (int, np.integer)):
        raise ValueError(f"{where}: height and width must be integers")
    if h < 1 or w < 1 or int(h) * int(w) >= (1 << 31):
        raise ValueError(f"{where}: needs h, w >= 1 and h*w < 2^31 (got {h} x {w})")
    return int(h), int(w)


def flatten(segmentations, sizes, where="segmentations_to_rle"):
    """Validated host tables of `ops.poly_rle`: xy float64 [2 * points], poly_offsets [NP + 1] in points, ann_offsets [A + 1] in polygons,
    sizes int32 [A, 2]."""
    segmentations = list(segmentations)
    sizes = [_size(s[0], s[1], where) for s in sizes]
    if len(sizes) != len(segmentations):
        raise ValueError(f"{where}: one size per segmentation")
    xy, poly_offsets, ann_offsets = [], [0], [0]
    for j, seg in enumerate(segmentations):
        for poly in _parts(seg, f"{where}: segmentation {j}"):
            xy.append(poly)
            poly_offsets.append(poly_offsets[-1] + poly.shape[0] // 2)
        ann_offsets.append(len(poly_offsets) - 1)
    return (np.concatenate(xy) if xy else np.zeros(0, np.float64), np.asarray(poly_offsets, np.int64), np.asarray(ann_offsets, np.int64),
            np.asarray(sizes, np.int32).reshape(-1, 2))


def segmentations_to_rle(segmentations, sizes, device=None):
    """Polygon segmentations of images of different sizes -> PolygonRLE, in one conversion.  sizes: one (h, w) per segmentation."""
    from . import ops
    xy, po, ao, sz = flatten(segmentations, sizes)
    counts, offsets, area, bbox = ops.poly_rle(xy, po, ao, sz, device=device)
    return PolygonRLE(counts, offsets, area, bbox, sz)


def polygons_to_rle(segmentations, height, width, device=None):
    """The polygon segmentations of one image's annotations -> RLEBatch, one mask per annotation (every field on the device)."""
    from . import ops
    segmentations = list(segmentations)
    h, w = _size(height, width, "polygons_to_rle")
    xy, po, ao, sz = flatten(segmentations, [(h, w)] * len(segmentations), "polygons_to_rle")
    counts, offsets, area, bbox = ops.poly_rle(xy, po, ao, sz, device=device)
    return RLEBatch((h, w), counts, offsets, area, bbox)


def dataset_to_rle(dataset, device=None):
    """A shallow copy of a COCO / LVIS dataset dict in which every polygon `segmentation` is replaced by {"size": [h, w], "counts": [...]}
    (h, w from `images`), by one conversion for the whole dataset.  Run-length and bitmap segmentations, and annotations without one, pass
    through as the same objects.  The result is what COCOEval(..., "segm") reads."""
    if not isinstance(dataset, dict) or "images" not in dataset:
        raise ValueError("dataset_to_rle: the dataset must be a COCO / LVIS dict with `images`")
    anns = list(dataset.get("annotations", []))
    size_of = {im["id"]: (im["height"], im["width"]) for im in dataset["images"]}
    which = [j for j, a in enumerate(anns) if is_polygon_segmentation(a.get("segmentation"))]
    out = dict(dataset)
    if not which:
        out["annotations"] = anns
        return out
    for j in which:
        if anns[j]["image_id"] not in size_of:
            raise ValueError(f"dataset_to_rle: annotation {anns[j].get('id', j)} names image {anns[j]['image_id']}, which `images` lacks")
    r = segmentations_to_rle([anns[j]["segmentation"] for j in which], [size_of[anns[j]["image_id"]] for j in which], device)
    host = np.ascontiguousarray(r.counts.detach().cpu().numpy(), dtype=np.int32)
    for n, j in enumerate(which):
        a = dict(anns[j])
        a["segmentation"] = {"size": [int(r.sizes[n][0]), int(r.sizes[n][1])], "counts": host[r.offsets[n]:r.offsets[n + 1]].tolist()}
        anns[j] = a
    out["annotations"] = anns
    return out
