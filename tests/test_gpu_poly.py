"""The polygon kernels (csrc/poly_kernels.hip: mi355det_poly_* and mi355det_rle_decode) against tests/poly_oracle.py.

Everything is integers and compared with ==: counts, offsets, area, bbox, bitmaps.  The oracle walks each ring as one list, takes run
lengths by the sort-and-skip loop and unions through bitmaps; the kernels walk edge by edge, use the parity of the multiplicities and
union by coverage events.  Each size's annotations are made and encoded by the oracle once (`case`) and shared by the tests."""
import functools

import numpy as np
import pytest

from tests import poly_oracle as po
from tests.test_oracle_poly import PINNED, SQUARE, UNIONS

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [(1, 1), (7, 5), (37, 53), (5, 300), (300, 4), (19, 1000)]


def dev():
    return torch.device("cuda:0")


def special_annotations(h, w):
    """The cases a random draw may miss: the empty list, one flat polygon, a triangle, more than 64 vertices, edges of more than 64 walk
    steps and (at w = 1000: about 5000) of more than 4096, a part given twice, and 5 parts."""
    k = 70
    ang = 2 * np.pi * np.arange(k) / k
    ring = np.round(np.stack([w / 2 + (w / 2 + 3) * np.cos(ang), h / 2 + (h / 2 + 3) * np.sin(ang)], 1), 1).reshape(-1).tolist()
    wide = [-6.0, -2.5, w + 6.0, h / 2, w + 6.0, h + 6.0, -6.0, h + 5.5]                  # the edges span the image: 5*(w + 12) steps
    sliver = [0.0, 0.0, float(w), float(h), float(w), 0.0]
    tri = [0.5, 0.25, w - 0.5, 0.75, w / 2, h + 2.0]
    return [[], tri, [tri], [ring], [wide], [sliver, sliver], [ring, wide, tri, sliver, ring]]


@functools.lru_cache(maxsize=None)
def case(h, w):
    """(segmentations, oracle counts, offsets, area, bbox, oracle bitmaps [A, h, w]) of about 50 annotations, at most about 160 polygons."""
    rng = np.random.default_rng(1000 * h + w)
    segs = special_annotations(h, w) + [po.random_annotation(rng, h, w) for _ in range(44)]
    assert sum(len(po.parts_of(s)) for s in segs) <= 300
    counts, offs, area, bbox = po.encode_annotations(segs, [(h, w)] * len(segs))
    bitmaps = np.stack([po.annotation_mask(s, h, w) for s in segs])
    return segs, counts, offs, area, bbox, bitmaps


@functools.lru_cache(maxsize=None)
def device_batch(h, w):
    from object_detectors_amd.polygons import polygons_to_rle
    return polygons_to_rle(case(h, w)[0], h, w, dev())


def assert_fields(counts, offsets, area, bbox, want):
    w_counts, w_offs, w_area, w_bbox = want
    assert [int(o) for o in offsets] == w_offs
    got = counts.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), w_counts)
    assert area.dtype == torch.int64 and np.array_equal(area.cpu().numpy(), w_area)
    assert bbox.dtype == torch.int32 and np.array_equal(bbox.cpu().numpy(), w_bbox)


def test_pinned_cases_in_one_call():
    """The hand-checked polygons and unions of tests/test_oracle_poly.py, each at its own image size, in one conversion."""
    from object_detectors_amd.polygons import segmentations_to_rle
    segs = [p for _h, _w, p, _c in PINNED] + [parts for _n, parts, _b in UNIONS] + [[]]
    sizes = [(h, w) for h, w, _p, _c in PINNED] + [(12, 12)] * len(UNIONS) + [(5, 7)]
    r = segmentations_to_rle(segs, sizes, dev())
    got = r.counts.cpu().tolist()
    for j, (_h, _w, _p, want) in enumerate(PINNED):
        assert got[r.offsets[j]:r.offsets[j + 1]] == want, j
    assert got[r.offsets[-2]:] == [35]
    assert_fields(r.counts, r.offsets, r.area, r.bbox, po.encode_annotations(segs, sizes))
    assert np.array_equal(r.sizes, np.asarray(sizes, np.int32))


@pytest.mark.parametrize("h,w", SIZES)
def test_random_annotations_exact(h, w):
    segs, counts, offs, area, bbox, _bits = case(h, w)
    b = device_batch(h, w)
    assert b.size == (h, w) and len(b) == len(segs) and b.counts.is_cuda and b.area.is_cuda and b.bbox.is_cuda
    assert_fields(b.counts, b.offsets, b.area, b.bbox, (counts, offs, area, bbox))
    c = b.counts_host().astype(np.int64)
    for j in range(len(segs)):
        one = c[offs[j]:offs[j + 1]]
        assert int(one.sum()) == h * w and (one[1:] > 0).all()                  # canonical: only the first count may be 0


def test_long_edges_are_in_the_sample():
    """More than 64 and more than 4096 walk steps on one edge, 3 and more than 64 vertices, 1 to 5 parts: the sample holds them."""
    segs = case(19, 1000)[0]
    steps = []
    for s in segs:
        for p in po.parts_of(s):
            X, Y = po.scale(p)
            steps += [max(abs(X[j + 1] - X[j]), abs(Y[j + 1] - Y[j])) for j in range(len(X) - 1)]
    assert max(steps) > 4096 and any(64 < n <= 4096 for n in steps)
    verts = [len(p) // 2 for s in segs for p in po.parts_of(s)]
    assert min(verts) == 3 and max(verts) > 64
    assert {len(po.parts_of(s)) for s in segs} >= {0, 1, 2, 3, 4, 5}


@pytest.mark.parametrize("h,w", SIZES)
def test_two_calls_give_identical_bits(h, w):
    from object_detectors_amd.polygons import polygons_to_rle
    a, b = device_batch(h, w), polygons_to_rle(case(h, w)[0], h, w, dev())
    assert a.offsets == b.offsets
    for x, y in ((a.counts, b.counts), (a.area, b.area), (a.bbox, b.bbox)):
        assert torch.equal(x, y)


def test_several_sizes_in_one_call_and_no_annotations():
    from object_detectors_amd.polygons import polygons_to_rle, segmentations_to_rle
    rng = np.random.default_rng(3)
    segs, sizes = [], []
    for _ in range(60):
        h, w = SIZES[int(rng.integers(0, len(SIZES) - 1))]
        segs.append(po.random_annotation(rng, h, w) if rng.integers(0, 8) else [])
        sizes.append((h, w))
    r = segmentations_to_rle(segs, sizes, dev())
    assert_fields(r.counts, r.offsets, r.area, r.bbox, po.encode_annotations(segs, sizes))
    none = segmentations_to_rle([], [], dev())
    assert none.offsets == [0] and none.counts.shape == (0,) and none.area.shape == (0,) and none.bbox.shape == (0, 4)
    assert none.counts.dtype == torch.int32 and none.counts.is_cuda
    b = polygons_to_rle([], 7, 5, dev())
    assert len(b) == 0 and b.size == (7, 5)
    only_empty = polygons_to_rle([[], []], 7, 5, dev())                         # annotations, but not one polygon
    assert only_empty.counts.cpu().tolist() == [35, 35] and only_empty.area.cpu().tolist() == [0, 0]


SCAN_TRIANGLES = [[0.5, 0.5, 3.5, 0.5, 2.0, 3.5], [0.0, 0.0, 4.0, 4.0, 4.0, 0.0], [1.0, 1.0, 3.0, 1.25, 1.25, 3.0]]
SCAN_POOL = [[t] for t in SCAN_TRIANGLES] + [[SCAN_TRIANGLES[0], SCAN_TRIANGLES[2]], []]          # one part, one part, one part, two, none


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2048, 2049, 8191, 8192, 8193, 16385])
def test_run_offsets_at_the_edges_of_the_scan(n):
    """The offsets scan (csrc/offsets_scan.h: over the polygons' points and toggles and over the annotations' runs) at one item, a wave
    boundary, the step from the small block to the large one (256 x 8 items), a round of 1024 x 8 items and the carry into a third round:
    n annotations of triangles on 4 x 4 images, a deterministic mix of one part, two parts and none, each form encoded by the oracle once."""
    from object_detectors_amd.polygons import polygons_to_rle
    p_counts, p_offs, p_area, p_bbox = po.encode_annotations(SCAN_POOL, [(4, 4)] * len(SCAN_POOL))
    p_offs = np.asarray(p_offs, np.int64)
    i = np.arange(n)
    kind = np.where(i % 11 == 3, 3, np.where(i % 11 == 7, 4, (i + i // 5) % 3))
    offs = np.concatenate([[0], np.cumsum(np.diff(p_offs)[kind])])
    assert n < 63 or len(set(np.diff(offs).tolist())) >= 3
    b = polygons_to_rle([SCAN_POOL[k] for k in kind], 4, 4, dev())
    want = np.concatenate([p_counts[p_offs[k]:p_offs[k + 1]] for k in kind]) if n else np.zeros(0, np.int64)
    assert len(b) == n
    assert_fields(b.counts, b.offsets, b.area, b.bbox, (want, offs.tolist(), np.asarray(p_area)[kind], np.asarray(p_bbox).reshape(-1, 4)[kind]))


def test_nothing_is_written_past_the_capacity():
    from object_detectors_amd import ops
    from object_detectors_amd.polygons import flatten
    h, w = 37, 53
    segs, counts, offs, _area, _bbox, _bits = case(h, w)
    tables = flatten(segs, [(h, w)] * len(segs))
    total = offs[-1]
    buf = torch.full((total + 64,), -7, dtype=torch.int32, device=dev())
    got, got_offs, _a, _b = ops.poly_rle(*tables, capacity=total, device=dev(), out=buf)
    assert got.data_ptr() == buf.data_ptr() and got_offs == offs
    host = buf.cpu().numpy()
    assert np.array_equal(host[:total].astype(np.int64), counts) and (host[total:] == -7).all()
    with pytest.raises(ValueError):
        ops.poly_rle(*tables, capacity=total - 1, device=dev(), out=buf)       # refused on the host side of the entry point, no launch
    assert (buf.cpu().numpy()[total:] == -7).all()


@pytest.mark.parametrize("h,w", SIZES)
def test_decode_and_round_trip(h, w):
    """ops.mask_rle_decode == RLEBatch.decode() == the oracle's bitmaps, and the existing encoder gives the same counts back."""
    from object_detectors_amd import ops
    bits = case(h, w)[5]
    b = device_batch(h, w)
    got = ops.mask_rle_decode(b)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == bits.shape
    assert torch.equal(got.cpu(), b.decode()) and np.array_equal(got.cpu().numpy(), bits)
    again = ops.mask_rle_decode(b.counts, torch.tensor(b.offsets), b.size)
    assert torch.equal(again, got)
    back = ops.mask_rle_dense(got.float())
    assert back.offsets == b.offsets and torch.equal(back.counts, b.counts)
    assert torch.equal(back.area, b.area) and torch.equal(back.bbox, b.bbox)


def test_decode_of_no_masks_and_of_short_counts():
    from object_detectors_amd import ops
    none = ops.mask_rle_decode(torch.empty(0, dtype=torch.int32, device=dev()), [0], (4, 6))
    assert tuple(none.shape) == (0, 4, 6) and none.dtype == torch.uint8
    # counts that run past h*w are cut there, counts that stop short leave zeros: nothing is written outside the mask
    c = torch.tensor([3, 100, 5, 2, 1], dtype=torch.int32, device=dev())
    got = ops.mask_rle_decode(c, [0, 2, 5], (4, 6)).cpu().numpy()
    want = np.zeros((2, 24), np.uint8)
    want[0, 3:] = 1
    want[1, 5:7] = 1
    assert np.array_equal(got, want.reshape(2, 6, 4).transpose(0, 2, 1))


def test_convert_coco_poly_to_mask_and_mask_targets():
    from object_detectors_amd import ops
    from object_detectors_amd.tvision.coco_utils import convert_coco_poly_to_mask
    h, w = 37, 53
    segs, _c, _o, _a, _b, bits = case(h, w)
    masks = convert_coco_poly_to_mask(segs, h, w, dev())
    assert masks.dtype == torch.uint8 and masks.is_cuda and np.array_equal(masks.cpu().numpy(), bits)
    none = convert_coco_poly_to_mask([], h, w, dev())
    assert tuple(none.shape) == (0, h, w) and none.dtype == torch.uint8
    rng = np.random.default_rng(8)
    n = 40
    x0, y0 = rng.uniform(0, w - 8, n), rng.uniform(0, h - 8, n)
    rois = np.stack([np.zeros(n), x0, y0, x0 + rng.uniform(2, 30, n), y0 + rng.uniform(2, 30, n)], 1).astype(np.float32)
    gt = torch.from_numpy(rng.integers(0, len(segs), n)).to(dev())
    rois = torch.from_numpy(rois).to(dev())
    want = ops.mask_targets([torch.from_numpy(bits).to(dev())], rois, gt)
    assert torch.equal(ops.mask_targets([masks], rois, gt), want) and want.sum() > 0


def test_convert_coco_polys_to_mask_target():
    """coco_utils.py:50-108: the crowd is dropped, the boxes become clamped corners, the empty box is filtered with its mask."""
    from object_detectors_amd.tvision.coco_utils import ConvertCocoPolysToMask
    tri = [1, 1, 9, 1, 9, 9]
    anno = [{"bbox": [1, 1, 8, 8], "category_id": 3, "segmentation": [SQUARE], "area": 64.0, "iscrowd": 0, "keypoints": [1, 2, 2, 0, 0, 0]},
            {"bbox": [0, 0, 5, 5], "category_id": 4, "segmentation": [SQUARE], "area": 1.0, "iscrowd": 1, "keypoints": [0] * 6},
            {"bbox": [4, 4, 0, 3], "category_id": 5, "segmentation": [tri], "area": 0.0, "iscrowd": 0, "keypoints": [0] * 6},
            {"bbox": [1, 1, 20, 8], "category_id": 6, "segmentation": [tri, SQUARE], "area": 64.0, "iscrowd": 0, "keypoints": [3, 3, 1, 4, 4, 2]}]
    image = torch.zeros(3, 12, 14)
    out_image, t = ConvertCocoPolysToMask(dev())(image, {"image_id": 17, "annotations": anno})
    assert out_image is image and t["image_id"].tolist() == [17]
    assert t["boxes"].tolist() == [[1, 1, 9, 9], [1, 1, 14, 9]] and t["boxes"].dtype == torch.float32
    assert t["labels"].tolist() == [3, 6] and t["labels"].dtype == torch.int64
    want = np.stack([po.annotation_mask([SQUARE], 12, 14), po.annotation_mask([tri, SQUARE], 12, 14)])
    assert t["masks"].is_cuda and t["masks"].dtype == torch.uint8 and np.array_equal(t["masks"].cpu().numpy(), want)
    assert t["keypoints"].tolist() == [[[1, 2, 2], [0, 0, 0]], [[3, 3, 1], [4, 4, 2]]]
    assert t["area"].tolist() == [64.0, 0.0, 64.0] and t["iscrowd"].tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- evaluation
def make_polygon_dataset(seed):
    """Images of two sizes, polygon ground truth of 1 to 3 parts (one annotation already run lengths), and detections that are jittered
    copies of it, rasterised by the oracle."""
    rng = np.random.default_rng(seed)
    images = [{"id": 10 + i, "height": h, "width": w} for i, (h, w) in enumerate([(37, 53), (37, 53), (30, 44), (30, 44)])]
    anns, results = [], []
    for im in images:
        h, w = im["height"], im["width"]
        for cat in (1, 2):
            for _ in range(int(rng.integers(1, 4))):
                cx, cy, r = rng.uniform(8, w - 8), rng.uniform(8, h - 8), rng.uniform(3, 9)
                seg = []
                for _p in range(int(rng.integers(1, 4))):
                    k = int(rng.integers(3, 9))
                    ang = np.sort(rng.uniform(0, 2 * np.pi, k))
                    rad = rng.uniform(0.5, 1.0, k) * r
                    ox, oy = rng.uniform(-3, 3, 2)
                    seg.append(np.round(np.stack([cx + ox + rad * np.cos(ang), cy + oy + rad * np.sin(ang)], 1), 2).reshape(-1).tolist())
                m = po.annotation_mask(seg, h, w)
                anns.append({"id": len(anns) + 1, "image_id": im["id"], "category_id": cat, "segmentation": seg, "bbox": [0, 0, 1, 1],
                             "area": float(m.sum()) * [1.0, 10.0, 100.0][len(anns) % 3], "iscrowd": int(rng.uniform() < 0.2)})
                for _d in range(int(rng.integers(0, 3))):
                    d = np.roll(m, (int(rng.integers(-1, 2)), int(rng.integers(-1, 2))), (0, 1))
                    d[int(rng.integers(0, h))] = 0
                    results.append({"image_id": im["id"], "category_id": cat, "score": float(rng.integers(1, 21)) / 20,
                                    "segmentation": {"size": [h, w], "counts": po.ro.encode(d).tolist()}})
    seg0 = anns[0]["segmentation"]
    anns[0] = dict(anns[0], segmentation={"size": [37, 53], "counts": po.annotation_counts(seg0, 37, 53).tolist()})
    return {"images": images, "categories": [{"id": 1}, {"id": 2}], "annotations": anns}, results


def _evaluate(dataset, results):
    from object_detectors_amd.cocoeval import COCOEval
    e = COCOEval(dataset, "segm")
    e.add_results(results)
    e.evaluate()
    e.accumulate()
    e.summarize()
    return e


def test_cocoeval_on_converted_dataset():
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.polygons import dataset_to_rle, is_polygon_segmentation
    ds, results = make_polygon_dataset(31)
    size_of = {im["id"]: (im["height"], im["width"]) for im in ds["images"]}
    by_oracle = dict(ds, annotations=[
        dict(a, segmentation={"size": list(size_of[a["image_id"]]), "counts": po.annotation_counts(a["segmentation"], *size_of[a["image_id"]]).tolist()})
        if is_polygon_segmentation(a["segmentation"]) else a for a in ds["annotations"]])
    converted = dataset_to_rle(ds, dev())
    assert converted["annotations"][0] is ds["annotations"][0]                 # run lengths pass through as the same object
    assert all(isinstance(a["segmentation"], dict) for a in converted["annotations"])
    assert [a["segmentation"]["counts"] for a in converted["annotations"]] == [a["segmentation"]["counts"] for a in by_oracle["annotations"]]
    assert is_polygon_segmentation(ds["annotations"][1]["segmentation"])      # the input is left as it was
    got, want = _evaluate(converted, results), _evaluate(by_oracle, results)
    assert want.stats[0] > 0
    for name in ("stats", "precision", "recall"):
        assert np.array_equal(getattr(got, name), getattr(want, name)), name
    with pytest.raises(NotImplementedError, match="polygon"):                  # wiring the evaluator itself is a later change
        COCOEval(ds, "segm")
