"""The COCO counts-string codec of the library (mi355det_rle_to_string / mi355det_rle_from_string) and the host side of the run-length
results (RLEBatch, prepare_for_coco_segmentation), without a GPU.

The vectors below are the encoding of those counts under the rule stated in tests/rle_oracle.py (pycocotools rleToString, recalled; no
string here came from pycocotools itself).  The g16 case runs the reference's own pasted masks (tests/golden/g16_maskrcnn.npz, paste_out)
through the numpy encoder: no pixel of that fixture lies within 2e-6 of 0.5, so `> 0.5` pins its run lengths exactly."""
import os

import numpy as np
import pytest

from tests import rle_oracle as ro

torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_maskrcnn.npz")

VECTORS = [
    ([6], "6"),
    ([0, 6], "06"),
    ([0, 1, 1, 1, 1, 1, 1], "0110000"),
    ([3, 1, 3, 1, 3, 1, 2], "313000O"),
    ([4, 2, 1, 2, 3], "42102"),
    ([5, 3, 1000, 2, 40000, 7, 1, 1048576], "53Xo0OhRV15QnhNiooo0"),
    ([100000, 1, 99999, 2, 1, 300000], "PeQ31odQ31R[nLnnT9"),
]


@pytest.fixture(scope="module")
def rle():
    from object_detectors_amd import build
    build.build()
    from object_detectors_amd import rle as mod
    return mod


@pytest.mark.parametrize("counts,string", VECTORS)
def test_vectors(rle, counts, string):
    assert ro.to_string(counts) == string
    assert rle.counts_to_string(counts) == string
    assert rle.string_to_counts(string).tolist() == counts
    assert ro.from_string(string).tolist() == counts


def test_three_by_four_mask(rle):
    m = np.zeros((3, 4), np.uint8)
    m[1:3, 1:3] = 1
    assert ro.encode(m).tolist() == [4, 2, 1, 2, 3]
    assert rle.counts_to_string(ro.encode(m)) == "42102"
    assert ro.area(ro.encode(m)) == 4 and ro.bbox(m) == [1, 1, 2, 2]
    assert np.array_equal(ro.decode([4, 2, 1, 2, 3], 3, 4), m)
    assert ro.encode(np.zeros((2, 3))).tolist() == [6] and ro.encode(np.ones((2, 3))).tolist() == [0, 6]


def test_random_masks_c_equals_numpy(rle):
    rng = np.random.default_rng(20)
    for _ in range(200):
        h, w = int(rng.integers(1, 9)), int(rng.integers(1, 9))
        m = (rng.uniform(size=(h, w)) < rng.uniform()).astype(np.uint8)
        c = ro.encode(m)
        assert int(c.sum()) == h * w
        s = ro.to_string(c)
        assert rle.counts_to_string(c) == s
        back = rle.string_to_counts(s)
        assert back.tolist() == c.tolist() == ro.from_string(s).tolist()
        assert np.array_equal(ro.decode(back, h, w), m)


def test_short_cap_is_an_error(rle):
    counts, string = VECTORS[5]
    n = len(string)
    assert rle.counts_to_string(counts, cap=n + 1) == string              # the characters and the NUL
    with pytest.raises(ValueError):
        rle.counts_to_string(counts, cap=n)                               # one byte short
    with pytest.raises(ValueError):
        rle.counts_to_string(counts, cap=0)
    assert rle.string_to_counts(string, cap=len(counts)).tolist() == counts
    with pytest.raises(ValueError):
        rle.string_to_counts(string, cap=len(counts) - 1)
    with pytest.raises(ValueError):
        rle.string_to_counts("5o")                                        # ends inside a count
    with pytest.raises(ValueError):
        rle.string_to_counts("5 3")                                       # a character outside the alphabet


def test_short_cap_writes_nothing_past_cap():
    import ctypes as C
    from object_detectors_amd import _lib
    counts, string = VECTORS[6]
    c = np.asarray(counts, np.int32)
    cap = 7
    buf = C.create_string_buffer(b"\x7f" * 64, 64)
    assert _lib.lib().mi355det_rle_to_string(c.ctypes.data_as(C.c_void_p), len(counts), buf, cap) < 0
    assert buf.raw[cap:] == b"\x7f" * (64 - cap)
    out = np.full(16, -7, np.int32)
    assert _lib.lib().mi355det_rle_from_string(string.encode(), out.ctypes.data_as(C.c_void_p), 2) < 0
    assert (out[2:] == -7).all()
    # sizing calls: no buffer
    assert _lib.lib().mi355det_rle_to_string(c.ctypes.data_as(C.c_void_p), len(counts), None, 0) == len(string)
    assert _lib.lib().mi355det_rle_from_string(string.encode(), None, 0) == len(counts)


def test_reference_paste_output_through_the_encoder(rle):
    g = np.load(G, allow_pickle=False)
    v = g["paste_out"][:, 0]
    assert float(np.abs(v - np.float32(0.5)).min()) > 2e-6
    masks = v > 0.5
    cs = [ro.encode(m) for m in masks]
    assert [c.size for c in cs] == [63, 1, 295, 3]
    strings = [ro.to_string(c) for c in cs]
    for s, head in zip(strings, ["032NO0g0", "PX1", "Sd0461LL", "02nW1"]):
        assert s.startswith(head), (s[:12], head)
    for c, s, m in zip(cs, strings, masks):
        assert rle.counts_to_string(c) == s and rle.string_to_counts(s).tolist() == c.tolist()
        assert np.array_equal(ro.decode(c, 32, 40), m)


def _hand_batch(rle):
    a = np.zeros((3, 4), np.uint8)
    a[1:3, 1:3] = 1
    b = np.ones((3, 4), np.uint8)
    c = np.zeros((3, 4), np.uint8)
    counts, offs, areas, boxes = ro.encode_batch(np.stack([a, b, c]))
    return rle.RLEBatch((3, 4), torch.from_numpy(counts.astype(np.int32)), offs, torch.tensor(areas), torch.tensor(boxes, dtype=torch.int32)), \
        np.stack([a, b, c])


def test_rle_batch_to_coco_and_decode(rle):
    batch, masks = _hand_batch(rle)
    assert len(batch) == 3 and batch.offsets == [0, 5, 7, 8]
    assert batch.to_coco() == [{"size": [3, 4], "counts": "42102"}, {"size": [3, 4], "counts": "0<"}, {"size": [3, 4], "counts": "<"}]
    assert ro.to_string([0, 12]) == "0<" and ro.to_string([12]) == "<"
    dec = batch.decode()
    assert dec.dtype == torch.uint8 and np.array_equal(dec.numpy(), masks)
    assert batch.area.tolist() == [4, 12, 0] and batch.bbox.tolist() == [[1, 1, 2, 2], [0, 0, 4, 3], [0, 0, 0, 0]]
    with pytest.raises(ValueError):
        rle.RLEBatch((3, 4), torch.zeros(5, dtype=torch.int32), [0, 5, 5])       # a mask without a count
    with pytest.raises(ValueError):
        rle.RLEBatch((3, 4), torch.tensor([4, 2, 1, 2, 2], dtype=torch.int32), [0, 5]).decode()     # does not add up to 12


def test_prepare_for_coco_segmentation_on_rle_batch(rle):
    from object_detectors_amd.tvision.coco_eval import prepare_for_coco_segmentation
    batch, _ = _hand_batch(rle)
    preds = {17: {"boxes": torch.zeros(3, 4), "scores": torch.tensor([0.9, 0.5, 0.25]), "labels": torch.tensor([3, 1, 2]), "masks": batch},
             18: {},
             19: {"boxes": torch.zeros(0, 4), "scores": torch.zeros(0), "labels": torch.zeros(0, dtype=torch.int64),
                  "masks": rle.RLEBatch((3, 4), torch.zeros(0, dtype=torch.int32), [0])}}
    res = prepare_for_coco_segmentation(preds)
    assert len(res) == 3
    for r, (lab, score, counts) in zip(res, [(3, 0.9, "42102"), (1, 0.5, "0<"), (2, 0.25, "<")]):
        assert list(r) == ["image_id", "category_id", "segmentation", "score"]
        assert r["image_id"] == 17 and r["category_id"] == lab and r["score"] == pytest.approx(score)
        assert r["segmentation"] == {"size": [3, 4], "counts": counts}
