"""The run-length kernels (csrc/rle_kernels.hip: mi355det_mask_rle_count / _emit) against tests/rle_oracle.py.

Everything here is exact: counts, offsets, area and bbox are integers.  The dense predicate is held to the numpy encoder on patterns that
exercise every transition case; the fused paste predicate to the dense kernel and to the numpy encoder, both applied to
`ops.paste_masks(...) > 0.5` on the same inputs (the two kernels share the pixel rule of csrc/mask_paste.h, so the bits agree exactly); then
to the reference's own pasted masks (tests/golden/g16_maskrcnn.npz) and, through MaskRCNN(mask_format="rle"), to the dense model output."""
import os

import numpy as np
import pytest

from tests import mask_oracle as mo
from tests import rle_oracle as ro

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_maskrcnn.npz")


def dev():
    return torch.device("cuda:0")


def check_batch(batch, bits):
    """batch (RLEBatch) == the numpy encoding of bits [D, H, W] (bool), field by field."""
    d, h, w = bits.shape
    counts, offs, areas, boxes = ro.encode_batch(bits)
    assert batch.size == (h, w) and len(batch) == d
    assert batch.offsets == offs
    got = batch.counts.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), counts)
    assert batch.area.dtype == torch.int64 and batch.area.cpu().tolist() == areas
    assert batch.bbox.dtype == torch.int32 and batch.bbox.cpu().tolist() == boxes
    for i in range(d):
        c = got[offs[i]:offs[i + 1]].astype(np.int64)
        assert int(c.sum()) == h * w and int(c[1::2].sum()) == areas[i]


def dense_patterns(h, w, seed):
    """fp32 [9, h, w]: every transition case of the column-major walk."""
    rng = np.random.default_rng(seed)
    p = np.zeros((9, h, w), np.float32)
    p[1] = 1.0                                             # all one: [0, h*w]
    p[2, 0, 0] = 1.0                                       # only pixel 0: a leading run of 0 zeros
    p[3, h - 1, w - 1] = 1.0                               # only the last pixel
    yy, xx = np.mgrid[0:h, 0:w]
    p[4] = ((yy + xx) & 1).astype(np.float32)              # checkerboard: a transition at every pixel of a column (odd h: not at the seam)
    p[5, h - 2:, 1] = 1.0                                  # one run from the bottom of column 1 ...
    p[5, :2, 2] = 1.0                                      # ... into the top of column 2 (no transition at the seam)
    p[5, h - 1, w - 2] = 1.0                               # a run that ends with its column (the transition is the next column's first pixel)
    p[6] = 0.5                                             # exactly the threshold: strict >, so 0
    p[6, 1, 1] = np.nextafter(np.float32(0.5), np.float32(1))
    p[7] = rng.uniform(0, 1, (h, w)).astype(np.float32)
    p[8] = (rng.uniform(0, 1, (h, w)) < 0.03).astype(np.float32) * 0.9      # sparse: most columns empty
    return p


@pytest.mark.parametrize("h,w", [(7, 5), (37, 53), (19, 300), (300, 21)])
def test_dense_exact(h, w):
    from object_detectors_amd import ops
    p = dense_patterns(h, w, 100 + h)
    batch = ops.mask_rle_dense(torch.from_numpy(p).to(dev()))
    check_batch(batch, p > np.float32(0.5))
    assert batch.counts_of(0).tolist() == [h * w] and batch.counts_of(1).tolist() == [0, h * w]
    assert batch.counts_of(2).tolist() == [0, 1, h * w - 1] and batch.counts_of(3).tolist() == [h * w - 1, 1]
    assert batch.counts_of(6).tolist() == [h + 1, 1, h * w - h - 2]
    assert np.array_equal(batch.decode().numpy(), (p > np.float32(0.5)).astype(np.uint8))
    # the [D, 1, H, W] form of the reference, another threshold, and the strings
    b2 = ops.mask_rle_dense(torch.from_numpy(p[:, None]).to(dev()), threshold=0.25)
    check_batch(b2, p > np.float32(0.25))
    assert [r["counts"] for r in batch.to_coco()] == [ro.to_string(batch.counts_of(i)) for i in range(len(batch))]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2048, 2049, 8191, 8192, 8193, 16385])
def test_run_offsets_at_the_edges_of_the_scan(n):
    """The offsets scan (csrc/offsets_scan.h) at one item, a wave boundary, the step from the small block to the large one (256 x 8 items),
    a round of 1024 x 8 items and the carry into a third round: n dense 2 x 2 masks, a deterministic mix of all 16, each pattern encoded by the oracle once."""
    from object_detectors_amd import ops
    pattern = ((np.arange(16)[:, None] >> np.arange(4)) & 1).astype(bool).reshape(16, 2, 2)
    p_counts, p_offs, p_area, p_bbox = ro.encode_batch(pattern)
    p_offs = np.asarray(p_offs, np.int64)
    kind = (np.arange(n) * 7 + np.arange(n) // 5) % 16
    offs = np.concatenate([[0], np.cumsum(np.diff(p_offs)[kind])])
    assert n < 16 or len(set(np.diff(offs).tolist())) >= 4
    batch = ops.mask_rle_dense(torch.from_numpy(pattern[kind].astype(np.float32)).to(dev()))
    assert batch.size == (2, 2) and len(batch) == n and batch.offsets == offs.tolist()
    want = np.concatenate([p_counts[p_offs[k]:p_offs[k + 1]] for k in kind]) if n else np.zeros(0, np.int64)
    got = batch.counts.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), want)
    assert batch.area.dtype == torch.int64 and np.array_equal(batch.area.cpu().numpy(), np.asarray(p_area, np.int64)[kind])
    assert batch.bbox.dtype == torch.int32 and np.array_equal(batch.bbox.cpu().numpy(), np.asarray(p_bbox, np.int32).reshape(16, 4)[kind])
    if 0 < n <= 65:
        assert np.array_equal(batch.decode().numpy(), pattern[kind].astype(np.uint8))


def test_dense_no_masks():
    from object_detectors_amd import ops
    b = ops.mask_rle_dense(torch.zeros((0, 6, 4), device=dev()))
    assert len(b) == 0 and b.offsets == [0] and b.counts.shape == (0,) and b.to_coco() == [] and b.decode().shape == (0, 6, 4)
    b = ops.mask_rle_paste(torch.zeros((0, 1, 28, 28), device=dev()), torch.zeros((0, 4), device=dev()), (6, 4))
    assert len(b) == 0 and b.size == (6, 4) and b.area.shape == (0,) and b.bbox.shape == (0, 4)


def paste_cases(h, w, m, seed):
    """(probabilities [24, 1, m, m], boxes [24, 4]): six kinds of box x four kinds of probabilities."""
    rng = np.random.default_rng(seed)
    boxes = np.array([[w * 0.2, h * 0.25, w * 0.7, h * 0.8],                 # inside
                      [-6.5, -4.25, w * 0.4, h * 0.5],                       # clipped at the top-left
                      [w * 0.55, h * 0.4, w + 7.5, h + 3.25],                # clipped at the bottom-right
                      [-5.0, -5.0, w + 5.0, h + 5.0],                        # the whole image and beyond: box rows 0..h-1, runs wrap
                      [10.2, 11.3, 10.6, 11.9],                              # sub-pixel
                      [w + 10.0, h + 10.0, w + 30.0, h + 40.0]], np.float32)     # wholly outside: [h*w]
    yy, xx = np.mgrid[0:m, 0:m].astype(np.float32)
    blob = np.exp(-(((yy - m * 0.45) / (m * 0.3)) ** 2 + ((xx - m * 0.55) / (m * 0.22)) ** 2)).astype(np.float32)
    probs = [rng.uniform(0, 1, (m, m)).astype(np.float32), np.ones((m, m), np.float32), np.zeros((m, m), np.float32), blob]
    pp = np.stack([p for p in probs for _ in boxes])[:, None]
    bb = np.concatenate([boxes for _ in probs])
    return pp, bb


@pytest.mark.parametrize("h,w,pad", [(37, 53, 1), (64, 300, 1), (37, 53, 0)])
def test_paste_exact(h, w, pad):
    from object_detectors_amd import ops
    pp, bb = paste_cases(h, w, 28, 7 * h + pad)
    tp, tb = torch.from_numpy(pp).to(dev()), torch.from_numpy(bb).to(dev())
    fused = ops.mask_rle_paste(tp, tb, (h, w), padding=pad)
    pasted = ops.paste_masks(tp, tb, (h, w), padding=pad)
    dense = ops.mask_rle_dense(pasted)
    bits = pasted[:, 0].cpu().numpy() > np.float32(0.5)
    check_batch(dense, bits)
    check_batch(fused, bits)
    assert fused.offsets == dense.offsets and torch.equal(fused.counts, dense.counts)
    assert torch.equal(fused.area, dense.area) and torch.equal(fused.bbox, dense.bbox)
    for k in range(4):                                     # every kind of probabilities: the box wholly outside is the one run [h*w]
        assert fused.counts_of(6 * k + 5).tolist() == [h * w]
    assert int(fused.area[6 + 3]) == h * w if pad == 0 else int(fused.area[6 + 3]) > 0      # all ones, whole image
    assert fused.area[12:18].tolist() == [0] * 6           # all-zero probabilities
    again = ops.mask_rle_paste(tp, tb, (h, w), padding=pad)
    assert again.offsets == fused.offsets and torch.equal(again.counts, fused.counts)


def test_paste_800px():
    from object_detectors_amd import ops
    rng = np.random.default_rng(12)
    d = 12
    x1, y1 = rng.uniform(-40, 1000, d), rng.uniform(-40, 760, d)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0.5, 300, d), y1 + rng.uniform(0.5, 300, d)], 1).astype(np.float32)
    masks = rng.uniform(0, 1, (d, 1, 28, 28)).astype(np.float32)
    tp, tb = torch.from_numpy(masks).to(dev()), torch.from_numpy(boxes).to(dev())
    fused = ops.mask_rle_paste(tp, tb, (800, 1066))
    bits = ops.paste_masks(tp, tb, (800, 1066))[:, 0].cpu().numpy() > np.float32(0.5)
    check_batch(fused, bits)


def test_reference_fixture():
    from object_detectors_amd import ops
    g = np.load(G, allow_pickle=False)
    assert float(np.abs(g["paste_out"] - np.float32(0.5)).min()) > 2e-6
    fused = ops.mask_rle_paste(torch.from_numpy(g["paste_masks"]).to(dev()), torch.from_numpy(g["paste_boxes"]).to(dev()), (32, 40))
    check_batch(fused, g["paste_out"][:, 0] > np.float32(0.5))
    assert [len(fused.counts_of(i)) for i in range(4)] == [63, 1, 295, 3]
    for r, head in zip(fused.to_coco(), ["032NO0g0", "PX1", "Sd0461LL", "02nW1"]):
        assert r["size"] == [32, 40] and r["counts"].startswith(head)
    for i, o_s in enumerate([(96, 128), (50, 45)]):
        v = mo.paste_masks_in_image(g[f"det_probs{i}"], g[f"post_boxes{i}"], o_s)[:, 0]
        near = np.abs(v - np.float32(0.5)) <= 2e-6
        assert float(near.mean()) < 1e-3                   # the CPU restatement itself: the share of pixels too close to the threshold to pin
        fused = ops.mask_rle_paste(torch.from_numpy(g[f"det_probs{i}"]).to(dev()), torch.from_numpy(g[f"post_boxes{i}"]).to(dev()), o_s)
        got = fused.decode().numpy().astype(bool)
        assert np.array_equal(got[~near], (v > np.float32(0.5))[~near])


def test_model_rle_equals_dense_masks():
    from oracle import detrand
    from object_detectors_amd.rle import RLEBatch
    from object_detectors_amd.tvision.coco_eval import prepare_for_coco_segmentation
    from object_detectors_amd.tvision.mask_rcnn import maskrcnn_resnet50_fpn
    torch.manual_seed(2)
    model = maskrcnn_resnet50_fpn(num_classes=5, device=dev(), seed=2, min_size=128, max_size=128, box_score_thresh=0.0, mask_format="rle")
    model.eval()
    imgs = [torch.from_numpy(detrand.uniform(4300 + i, (3, h, w), 0.0, 1.0)).to(dev()) for i, (h, w) in enumerate([(100, 140), (150, 90)])]
    with torch.no_grad():
        det_rle = model(imgs)
        model.mask_format = "dense"
        det = model(imgs)
    torch.cuda.synchronize()
    total = 0
    for i, (a, b) in enumerate(zip(det_rle, det)):
        h0, w0 = (int(v) for v in imgs[i].shape[-2:])
        n = int(b["boxes"].shape[0])
        total += n
        assert torch.equal(a["boxes"], b["boxes"]) and torch.equal(a["scores"], b["scores"]) and torch.equal(a["labels"], b["labels"])
        assert isinstance(a["masks"], RLEBatch) and a["masks"].size == (h0, w0) and len(a["masks"]) == n
        assert b["masks"].shape == (n, 1, h0, w0)
        bits = (b["masks"][:, 0] > 0.5).cpu()
        assert torch.equal(a["masks"].decode(), bits.to(torch.uint8))
        assert a["masks"].area.cpu().tolist() == bits.flatten(1).sum(1).tolist()
    assert total > 0
    assert prepare_for_coco_segmentation(dict(enumerate(det_rle))) == prepare_for_coco_segmentation(dict(enumerate(det)))
    with pytest.raises(ValueError):
        model.transform.postprocess([], [], [], mask_format="polygon")


def test_errors():
    from object_detectors_amd import _lib, ops
    L = _lib.lib()
    x = torch.zeros((1, 4, 4), device=dev())
    ro64 = torch.zeros(2, dtype=torch.int64, device=dev())
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev())
    # im_h*im_w >= 2^31: refused on the arguments alone (nothing of that size exists, nothing is launched)
    st = L.mi355det_mask_rle_count(_lib.ptr(x), None, None, 1, 1, 0, 65536, 32768, 0.5, _lib.ptr(ro64), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert st == -1 and b"2147483648" in L.mi355det_last_error()
    with pytest.raises(ValueError):
        _lib.check(st, "mask_rle_count")
    assert L.mi355det_mask_rle_count(None, None, None, 1, 28, 1, 4, 4, 0.5, _lib.ptr(ro64), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1
    assert b"missing operand" in L.mi355det_last_error()
    assert L.mi355det_mask_rle_count(_lib.ptr(x), None, None, 1, 1, 0, 4, 4, 0.5, _lib.ptr(ro64), _lib.ptr(ws), 8, _lib.stream_ptr()) == -3
    assert L.mi355det_mask_rle_count(_lib.ptr(x), None, None, 1, 1, 0, 0, 4, 0.5, _lib.ptr(ro64), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1
    # what the emit pass says of the numbers read back from the count pass, word for word (refused before any launch)
    buf = torch.zeros(8, dtype=torch.int32, device=dev())
    emit = lambda total=3, counts=_lib.ptr(buf), cap=3: L.mi355det_mask_rle_emit(
        _lib.ptr(x), None, None, 1, 1, 0, 4, 4, 0.5, _lib.ptr(ro64), total, counts, cap, None, None, _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    for kw, text in ((dict(cap=2), "mask_rle_emit: capacity 2 is smaller than the 3 counts"),
                     (dict(total=0), "mask_rle_emit: total_runs 0 is below one count per mask"),
                     (dict(counts=None), "mask_rle_emit: missing operand")):
        assert emit(**kw) == -1, kw
        assert L.mi355det_last_error().decode() == text
    with pytest.raises(ValueError):
        ops.mask_rle_dense(torch.zeros((1, 4, 4)))                        # a CPU tensor
    with pytest.raises(ValueError):
        ops.mask_rle_paste(torch.zeros((1, 1, 28, 28)), torch.zeros((1, 4)), (8, 8))
    with pytest.raises(ValueError):
        ops.mask_rle_paste(torch.zeros((1, 1, 28, 28), device=dev()), torch.zeros((1, 4), device=dev()), (8, 8), threshold=-0.1)
    p = torch.from_numpy(dense_patterns(7, 5, 1)).to(dev())
    total = ops.mask_rle_dense(p).offsets[-1]
    with pytest.raises(ValueError, match="capacity"):
        ops.mask_rle_dense(p, capacity=total - 1)                         # a short counts buffer: refused through check()
