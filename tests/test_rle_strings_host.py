"""Host side of the string route (ops.rle_strings*, rle.pack_strings, cocoeval._MaskStore, lviseval.LVISSegmEval): the wrappers refuse CPU
tensors, the C entries refuse bad tables before any launch, a mask store on the CPU keeps the host route, and the new names exist.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import rle_oracle as ro

torch = pytest.importorskip("torch")

MASKS = [np.array([[0, 1, 1], [0, 1, 0]], np.uint8), np.zeros((3, 2), np.uint8), np.ones((2, 2), np.uint8),
         np.array([[0, 0, 0, 1], [1, 1, 0, 1], [0, 1, 0, 1]], np.uint8)]


def _segs():
    return [{"size": list(m.shape), "counts": ro.to_string(ro.encode(m))} for m in MASKS]


def test_the_new_names_import():
    from object_detectors_amd import _lib, ops, rle
    from object_detectors_amd.cocoeval import _MaskStore
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    assert issubclass(LVISSegmEval, LVISEval)
    assert callable(ops.rle_strings) and callable(ops.rle_strings_count) and callable(ops.rle_strings_emit) and callable(rle.pack_strings)
    assert callable(_MaskStore.add_strings)
    for name in ("mi355det_rle_strings_count", "mi355det_rle_strings_emit"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
    assert [ops.RLESTR_RANGE, ops.RLESTR_SIZE, ops.RLESTR_ALPHABET, ops.RLESTR_LONG, ops.RLESTR_OPEN, ops.RLESTR_INT32, ops.RLESTR_NEGATIVE,
            ops.RLESTR_SUM] == [1, 2, 4, 8, 16, 32, 64, 128]
    header = open(_lib.HERE + "/../include/mi355det.h").read()
    for name, bit in (("RANGE", 1), ("SIZE", 2), ("ALPHABET", 4), ("LONG", 8), ("OPEN", 16), ("INT32", 32), ("NEGATIVE", 64), ("SUM", 128)):
        assert f"#define MI355DET_RLESTR_{name} {bit} " in header


def test_pack_strings():
    from object_detectors_amd.rle import pack_strings
    packed, off = pack_strings(["ab", "", "cde"])
    assert packed.dtype == np.uint8 and packed.tobytes() == b"abcde" and off.dtype == np.int64 and off.tolist() == [0, 2, 2, 5]
    packed, off = pack_strings([b"ab", "c", b"\xff"])                 # bytes pass as they are
    assert packed.tobytes() == b"abc\xff" and off.tolist() == [0, 2, 3, 4]
    packed, off = pack_strings(["ab\0cd", b"e\0", "f"])               # a string ends at its first NUL, as for the C codec
    assert packed.tobytes() == b"abef" and off.tolist() == [0, 2, 3, 4]
    packed, off = pack_strings([])
    assert packed.size == 0 and off.tolist() == [0]


def test_wrappers_refuse_cpu_tensors():
    from object_detectors_amd import ops
    b, off, sz = torch.zeros(4, dtype=torch.uint8), torch.tensor([0, 4]), torch.tensor([[2, 2]], dtype=torch.int32)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.rle_strings_count(b, np.array([0, 4]), off, sz)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.rle_strings_emit(b, off, sz, torch.tensor([0, 1]), 1)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.rle_strings(np.zeros(4, np.uint8), np.array([0, 4]), np.array([[2, 2]]), device="cpu")


def test_c_entries_refuse_bad_tables():
    """Every refusal comes before a launch: the pointers are host memory (or made up), and nothing is ever read through them."""
    from object_detectors_amd import _lib
    L = _lib.lib()
    off = np.array([0, 3, 5], np.int64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    fake = C.c_void_p(4096)                                           # stands for a device table; refused calls do not touch it
    out, num_bad, status = np.zeros(3, np.int64), np.zeros(1, np.int64), np.zeros(2, np.uint8)
    count = lambda bytes_=fake, nb=5, host=p(off), dev=fake, sizes=fake, n=2, runs=p(out), st=p(status), bad=p(num_bad): \
        L.mi355det_rle_strings_count(bytes_, nb, host, dev, sizes, n, runs, st, bad, None)
    for kw in (dict(n=-1), dict(nb=-1), dict(host=None), dict(dev=None), dict(sizes=None), dict(bytes_=None), dict(runs=None), dict(st=None),
               dict(bad=None)):
        assert count(**kw) == -1, kw
        assert L.mi355det_last_error().decode().startswith("rle_strings_count")
    assert count(host=p(np.array([0, 6, 5], np.int64))) == -1 and b"descend" in L.mi355det_last_error()
    assert count(host=p(np.array([1, 3, 5], np.int64))) == -1 and count(host=p(np.array([0, 3, 4], np.int64))) == -1
    emit = lambda bytes_=fake, nb=5, dev=fake, sizes=fake, n=2, runs=fake, total=4, counts=fake, cap=4: \
        L.mi355det_rle_strings_emit(bytes_, nb, dev, sizes, n, runs, total, counts, cap, None, None, None)
    for kw in (dict(n=-1), dict(dev=None), dict(sizes=None), dict(bytes_=None), dict(runs=None), dict(counts=None), dict(total=-1), dict(cap=3)):
        assert emit(**kw) == -1, kw
        assert L.mi355det_last_error().decode().startswith("rle_strings_emit")
    assert emit(n=0, dev=None, sizes=None, runs=None, counts=None) == 0          # no mask: nothing to do, no launch
    # what the emit pass says of the numbers read back from the count pass, word for word
    for kw, text in ((dict(cap=3), "rle_strings_emit: capacity 3 is smaller than the 4 counts"),
                     (dict(total=-1), "rle_strings_emit: total_runs -1 is negative"),          # a refused mask owns no counts: 0 passes
                     (dict(counts=None), "rle_strings_emit: missing operand")):
        assert emit(**kw) == -1, kw
        assert L.mi355det_last_error().decode() == text


def test_cpu_store_keeps_the_host_route():
    """_MaskStore on the CPU: strings go through the host codec (the string wrappers would refuse the device), the arrays are the rules'
    and stay on the CPU."""
    from object_detectors_amd.cocoeval import _MaskStore
    store = _MaskStore(torch.device("cpu"))
    store.add_segmentations(_segs())
    counts, runs, area, bbox, sizes = store.tensors()
    want = [ro.encode(m) for m in MASKS]
    assert all(t.device.type == "cpu" for t in (counts, runs, area, bbox))
    assert counts.dtype == torch.int32 and counts.tolist() == np.concatenate(want).tolist()
    assert runs.tolist() == np.concatenate([[0], np.cumsum([len(c) for c in want])]).tolist()
    assert area.tolist() == [float(m.sum()) for m in MASKS] and bbox.tolist() == [[float(v) for v in ro.bbox(m)] for m in MASKS]
    assert sizes.tolist() == [list(m.shape) for m in MASKS]
    with pytest.raises(ValueError, match="rle_from_string: character"):
        _MaskStore("cpu").add_segmentations([_segs()[0], {"size": [2, 2], "counts": "1!"}])
    with pytest.raises(ValueError, match="COCOEval: run lengths that do not add up to 2x2"):
        _MaskStore("cpu").add_segmentations([{"size": [2, 2], "counts": ro.to_string([1, 2])}])


def test_route_choice_reads_the_form_of_the_input():
    from object_detectors_amd.cocoeval import _counts_strings
    segs = _segs()
    sizes, strings = _counts_strings(segs)
    assert sizes.dtype == np.int32 and sizes.tolist() == [list(m.shape) for m in MASKS] and strings == [s["counts"] for s in segs]
    assert _counts_strings([dict(s, counts=s["counts"].encode()) for s in segs]) is not None
    assert _counts_strings([]) is None
    assert _counts_strings(segs + [{"size": [2, 2], "counts": [1, 3]}]) is None           # a count list among them: the host route
    assert _counts_strings(segs + [MASKS[0]]) is None                                      # a bitmap
    assert _counts_strings([{"size": [2, 2], "counts": "1é"}]) is None                # not ASCII: the host codec refuses it
    assert _counts_strings([{"size": [1 << 16, 1 << 15], "counts": "0"}]) is None and _counts_strings([{"size": [0, 4], "counts": "0"}]) is None
    assert _counts_strings([{"counts": "0"}]) is None


def test_lvis_segm_eval_on_the_host():
    """What LVISSegmEval checks before any device work, and that LVISEval keeps refusing `segm`."""
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    images = [{"id": 1, "height": 4, "width": 4, "neg_category_ids": [], "not_exhaustive_category_ids": []}]
    dataset = {"images": images, "categories": [{"id": 1, "frequency": "f"}],
               "annotations": [{"id": 1, "image_id": 1, "category_id": 1, "area": 8.0, "segmentation": {"size": [4, 4], "counts": [0, 8, 8]}}]}
    with pytest.raises(NotImplementedError, match="LVISSegmEval"):
        LVISEval(dataset, iou_type="segm", device="cpu")
    e = LVISSegmEval(dataset, device="cpu")
    assert e.iou_type == "segm" and e.name == "LVISSegmEval" and e.num_added == 0
    e.add_results([{"image_id": 1, "category_id": 1, "score": 0.5, "segmentation": {"size": [4, 4], "counts": ro.to_string([0, 8, 8])}}])
    assert e.num_added == 1 and e._masks.tensors()[2].tolist() == [8.0] and e._masks.tensors()[3].tolist() == [[0.0, 0.0, 2.0, 4.0]]
    with pytest.raises(ValueError, match="image 1 is 2x8, the image 4x4"):
        e.add_results([{"image_id": 1, "category_id": 1, "score": 0.5, "segmentation": {"size": [2, 8], "counts": ro.to_string([0, 8, 8])}}])
    assert e.num_added == 1
    with pytest.raises(ValueError, match="segmentation"):
        e.add_results([{"image_id": 1, "category_id": 1, "score": 0.5, "bbox": [0, 0, 1, 1]}])
    for field in ("height", "width"):
        broken = dict(dataset, images=[{k: v for k, v in images[0].items() if k != field}])
        with pytest.raises(ValueError, match="image 1 of the ground truth has no height and width"):
            LVISSegmEval(broken, device="cpu")
