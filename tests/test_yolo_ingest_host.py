"""Host side of the YOLO ingest (yolo/dsets/transformations.py: ResizeToTensor, mi355det_yolo_ingest_u8, mi355det_yolo_targets): the tap
tables against the literal rule of tests/cubic_oracle.py, their cache, the refusals (all raised before any launch, so no device is needed),
the C layout of the two structs, the host checks of the C entries and the label maps."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from object_detectors_amd.yolo.dsets import transformations as tr  # noqa: E402
from tests import cubic_oracle as co  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the reference's 80 labels -> COCO's 91 category ids (the values of yolo/dsets/transformations.py:60-68, coco_80_91.json)
COCO_80_91 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41,
              42, 43, 44, 46, 47, 48, 49, 50, 51, 52, 53, 54, 55, 56, 57, 58, 59, 60, 61, 62, 63, 64, 65, 67, 70, 72, 73, 74, 75, 76, 77, 78, 79, 80, 81,
              82, 84, 85, 86, 87, 88, 89, 90]


@pytest.mark.parametrize("dst", [32, 64, 96])
def test_tap_tables_equal_the_literal_rule(dst):
    for src in range(1, 131):
        got = tr.cubic_taps(src, dst)
        want = co.taps(src, dst)
        assert got.dtype == tr.TAP_DTYPE and got.shape == (dst,) and not got.flags.writeable
        assert got["s"].tolist() == [s for s, _ in want], (src, dst)
        assert got["w"].tolist() == [list(w) for _, w in want], (src, dst)


def test_tap_tables_are_cached_per_pair():
    a = tr.cubic_taps(480, 640)
    assert tr.cubic_taps(480, 640) is a and tr.cubic_taps(np.int64(480), 640) is a
    assert tr.cubic_taps(640, 480) is not a and tr.cubic_taps(480, 641) is not a
    with pytest.raises(ValueError):
        tr.cubic_taps(0, 32)


def test_normalised_bytes_are_the_literal_values():
    lut = tr.normalised_bytes()
    assert lut.dtype == torch.float32 and tuple(lut.shape) == (3, 256)
    every = np.arange(256, dtype=np.uint8).reshape(16, 16)
    want = co.literal_image(np.stack([every] * 3, -1))[0]
    assert torch.equal(lut.reshape(3, 16, 16), want)


def _u8(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_refusals_are_raised_on_the_host():
    t = tr.ResizeToTensor(64)
    a, b = _u8(20, 30), _u8(16, 16, 1)
    tg = {"bbox": np.array([[1.0, 2.0, 9.0, 8.0]]), "category_id": [3], "area": [72.0], "image_id": 7}
    with pytest.raises(ValueError, match="empty"):
        t.batch([])
    with pytest.raises(TypeError, match="uint8"):
        t.batch([a, b.float()])
    with pytest.raises(TypeError, match="uint8"):
        t.batch([np.zeros((4, 4, 3), np.int16)])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.batch([a.permute(2, 0, 1)])                            # CHW
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.batch([a[None]])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.batch([a[..., :1]])                                    # a grey image is [H, W]
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.batch([a[:0]])
    with pytest.raises(ValueError, match="all on the CPU or all on one device"):
        t.batch([a, b.to("meta")])
    with pytest.raises(ValueError, match="flips"):
        t.batch([a, b], flips=[True])
    with pytest.raises(ValueError, match="targets"):
        t.batch([a, b], [tg])
    with pytest.raises(ValueError, match=r"shape \[G, 4\]"):
        t.batch([a], [dict(tg, bbox=np.zeros((3, 5)))])
    with pytest.raises(ValueError, match=r"shape \[G, 4\]"):
        t.batch([a], [dict(tg, bbox=np.zeros(4))])
    with pytest.raises(ValueError, match="areas"):
        t.batch([a], [dict(tg, area=[1.0, 2.0])])
    for scale in (0, -32, 41.5):
        with pytest.raises(ValueError, match="scale"):
            tr.ResizeToTensor(scale)
    with pytest.raises(ValueError, match="empty"):               # the per-sample form goes through the same checks
        tr.ResizeToTensor(32).batch(())
    with pytest.raises(TypeError, match="uint8"):
        tr.ResizeToTensor(32)((a.float(), tg))


def test_augment_is_not_built():
    with pytest.raises(NotImplementedError, match="imgaug"):
        tr.Augment()
    with pytest.raises(NotImplementedError, match="imgaug"):
        tr.Augment(num_of_augms=2)


def test_label_maps_match_the_reference():
    m = tr.COCO91_80()
    assert len(COCO_80_91) == 80 and m.data_inv == {v: k for k, v in enumerate(COCO_80_91)}
    ids = torch.tensor([1, 13, 90, 46, 27], dtype=torch.int64)
    img, tg = m(("img", {"category_id": ids, "bbox": "kept"}))
    assert img == "img" and tg["bbox"] == "kept" and tg["category_id"].dtype == torch.int64
    assert tg["category_id"].tolist() == [0, 11, 79, 40, 24]
    with pytest.raises(KeyError):
        m(("img", {"category_id": torch.tensor([12])}))          # 12 is one of the ids COCO never used
    ids = torch.tensor([1, 5, 80], dtype=torch.int64)
    _, tg = tr.Class1_0()(("img", {"category_id": ids}))
    assert tg["category_id"] is ids and ids.tolist() == [0, 4, 79]


def test_shim_registers_the_module():
    import sys
    from object_detectors_amd import shims
    shims.install(torchvision=False)
    try:
        from dsets import transformations
        assert transformations.ResizeToTensor is tr.ResizeToTensor and transformations.COCO91_80 is tr.COCO91_80
    finally:
        shims.uninstall()
    assert "dsets.transformations" not in sys.modules


def test_struct_sizes_match_c():
    """The ctypes mirrors of mi355det_cubic_tap and mi355det_yolo_image, and the numpy dtype of the tap tables, have the C layout."""
    from object_detectors_amd import _lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mi355det.h"
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d\n", sizeof(mi355det_cubic_tap), offsetof(mi355det_cubic_tap, w),
  sizeof(mi355det_yolo_image), offsetof(mi355det_yolo_image, h), offsetof(mi355det_yolo_image, channels), offsetof(mi355det_yolo_image, flip),
  offsetof(mi355det_yolo_image, xtab), offsetof(mi355det_yolo_image, ytab), MI355DET_YOLO_TILE_H, MI355DET_YOLO_TILE_W); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    T, S = _lib.CubicTap, _lib.YoloImage
    assert out == [ctypes.sizeof(T), T.w.offset, ctypes.sizeof(S), S.h.offset, S.channels.offset, S.flip.offset, S.xtab.offset, S.ytab.offset,
                   _lib.YOLO_TILE_H, _lib.YOLO_TILE_W]
    assert ctypes.sizeof(T) == 12 and ctypes.sizeof(S) == 32
    assert tr.TAP_DTYPE.itemsize == 12 and tr.TAP_DTYPE.fields["s"][1] == 0 and tr.TAP_DTYPE.fields["w"][1] == T.w.offset


def test_c_entries_reject_bad_arguments_before_any_launch():
    """The host checks of the new entries return MI355DET_EINVAL (-1) before a launch, so they can be exercised without a device."""
    from object_detectors_amd import _lib, build
    build.build()
    L = _lib.lib()
    dummy = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))        # never read: every call below fails first
    size, n_taps = 32, 96

    def table(n=2, **kw):
        t = (_lib.YoloImage * n)()
        for i in range(n):
            t[i] = _lib.YoloImage(i * 3 * 20 * 30, 20, 30, 3, 0, 0, 32)
            for k, v in kw.items():
                setattr(t[i], k, v)
        return t

    def ingest(t, n=2, nbytes=2 * 3 * 20 * 30, packed=dummy, tab_dev=dummy, taps=dummy, ntaps=n_taps, lut=dummy, out=dummy, size=size):
        return L.mi355det_yolo_ingest_u8(packed, nbytes, None if t is None else ctypes.cast(t, ctypes.c_void_p), tab_dev, n, taps, ntaps, lut, out,
                                         size, None)
    assert ingest(table(), n=0) == -1 and b"n > 0" in L.mi355det_last_error()
    assert ingest(table(), n=-3) == -1
    assert ingest(None) == -1 and b"null" in L.mi355det_last_error()
    for null in ("packed", "tab_dev", "taps", "lut", "out"):
        assert ingest(table(), **{null: None}) == -1 and b"null" in L.mi355det_last_error(), null
    assert ingest(table(), size=0) == -1 and b"size > 0" in L.mi355det_last_error()
    assert ingest(table(), size=-64) == -1
    assert ingest(table(h=0)) == -1 and ingest(table(w=-1)) == -1 and b"sizes" in L.mi355det_last_error()
    assert ingest(table(channels=2)) == -1 and ingest(table(channels=0)) == -1 and b"channels" in L.mi355det_last_error()
    assert ingest(table(), nbytes=2 * 3 * 20 * 30 - 1) == -1 and b"outside" in L.mi355det_last_error()
    assert ingest(table(offset=-1)) == -1 and ingest(table(offset=1 << 40)) == -1
    assert ingest(table(channels=1), nbytes=3 * 20 * 30 + 20 * 30 - 1) == -1        # a grey image is h * w bytes
    assert ingest(table(xtab=-1)) == -1 and b"tap table" in L.mi355det_last_error()
    assert ingest(table(xtab=n_taps - size + 1)) == -1 and ingest(table(ytab=n_taps - size + 1)) == -1 and ingest(table(ytab=-5)) == -1
    assert ingest(table(), ntaps=63) == -1 and ingest(table(), ntaps=0) == -1
    assert ingest(table(ytab=0x7fffffff)) == -1                                      # the sum does not wrap

    def targets(boxes=dummy, area=dummy, g=4, off=dummy, tab=dummy, n=2, bbox=dummy, rel=dummy):
        return L.mi355det_yolo_targets(boxes, area, g, off, tab, n, bbox, rel, None)
    assert targets(n=0) == -1 and targets(g=-1) == -1
    for null in ("boxes", "area", "off", "tab", "bbox", "rel"):
        assert targets(**{null: None}) == -1 and b"null" in L.mi355det_last_error(), null
    assert targets(boxes=None, area=None, bbox=None, rel=None, g=0) == 0               # no boxes: nothing to launch
