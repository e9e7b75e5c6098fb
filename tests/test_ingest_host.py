"""Host side of the uint8 ingest route (tvision/transform.py:GeneralizedRCNNTransform.ingest, tvision/presets.py): the flip draws, the size and
layout planning, the refusals (all raised before any launch, so no device is needed) and the C layout of the image table."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from object_detectors_amd.tvision.presets import DetectionPresetEval, DetectionPresetTrain  # noqa: E402
from object_detectors_amd.tvision.transform import GeneralizedRCNNTransform, ImageList, plan_ingest, resized_size  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(37, 53), (64, 40), (50, 50), (120, 150), (33, 97), (1, 7)]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def test_flip_draws_follow_the_reference_sequence():
    for seed in (0, 5, 1234):
        torch.manual_seed(seed)
        got = DetectionPresetTrain("hflip", 0.5).draw(7)
        torch.manual_seed(seed)
        assert got == [bool(torch.rand(1) < 0.5) for _ in range(7)]
    assert any(got) and not all(got)
    torch.manual_seed(3)
    assert DetectionPresetTrain("hflip", 0.0).draw(4) == [False] * 4 and DetectionPresetTrain("hflip", 1.0).draw(4) == [True] * 4
    state = torch.get_rng_state()
    assert DetectionPresetEval().draw(5) == [False] * 5
    assert torch.equal(torch.get_rng_state(), state)            # evaluation draws nothing


def test_preset_policies():
    for policy in ("ssd", "ssdlite"):
        with pytest.raises(NotImplementedError, match="SSD"):
            DetectionPresetTrain(policy)
    with pytest.raises(ValueError, match='Unknown data augmentation policy "mosaic"'):
        DetectionPresetTrain("mosaic")
    assert DetectionPresetTrain().hflip_prob == 0.5


def test_plan_ingest_sizes_pad_offsets_tiles():
    plan = plan_ingest(SHAPES, 64, 96, 32)
    assert plan.sizes == [(64, 91), (96, 60), (63, 63), (64, 80), (32, 95), (13, 96)]       # (50, 50) -> 63: the float32 scale
    assert plan.pad == (96, 96)
    assert plan.offsets == [int(v) for v in np.concatenate([[0], np.cumsum([3 * h * w for h, w in SHAPES])[:-1]])]
    assert plan.nbytes == sum(3 * h * w for h, w in SHAPES)
    assert plan.first_tile[0] == 0 and all(b > a for a, b in zip(plan.first_tile, plan.first_tile[1:] + [plan.tiles]))
    from object_detectors_amd import _lib
    per_image = -(-96 // _lib.INGEST_TILE_H) * -(-96 // _lib.INGEST_TILE_W)
    assert plan.tiles == len(SHAPES) * per_image and plan.first_tile == [i * per_image for i in range(len(SHAPES))]
    # one min size per image (the training draws), a fixed size, and a pad that no image fills
    per = plan_ingest(SHAPES[:2], [48, 64], 96, 32)
    assert per.sizes == [resized_size(37, 53, 48.0, 96.0), resized_size(64, 40, 64.0, 96.0)] and per.sizes[1] == (96, 60) and per.pad == (96, 96)
    assert plan_ingest(SHAPES, 64, 96, 32, fixed_size=(80, 40)).sizes == [(40, 80)] * 6
    assert plan_ingest([(8, 8)], 40, 96, 32).pad == (64, 64)        # 8 * (1/8 * 40) = 40 exactly, rounded up to the next 32
    with pytest.raises(ValueError):
        plan_ingest(SHAPES, [64, 64], 96, 32)


def _u8(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_ingest_refusals_are_raised_on_the_host():
    t = GeneralizedRCNNTransform(64, 96, MEAN, STD)
    t.eval()
    a, b = _u8(20, 30), _u8(16, 16, 1)
    boxes = torch.tensor([[1.0, 2.0, 9.0, 8.0]])
    with pytest.raises(ValueError, match="empty"):
        t.ingest([])
    with pytest.raises(TypeError, match="uint8"):
        t.ingest([a, b.float()])
    with pytest.raises(TypeError, match="uint8"):
        t.ingest([np.zeros((4, 4, 3), np.int16)])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.ingest([a.permute(2, 0, 1)])                           # CHW
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.ingest([a[None]])
    with pytest.raises(ValueError, match=r"\[H, W, 3\]"):
        t.ingest([a[..., :1]])                                   # grayscale
    with pytest.raises(ValueError, match="all on the CPU or all on one device"):
        t.ingest([a, b.to("meta")])
    with pytest.raises(ValueError, match="flips"):
        t.ingest([a, b], flips=[True])
    with pytest.raises(ValueError, match="targets"):
        t.ingest([a, b], [{"boxes": boxes}])
    with pytest.raises(ValueError, match=r"shape \[N, 4\]"):
        t.ingest([a], [{"boxes": torch.zeros(3, 5)}])
    with pytest.raises(ValueError, match=r"shape \[N, 4\]"):
        t.ingest([a], [{"boxes": torch.zeros(4)}])
    with pytest.raises(ValueError, match="masks"):
        t.ingest([a], [{"boxes": boxes, "masks": torch.zeros(1, 30, 20, dtype=torch.uint8)}])
    with pytest.raises(ValueError, match="keypoints"):
        t.ingest([a], [{"boxes": boxes, "keypoints": torch.zeros(1, 17, 3)}])
    with pytest.raises(TypeError):                               # the float route keeps refusing uint8, and the new one floats
        t([a.permute(2, 0, 1)])


def test_image_list_keeps_the_original_sizes():
    il = ImageList(torch.zeros(1, 3, 32, 32), [(20, 30)])
    assert il.original_image_sizes is None and il.to("cpu").original_image_sizes is None
    il = ImageList(torch.zeros(1, 3, 32, 32), [(20, 30)], [(10, 15)])
    assert il.to("cpu").original_image_sizes == [(10, 15)] and il.to("cpu").image_sizes == [(20, 30)]


def test_c_entries_reject_bad_arguments_before_any_launch():
    """The host checks of the new entries return MI355DET_EINVAL (-1) before a launch, so they can be exercised without a device."""
    from object_detectors_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert L.mi355det_ingest_tiles(96, 96) == plan_ingest(SHAPES, 64, 96, 32).first_tile[1] and L.mi355det_ingest_tiles(0, 96) == 0
    assert L.mi355det_ingest_tiles(800, 1344) == 50 * 21
    dummy = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))        # never read: every call below fails first
    tiles = L.mi355det_ingest_tiles(96, 96)

    def table(n=2, **kw):
        t = (_lib.IngestImage * n)()
        for i in range(n):
            t[i] = _lib.IngestImage(i * 3 * 20 * 30, 20, 30, 64, 96, 0, i * tiles)
            for k, v in kw.items():
                setattr(t[i], k, v)
        return t

    def ingest(t, n=2, nbytes=2 * 3 * 20 * 30, tab_dev=dummy, ph=96, pw=96):
        return L.mi355det_ingest_u8(dummy, nbytes, None if t is None else ctypes.cast(t, ctypes.c_void_p), tab_dev, n, dummy, dummy, dummy, ph, pw,
                                    None)
    assert ingest(table(), n=0) == -1 and b"n > 0" in L.mi355det_last_error()
    assert ingest(None) == -1 and ingest(table(), tab_dev=None) == -1
    assert ingest(table(), ph=32) == -1 and b"pad < out" in L.mi355det_last_error()
    assert ingest(table(), pw=64) == -1
    assert ingest(table(h=0)) == -1 and ingest(table(out_w=0)) == -1
    assert ingest(table(), nbytes=2 * 3 * 20 * 30 - 1) == -1 and b"outside" in L.mi355det_last_error()
    assert ingest(table(offset=-1)) == -1
    assert ingest(table(first_tile=0)) == -1 and b"first_tile" in L.mi355det_last_error()
    assert L.mi355det_flip_resize_boxes(dummy, dummy, 4, dummy, dummy, 0, None) == -1
    assert L.mi355det_flip_resize_boxes(dummy, dummy, 4, None, dummy, 2, None) == -1
    assert L.mi355det_flip_resize_boxes(dummy, dummy, 4, dummy, None, 2, None) == -1
    assert L.mi355det_flip_resize_boxes(dummy, dummy, -1, dummy, dummy, 2, None) == -1
    assert L.mi355det_flip_resize_boxes(None, None, 0, dummy, dummy, 2, None) == 0          # no boxes: nothing to launch
    assert L.mi355det_mask_flip_resize_nearest(dummy, 1, 0, 5, dummy, 4, 4, 1, None) == -1
    assert L.mi355det_mask_flip_resize_nearest(None, 0, 5, 5, None, 4, 4, 1, None) == 0


def test_table_struct_matches_c():
    """The ctypes mirror of mi355det_ingest_image has the C layout (a tiny gcc program, as tests/test_abi.py does for the other structs)."""
    from object_detectors_amd import _lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mi355det.h"
int main(void){ printf("%zu %zu %zu %zu %zu %d %d\n", sizeof(mi355det_ingest_image), offsetof(mi355det_ingest_image, h),
  offsetof(mi355det_ingest_image, out_h), offsetof(mi355det_ingest_image, flip), offsetof(mi355det_ingest_image, first_tile),
  MI355DET_INGEST_TILE_H, MI355DET_INGEST_TILE_W); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    S = _lib.IngestImage
    assert out == [ctypes.sizeof(S), S.h.offset, S.out_h.offset, S.flip.offset, S.first_tile.offset, _lib.INGEST_TILE_H, _lib.INGEST_TILE_W]
    assert ctypes.sizeof(S) == 32
