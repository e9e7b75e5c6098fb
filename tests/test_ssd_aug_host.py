"""Host side of the SSD augmentations (tvision/transforms.py, GeneralizedRCNNTransform.ingest(augment=...)): the draws against a literal
per-sample loop in the order of detection/transforms.py, the refusals (all raised before any launch, so no device is needed), the EINVAL
returns of the C entries and the C layout of the two new tables."""
import ctypes
import os
import subprocess
import tempfile

import pytest

torch = pytest.importorskip("torch")

from object_detectors_amd.tvision import transforms as T  # noqa: E402  (absent before this feature: every test of this file fails there)
from object_detectors_amd.tvision.transform import GeneralizedRCNNTransform  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the last is (4, 7), not the (1, 7) of the GPU tests: `new_w / new_h` of transforms.py:93 divides by int(1 * r) = 0 on an image one row
# high, in the reference and so in its mirror (test_draw_on_an_image_too_small_for_a_crop)
SHAPES = [(37, 53), (64, 40), (50, 50), (120, 150), (33, 97), (4, 7)]
COUNTS = [3, 0, 1, 5, 2, 1]
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
OPTIONS = [0.0, 0.1, 0.3, 0.5, 0.7, 0.9, 1.0]


def random_targets(seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for (h, w), k in zip(SHAPES, COUNTS):
        a, b = torch.rand(k, 2, generator=g) * 0.6, 0.05 + torch.rand(k, 2, generator=g) * 0.35
        out.append({"boxes": torch.cat([a, a + b], 1) * torch.tensor([w, h, w, h], dtype=torch.float32), "labels": torch.arange(k) + 1})
    return out


def jitter(lo, hi):
    torch.randperm(4)
    return float(torch.empty(1).uniform_(lo, hi))


def literal_sample(policy, h, w, boxes, labels, hflip_prob=0.5):
    """One sample through the reference's Compose, in this test's own words: every draw and every box operation of
    detection/transforms.py:190-239, 132-187, 54-129 and 30-37 in their order, the pixels left out."""
    ops, perm, zoom, crop = [], None, None, None
    if policy == "ssd":
        r = torch.rand(7)
        if r[0] < 0.5:
            ops.append(("brightness", jitter(0.875, 1.125)))
        before = r[1] < 0.5
        if before and r[2] < 0.5:
            ops.append(("contrast", jitter(0.5, 1.5)))
        if r[3] < 0.5:
            ops.append(("saturation", jitter(0.5, 1.5)))
        if r[4] < 0.5:
            ops.append(("hue", jitter(-0.05, 0.05)))
        if not before and r[5] < 0.5:
            ops.append(("contrast", jitter(0.5, 1.5)))
        if r[6] < 0.5:
            perm = tuple(torch.randperm(3).tolist())
        if not (torch.rand(1) < 0.5):
            r = 1.0 + torch.rand(1) * 3.0
            cw, ch = int(w * r), int(h * r)
            r = torch.rand(2)
            left, top = int((cw - w) * r[0]), int((ch - h) * r[1])
            boxes[:, 0::2] += left
            boxes[:, 1::2] += top
            zoom = (ch, cw, left, top, (123, 117, 104))
            h, w = ch, cw
    done = False
    while not done:
        lo = OPTIONS[int(torch.randint(low=0, high=7, size=(1,)))]
        if lo >= 1.0:
            break
        for _ in range(40):
            r = 0.3 + 0.7 * torch.rand(2)
            nw, nh = int(w * r[0]), int(h * r[1])
            if not (0.5 <= nw / nh <= 2.0):
                continue
            r = torch.rand(2)
            left, top = int((w - nw) * r[0]), int((h - nh) * r[1])
            right, bottom = left + nw, top + nh
            if left == right or top == bottom:
                continue
            cx, cy = 0.5 * (boxes[:, 0] + boxes[:, 2]), 0.5 * (boxes[:, 1] + boxes[:, 3])
            inside = (left < cx) & (cx < right) & (top < cy) & (cy < bottom)
            if not inside.any():
                continue
            b = boxes[inside]
            win = torch.tensor([[left, top, right, bottom]], dtype=b.dtype)
            wh = (torch.min(b[:, None, 2:], win[:, 2:]) - torch.max(b[:, None, :2], win[:, :2])).clamp(min=0)
            inter = wh[:, :, 0] * wh[:, :, 1]
            area_b, area_w = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]), (win[:, 2] - win[:, 0]) * (win[:, 3] - win[:, 1])
            if (inter / (area_b[:, None] + area_w - inter)).max() < lo:
                continue
            boxes, labels = b, labels[inside]
            boxes[:, 0::2] -= left
            boxes[:, 1::2] -= top
            boxes[:, 0::2].clamp_(min=0, max=nw)
            boxes[:, 1::2].clamp_(min=0, max=nh)
            crop = (left, top, nw, nh)
            done = True
            break
    flip = bool(torch.rand(1) < hflip_prob)
    return (tuple(ops), perm, zoom, crop, flip), boxes, labels


@pytest.mark.parametrize("policy", ["ssd", "ssdlite"])
@pytest.mark.parametrize("seed", [0, 5, 1234])
def test_draw_follows_the_reference_sequence(policy, seed):
    targets = random_targets(seed + 1)
    before = [t["boxes"].clone() for t in targets]
    torch.manual_seed(seed)
    params, out = T.SSDAugmentation(policy).draw(SHAPES, targets)
    state = torch.get_rng_state()
    torch.manual_seed(seed)
    want = [literal_sample(policy, h, w, t["boxes"].clone(), t["labels"].clone()) for (h, w), t in zip(SHAPES, targets)]
    assert torch.equal(torch.get_rng_state(), state)
    for p, t, (dec, boxes, labels), (h, w), src, orig in zip(params, out, want, SHAPES, targets, before):
        assert (p.ops, p.permutation, p.zoom, p.crop, p.flip) == dec
        assert t["boxes"].dtype == torch.float32 and torch.equal(t["boxes"], boxes) and torch.equal(t["labels"], labels)
        assert torch.equal(src["boxes"], orig) and t["boxes"] is not src["boxes"] and t is not src           # the caller's are untouched
        wh, ww = p.window(h, w)
        if t["boxes"].numel():
            assert float(t["boxes"][:, 0::2].max()) <= ww and float(t["boxes"][:, 1::2].max()) <= wh and float(t["boxes"].min()) >= 0
        if policy == "ssdlite":
            assert p.ops == () and p.permutation is None and p.zoom is None


def test_draws_cover_every_decision():
    """Over a few seeds every kind of decision occurs, so the comparison above is not one of empty records."""
    seen = set()
    for seed in (0, 5, 1234):
        torch.manual_seed(seed)
        for p in T.SSDAugmentation("ssd").draw(SHAPES, random_targets(seed + 1))[0]:
            seen.update(name for name, _f in p.ops)
            names = [name for name, _f in p.ops]
            if "contrast" in names:
                seen.add("contrast first" if names.index("contrast") < len(names) - 1 and names[-1] != "contrast" else "contrast last")
            seen.update(k for k in ("permutation", "zoom", "crop") if getattr(p, k) is not None)
            seen.add("flip" if p.flip else "no flip")
            assert len(p.ops) <= 5 and names.count("contrast") <= 1
    assert {"brightness", "contrast", "saturation", "hue", "permutation", "zoom", "crop", "flip", "no flip"} <= seen


def test_draw_refusals():
    aug = T.SSDAugmentation("ssd")
    boxes = torch.tensor([[1.0, 2.0, 9.0, 8.0]])
    state = torch.get_rng_state()
    with pytest.raises(ValueError, match="targets can't be None"):
        aug.draw([(20, 30)], None)
    with pytest.raises(ValueError, match="targets for"):
        aug.draw([(20, 30), (16, 16)], [{"boxes": boxes}])
    with pytest.raises(ValueError, match="masks"):
        aug.draw([(20, 30)], [{"boxes": boxes, "masks": torch.zeros(1, 20, 30, dtype=torch.uint8)}])
    with pytest.raises(ValueError, match="keypoints"):
        aug.draw([(20, 30)], [{"boxes": boxes, "keypoints": torch.zeros(1, 17, 3)}])
    with pytest.raises(ValueError, match=r"shape \[N, 4\]"):
        aug.draw([(20, 30)], [{"boxes": torch.zeros(3, 5)}])
    with pytest.raises(ValueError, match=r"shape \[N, 4\]"):
        aug.draw([(20, 30)], [{"boxes": torch.zeros(4)}])
    with pytest.raises(ValueError, match=r"shape \[N, 4\]"):
        aug.draw([(20, 30)], [{"labels": torch.zeros(1)}])
    assert torch.equal(torch.get_rng_state(), state)            # a refusal draws nothing
    with pytest.raises(ValueError, match="Unknown SSD data augmentation policy"):
        T.SSDAugmentation("hflip")
    with pytest.raises(ValueError, match="side range"):
        T.RandomZoomOut(side_range=(0.5, 2.0))


def test_draw_on_an_image_too_small_for_a_crop():
    """The reference's crop divides by a height of zero on an image fewer than four rows high unless it draws leave-as-is first; the mirror
    does what it does."""
    torch.manual_seed(0)
    with pytest.raises(ZeroDivisionError):
        for _ in range(20):
            T.SSDAugmentation("ssdlite").draw([(1, 7)], [{"boxes": torch.tensor([[1.0, 0.0, 3.0, 1.0]])}])


def test_box_iou_restated():
    a = torch.tensor([[0.0, 0.0, 10.0, 10.0], [5.0, 5.0, 15.0, 15.0], [20.0, 20.0, 30.0, 30.0]])
    b = torch.tensor([[0.0, 0.0, 10.0, 10.0]])
    assert torch.equal(T.box_iou(a, b), torch.tensor([[1.0], [25.0 / 175.0], [0.0]]))


def _u8(h, w, seed=0):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def test_ingest_augment_refusals_are_raised_on_the_host():
    t = GeneralizedRCNNTransform(64, 96, MEAN, STD)
    t.eval()
    a = _u8(20, 30)
    boxes = torch.tensor([[1.0, 2.0, 9.0, 8.0]])
    P = T.AugmentParams
    with pytest.raises(ValueError, match="flips must be None"):
        t.ingest([a], augment=[P()], flips=[False])
    with pytest.raises(ValueError, match="augment records"):
        t.ingest([a], augment=[P(), P()])
    with pytest.raises(ValueError, match="masks"):
        t.ingest([a], [{"boxes": boxes, "masks": torch.zeros(1, 20, 30, dtype=torch.uint8)}], augment=[P()])
    with pytest.raises(ValueError, match="canvas"):
        t.ingest([a], augment=[P(zoom=(40, 60, 31, 0, (1, 2, 3)))])              # 31 + 30 > 60
    with pytest.raises(ValueError, match="canvas"):
        t.ingest([a], augment=[P(zoom=(19, 60, 0, 0, (1, 2, 3)))])
    with pytest.raises(ValueError, match="three bytes"):
        t.ingest([a], augment=[P(zoom=(40, 60, 0, 0, (1, 2, 300)))])
    with pytest.raises(ValueError, match="crop"):
        t.ingest([a], augment=[P(crop=(25, 0, 10, 10))])                         # 25 + 10 > 30 without a canvas
    with pytest.raises(ValueError, match="crop"):
        t.ingest([a], augment=[P(crop=(0, 0, 0, 10))])
    with pytest.raises(ValueError, match="permutation"):
        t.ingest([a], augment=[P(permutation=(0, 0, 1))])
    with pytest.raises(ValueError, match="one contrast"):
        t.ingest([a], augment=[P(ops=(("contrast", 1.0), ("contrast", 1.1)))])
    with pytest.raises(ValueError, match="at most 5"):
        t.ingest([a], augment=[P(ops=(("brightness", 1.0),) * 6)])
    with pytest.raises(ValueError, match="unknown photometric op"):
        t.ingest([a], augment=[P(ops=(("sharpness", 1.0),))])
    with pytest.raises(ValueError, match="hue factor"):
        t.ingest([a], augment=[P(ops=(("hue", 0.6),))])
    with pytest.raises(ValueError, match="negative or not finite"):
        t.ingest([a], augment=[P(ops=(("brightness", -0.1),))])
    with pytest.raises(ValueError, match="those `draw` returned"):
        t.ingest([a], [{"boxes": boxes}], augment=[P(crop=(0, 0, 8, 8))])        # a box that was not cropped


def test_c_entries_reject_bad_arguments_before_any_launch():
    from object_detectors_amd import _lib, build
    build.build()
    L = _lib.lib()
    assert L.mi355det_photo_blocks(1) == 1 and L.mi355det_photo_blocks(_lib.PHOTO_BLOCK_PIXELS + 1) == 2 and L.mi355det_photo_blocks(0) == 0
    dummy = ctypes.c_void_p(ctypes.addressof(ctypes.create_string_buffer(64)))        # never read: every call below fails first
    tiles = L.mi355det_ingest_tiles(96, 96)

    def table(n=2, **kw):
        t = (_lib.IngestAugImage * n)()
        for i in range(n):
            t[i] = _lib.IngestAugImage(i * 3 * 20 * 30, 20, 30, 40, 60, 5, 7, 2, 3, 30, 45, 64, 96, 0, i * tiles, 0x68757B, 0)
            for k, v in kw.items():
                setattr(t[i], k, v)
        return t

    def ingest(t, n=2, nbytes=2 * 3 * 20 * 30, tab_dev=dummy, ph=96, pw=96):
        return L.mi355det_ingest_aug_u8(dummy, nbytes, None if t is None else ctypes.cast(t, ctypes.c_void_p), tab_dev, n, dummy, dummy, dummy, ph,
                                        pw, None)
    assert ingest(table(), n=0) == -1 and b"n > 0" in L.mi355det_last_error()
    assert ingest(None) == -1 and ingest(table(), tab_dev=None) == -1
    assert ingest(table(), ph=32) == -1 and b"pad < out" in L.mi355det_last_error()
    assert ingest(table(h=0)) == -1 and ingest(table(out_w=0)) == -1
    assert ingest(table(), nbytes=2 * 3 * 20 * 30 - 1) == -1 and b"outside" in L.mi355det_last_error()
    assert ingest(table(offset=-1)) == -1
    assert ingest(table(first_tile=0)) == -1 and b"first_tile" in L.mi355det_last_error()
    for kw in ({"paste_top": 21}, {"paste_left": 31}, {"paste_top": -1}, {"paste_left": -1}, {"canvas_h": 24}, {"canvas_w": 36}):
        assert ingest(table(**kw)) == -1 and b"pasted image lies outside" in L.mi355det_last_error(), kw
    for kw in ({"crop_top": 11}, {"crop_left": 16}, {"crop_top": -1}, {"crop_left": -1}, {"crop_h": 39}, {"crop_w": 58}):
        assert ingest(table(**kw)) == -1 and b"crop lies outside" in L.mi355det_last_error(), kw
    for kw in ({"crop_h": 0}, {"crop_w": 0}, {"crop_w": -3}):
        assert ingest(table(**kw)) == -1 and b"zero side" in L.mi355det_last_error(), kw

    def photo(m=2, **kw):
        t = (_lib.PhotoImage * m)()
        for i in range(m):
            t[i] = _lib.PhotoImage(i * 3 * 20 * 30, 20 * 30, i, 2, (ctypes.c_int32 * 5)(1, 4, 0, 0, 0), (ctypes.c_float * 5)(1.1, 12.0, 0, 0, 0),
                                   (ctypes.c_int32 * 3)(0, 1, 2), 0)
            for k, v in kw.items():
                setattr(t[i], k, v)
        return t

    def distort(t, m=2, nbytes=2 * 3 * 20 * 30, tab_dev=dummy, sums=dummy, packed=dummy):
        return L.mi355det_photometric_u8(packed, nbytes, None if t is None else ctypes.cast(t, ctypes.c_void_p), tab_dev, m, sums, None)
    assert distort(photo(), m=0) == -1 and b"m > 0" in L.mi355det_last_error()
    assert distort(None) == -1 and distort(photo(), tab_dev=None) == -1 and distort(photo(), sums=None) == -1 and distort(photo(), packed=None) == -1
    assert distort(photo(), nbytes=2 * 3 * 20 * 30 - 1) == -1 and b"outside" in L.mi355det_last_error()
    assert distort(photo(pixels=0)) == -1 and distort(photo(offset=-3)) == -1
    assert distort(photo(n_ops=6)) == -1 and distort(photo(n_ops=-1)) == -1
    for codes in ((0, 4, 0, 0, 0), (1, 5, 0, 0, 0), (-1, 1, 0, 0, 0)):
        assert distort(photo(op=(ctypes.c_int32 * 5)(*codes))) == -1 and b"op code" in L.mi355det_last_error(), codes
    assert distort(photo(op=(ctypes.c_int32 * 5)(2, 2, 0, 0, 0))) == -1 and b"more than one contrast" in L.mi355det_last_error()
    assert distort(photo(factor=(ctypes.c_float * 5)(1.1, 12.5, 0, 0, 0))) == -1 and b"hue" in L.mi355det_last_error()
    assert distort(photo(factor=(ctypes.c_float * 5)(1.1, 256.0, 0, 0, 0))) == -1
    assert distort(photo(factor=(ctypes.c_float * 5)(-0.5, 12.0, 0, 0, 0))) == -1 and b"negative" in L.mi355det_last_error()
    assert distort(photo(factor=(ctypes.c_float * 5)(float("nan"), 12.0, 0, 0, 0))) == -1
    assert distort(photo(perm=(ctypes.c_int32 * 3)(0, 1, 1))) == -1 and b"permutation" in L.mi355det_last_error()
    assert distort(photo(perm=(ctypes.c_int32 * 3)(0, 1, 3))) == -1
    assert distort(photo(first_block=0)) == -1 and b"first_block" in L.mi355det_last_error()


def test_table_structs_match_c():
    """The ctypes mirrors of mi355det_ingest_aug_image and mi355det_photo_image have the C layout (a tiny gcc program, as
    tests/test_ingest_host.py does for mi355det_ingest_image, which keeps its 32 bytes)."""
    from object_detectors_amd import _lib
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "mi355det.h"
#define A mi355det_ingest_aug_image
#define P mi355det_photo_image
int main(void){ printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(A), offsetof(A, h), offsetof(A, canvas_h), offsetof(A, paste_top),
  offsetof(A, crop_top), offsetof(A, crop_h), offsetof(A, out_h), offsetof(A, flip), offsetof(A, first_tile), offsetof(A, fill_rgb),
  sizeof(mi355det_ingest_image));
  printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d\n", sizeof(P), offsetof(P, pixels), offsetof(P, first_block), offsetof(P, n_ops),
  offsetof(P, op), offsetof(P, factor), offsetof(P, perm), MI355DET_PHOTO_MAX_OPS, MI355DET_PHOTO_BLOCK_PIXELS, MI355DET_PHOTO_BRIGHTNESS,
  MI355DET_PHOTO_CONTRAST, MI355DET_PHOTO_SATURATION, MI355DET_PHOTO_HUE); return 0; }'''
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        with open(c, "w") as f:
            f.write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        a, p = [[int(v) for v in line.split()] for line in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()]
    A, P = _lib.IngestAugImage, _lib.PhotoImage
    assert a == [ctypes.sizeof(A), A.h.offset, A.canvas_h.offset, A.paste_top.offset, A.crop_top.offset, A.crop_h.offset, A.out_h.offset,
                 A.flip.offset, A.first_tile.offset, A.fill_rgb.offset, 32]
    assert p == [ctypes.sizeof(P), P.pixels.offset, P.first_block.offset, P.n_ops.offset, P.op.offset, P.factor.offset, P.perm.offset,
                 _lib.PHOTO_MAX_OPS, _lib.PHOTO_BLOCK_PIXELS] + [_lib.PHOTO_OPS[k] for k in ("brightness", "contrast", "saturation", "hue")]
    assert ctypes.sizeof(A) % 8 == 0 and ctypes.sizeof(P) % 8 == 0              # tables follow each other in one upload
