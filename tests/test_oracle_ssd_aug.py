"""The numpy oracle of the SSD augmentations (tests/ssd_aug_oracle.py) against Pillow itself where it is installed, exhaustively where
the domain allows it, and against a table recorded from Pillow (tests/golden/ssd_aug_pillow.npz, tools/record_ssd_aug_golden.py) where not:
the GPU tests compare the kernels with this oracle, so this file is what ties them to the reference's PIL route."""
import os

import numpy as np
import pytest

from tests import ssd_aug_oracle as o

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ssd_aug_pillow.npz")
FACTORS = (0.5, 0.875, 1.0, 1.125, 1.5)


class Params:
    def __init__(self, ops=(), permutation=None, zoom=None, crop=None, flip=False):
        self.ops, self.permutation, self.zoom, self.crop, self.flip = ops, permutation, zoom, crop, flip


def seeded(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


# ---- without Pillow: the recorded table -----------------------------------------------------------------------------------------

def test_golden_table_pins_every_stage():
    g = np.load(GOLDEN)
    rgb = g["rgb"]
    assert rgb.shape == (80, 64, 3) and rgb.dtype == np.uint8
    assert np.array_equal(o.luma(rgb), g["L"])
    assert np.array_equal(o.rgb_to_hsv(rgb), g["hsv"])
    assert np.array_equal(o.hsv_to_rgb(rgb), g["rgb_of_hsv"])
    for k, f in enumerate(g["factors"]):
        assert np.array_equal(o.brightness(rgb, f), g[f"brightness{k}"]), f
        assert np.array_equal(o.contrast(rgb, f), g[f"contrast{k}"]), f
        assert np.array_equal(o.saturation(rgb, f), g[f"saturation{k}"]), f
    for k, f in enumerate(g["hues"]):
        assert np.array_equal(o.hue(rgb, f), g[f"hue{k}"]), f
    assert not np.array_equal(g["hue0"], rgb) and not np.array_equal(g["contrast0"], g["contrast3"])


def test_to_tensor_and_back_is_the_identity_on_bytes():
    """The channel permutation goes through to_tensor and to_pil_image: float32(b) / 255, * 255, truncated, gives b for all 256 bytes."""
    b = np.arange(256, dtype=np.uint8)
    assert np.array_equal(((b.astype(np.float32) / np.float32(255)) * np.float32(255)).astype(np.uint8), b)
    img = seeded(5, 7, 1)
    assert np.array_equal(o.photometric(img, (), (2, 0, 1)), img[..., [2, 0, 1]])


def test_hue_shift_is_truncated_and_wraps():
    assert [o.hue_shift(f) for f in (0.05, -0.05, 0.5, -0.5, 0.0, -0.001)] == [12, 244, 127, 129, 0, 0]


def test_augment_geometry():
    img = seeded(6, 9, 2)
    fill = (123, 117, 104)
    out = o.augment(img, Params(zoom=(12, 20, 4, 3, fill)))
    assert out.shape == (12, 20, 3) and np.array_equal(out[3:9, 4:13], img)
    mask = np.ones((12, 20), bool)
    mask[3:9, 4:13] = False
    assert (out[mask] == np.asarray(fill, np.uint8)).all()
    win = o.augment(img, Params(zoom=(12, 20, 4, 3, fill), crop=(2, 1, 7, 5)))
    assert np.array_equal(win, out[1:6, 2:9])
    assert np.array_equal(o.augment(img, Params(zoom=(12, 20, 4, 3, fill), crop=(2, 1, 7, 5), flip=True)), win[:, ::-1])
    assert np.array_equal(o.augment(img, Params(crop=(1, 2, 3, 4))), img[2:6, 1:4])


# ---- with Pillow ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def pil():
    return pytest.importorskip("PIL.Image")


def test_blend_matches_pillow_for_every_byte_pair(pil):
    v, d = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8))
    for f in FACTORS:
        want = np.asarray(pil.blend(pil.fromarray(d, "L"), pil.fromarray(v, "L"), f))
        assert np.array_equal(o.blend(d, v, f), want), f
    for f in (0.5, 0.875, 1.125, 1.5):                      # brightness: the degenerate is black, floor(v * float32(f)) clipped
        b = np.arange(256)
        assert np.array_equal(o.blend(np.zeros(256, np.uint8), b, f), np.clip(np.floor(b * np.float32(f)), 0, 255).astype(np.uint8))


def test_hsv_conversions_match_pillow_for_every_colour(pil):
    b = np.arange(256, dtype=np.uint8)
    for lo in range(0, 256, 64):                             # the cube in four slabs of 2^22 colours
        cube = np.stack(np.meshgrid(b[lo:lo + 64], b, b, indexing="ij"), -1).reshape(1024, 4096, 3)
        assert np.array_equal(o.rgb_to_hsv(cube), np.asarray(pil.fromarray(cube, "RGB").convert("HSV")))
        assert np.array_equal(o.hsv_to_rgb(cube), np.asarray(pil.fromarray(cube, "HSV").convert("RGB")))


def pil_op(pil, name, img, f):
    """torchvision's F_pil adjust_* on a PIL image."""
    from PIL import ImageEnhance
    if name == "hue":
        h, s, v = img.convert("HSV").split()
        np_h = np.array(h, dtype=np.uint8)
        np_h += np.uint8(int(f * 255) & 255)                # np.uint8(hue_factor * 255) as numpy 1 casts it
        return pil.merge("HSV", (pil.fromarray(np_h, "L"), s, v)).convert("RGB")
    enhancer = {"brightness": ImageEnhance.Brightness, "contrast": ImageEnhance.Contrast, "saturation": ImageEnhance.Color}[name]
    return enhancer(img).enhance(f)


def test_contrast_saturation_brightness_hue_on_seeded_images(pil):
    for seed, (h, w) in enumerate([(37, 53), (64, 40), (1, 7), (120, 150)]):
        img = seeded(h, w, 40 + seed)
        if seed == 2:
            img[:] = [[200, 10, 10]]                         # a mean whose + 0.5 matters less than its truncation
        for name in ("contrast", "saturation", "brightness"):
            for f in FACTORS:
                assert np.array_equal(o.OPS[name](img, f), np.asarray(pil_op(pil, name, pil.fromarray(img, "RGB"), f))), (name, f, seed)
        for f in (-0.05, -0.02, 0.0, 0.013, 0.05):
            assert np.array_equal(o.hue(img, f), np.asarray(pil_op(pil, "hue", pil.fromarray(img, "RGB"), f))), (f, seed)
        from PIL import ImageStat
        assert o.contrast_degenerate(img) == int(ImageStat.Stat(pil.fromarray(img, "RGB").convert("L")).mean[0] + 0.5)


@pytest.mark.parametrize("contrast_first", [True, False])
def test_composed_ssd_chain_matches_pillow(pil, contrast_first):
    from PIL import ImageOps
    img = seeded(48, 60, 77)
    ops = [("brightness", 1.1)] + ([("contrast", 0.7)] if contrast_first else []) + [("saturation", 1.4), ("hue", -0.03)]
    ops += [] if contrast_first else [("contrast", 1.3)]
    p = Params(tuple(ops), (1, 2, 0), (120, 150, 31, 22, (123, 117, 104)), (20, 10, 90, 70), True)
    x = pil.fromarray(img, "RGB")
    for name, f in p.ops:
        x = pil_op(pil, name, x, f)
    x = pil.fromarray(np.ascontiguousarray(np.asarray(x)[..., list(p.permutation)]), "RGB")
    canvas_h, canvas_w, left, top, fill = p.zoom
    x = ImageOps.expand(x, border=(left, top, canvas_w - left - 60, canvas_h - top - 48), fill=fill)       # F.pad(image, [l, t, r, b], fill)
    assert x.size == (canvas_w, canvas_h)
    left, top, new_w, new_h = p.crop
    x = x.crop((left, top, left + new_w, top + new_h))                                                      # F.crop(image, top, left, h, w)
    x = x.transpose(pil.FLIP_LEFT_RIGHT)                                                                    # F.hflip
    assert np.array_equal(o.augment(img, p), np.asarray(x))
