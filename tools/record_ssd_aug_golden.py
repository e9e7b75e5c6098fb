"""Record tests/golden/ssd_aug_pillow.npz from Pillow: a few thousand colours through every stage of the SSD photometric chain, so that the
rules of tests/ssd_aug_oracle.py stay pinned where Pillow is not installed (tests/test_oracle_ssd_aug.py reads the file).

    python tools/record_ssd_aug_golden.py

The colours: an 80 x 64 image, 4096 seeded random colours followed by edge cases (greys, primaries, near-greys, and colours whose exact
hue is a whole number, where the order of the roundings in RGB -> HSV shows)."""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "ssd_aug_pillow.npz")
FACTORS = (0.5, 0.875, 1.125, 1.5)
HUES = (-0.05, -0.0123, 0.03, 0.05, 0.5)


def colours():
    rng = np.random.default_rng(20262)
    rand = rng.integers(0, 256, (4096, 3), dtype=np.uint8)
    edge = [(v, v, v) for v in (0, 1, 127, 128, 254, 255)]
    edge += [(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (1, 0, 0), (0, 1, 0), (0, 0, 1), (255, 254, 255)]
    for mx in (6, 12, 60, 120, 240, 255):                   # 255 * (mid - min) / (6 * cr) is a whole number for many of these
        for mn in (0, mx // 2):
            for mid in range(mn, mx + 1, max(1, (mx - mn) // 6)):
                edge += [(mx, mid, mn), (mn, mx, mid), (mid, mn, mx), (mx, mn, mid), (mid, mx, mn), (mn, mid, mx)]
    edge = np.asarray(edge, np.uint8)
    fillers = rng.integers(0, 256, (80 * 64 - 4096 - len(edge), 3), dtype=np.uint8)
    return np.concatenate([rand, edge, fillers]).reshape(80, 64, 3)


def adjust_hue(img, f):
    """torchvision's F_pil.adjust_hue; the shift is np.uint8(f * 255) as numpy 1 casts it: truncated towards zero, modulo 256."""
    h, s, v = img.convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    np_h += np.uint8(int(f * 255) & 255)
    return Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")


def main():
    rgb = colours()
    img = Image.fromarray(rgb, "RGB")
    out = {"rgb": rgb, "pillow": np.array(PIL.__version__), "factors": np.asarray(FACTORS), "hues": np.asarray(HUES),
           "L": np.asarray(img.convert("L")), "hsv": np.asarray(img.convert("HSV")),
           "rgb_of_hsv": np.asarray(Image.fromarray(rgb, "HSV").convert("RGB"))}
    for k, f in enumerate(FACTORS):
        out[f"brightness{k}"] = np.asarray(ImageEnhance.Brightness(img).enhance(f))
        out[f"contrast{k}"] = np.asarray(ImageEnhance.Contrast(img).enhance(f))
        out[f"saturation{k}"] = np.asarray(ImageEnhance.Color(img).enhance(f))
    for k, f in enumerate(HUES):
        out[f"hue{k}"] = np.asarray(adjust_hue(img, f))
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
