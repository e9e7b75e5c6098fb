"""A slow, literal numpy form of the SSD augmentations on bytes (RandomPhotometricDistort, RandomZoomOut, RandomIoUCrop and
RandomHorizontalFlip of detection/transforms.py:30-239 on PIL images), for the tests of `GeneralizedRCNNTransform.ingest(augment=...)`.
Nothing here imports PIL or the package: the rules are Pillow's 8-bit arithmetic restated (tests/test_oracle_ssd_aug.py holds them against
Pillow where it is installed, and against a table recorded from it where not), and a params record is read by its attributes alone.

    out = augment(img, params)        # img uint8 [H, W, 3]; the canvas is materialised, cropped and flipped: uint8 [new_h, new_w, 3]
"""
import numpy as np


def blend(d, v, f):
    """Image.blend(degenerate, image, f) per byte: d + f * (v - d) with f and the arithmetic in float32, clipped to [0, 255], truncated."""
    d, v = np.asarray(d).astype(np.int32), np.asarray(v).astype(np.int32)
    t = d.astype(np.float32) + np.float32(f) * (v - d).astype(np.float32)
    return np.clip(t, np.float32(0), np.float32(255)).astype(np.uint8)


def luma(rgb):
    """convert("L") of an RGB pixel: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    p = np.asarray(rgb).astype(np.uint32)
    return ((19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 0x8000) >> 16).astype(np.uint8)


def rgb_to_hsv(rgb):
    """convert("HSV") of RGB bytes.  V = max; S = int(255 * (cr / max)) with the quotient in float32; the hue's three quotients
    (max - c) / cr are float32, their combination with the sector constant is float64 and rounded to float32, h / 6 + 1 and its fmod by 1
    are float64 and rounded to float32 once more, and H = int(255 * that)."""
    p = np.asarray(rgb).astype(np.int32)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    mx, mn = p.max(-1), p.min(-1)
    grey = mx == mn
    cr = np.where(grey, 1, mx - mn).astype(np.float32)
    s = cr / np.where(grey, 1, mx).astype(np.float32)
    rc, gc, bc = [((mx - c).astype(np.float32) / cr).astype(np.float64) for c in (r, g, b)]
    h = np.where(r == mx, bc - gc, np.where(g == mx, 2.0 + rc - bc, 4.0 + gc - rc)).astype(np.float32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
    H = np.where(grey, 0, (h.astype(np.float64) * 255.0).astype(np.int32))
    S = np.where(grey, 0, (s.astype(np.float64) * 255.0).astype(np.int32))
    return np.stack([H, S, mx], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    """convert("RGB") of HSV bytes: h = H * 6 / 255, i = floor(h), f = h - i; p, q, t = round(V (1 - s)), round(V (1 - s f)),
    round(V (1 - s (1 - f))) with s = S / 255, all float64; the usual six cases; S == 0 gives grey."""
    p = np.asarray(hsv).astype(np.float64)
    H, S, V = p[..., 0], p[..., 1], p[..., 2]
    h = H * 6.0 / 255.0
    i = np.floor(h)
    f = h - i
    s = S / 255.0
    rnd = lambda x: np.floor(x + 0.5)                      # noqa: E731  (C's round on non-negative values)
    pp, q, t = rnd(V * (1.0 - s)), rnd(V * (1.0 - s * f)), rnd(V * (1.0 - s * (1.0 - f)))
    i = i.astype(np.int32) % 6
    r = np.choose(i, [V, q, pp, pp, t, V])
    g = np.choose(i, [t, V, V, q, pp, pp])
    b = np.choose(i, [pp, pp, t, V, V, q])
    out = np.stack([r, g, b], -1)
    out = np.where((S == 0)[..., None], V[..., None], out)
    return np.clip(out, 0, 255).astype(np.uint8)


def hue_shift(factor):
    """adjust_hue's `np.uint8(hue_factor * 255)`: the float64 product truncated towards zero, modulo 256."""
    return int(float(factor) * 255) & 255


def brightness(img, f):
    return blend(np.zeros_like(img), img, f)


def contrast_degenerate(img):
    """int(mean + 0.5) of L over the whole image, the mean the float64 quotient of the integer sum and h * w."""
    lum = luma(img)
    return int(int(lum.astype(np.int64).sum()) / lum.size + 0.5)


def contrast(img, f):
    return blend(np.full_like(img, contrast_degenerate(img)), img, f)


def saturation(img, f):
    return blend(np.repeat(luma(img)[..., None], 3, -1), img, f)


def hue(img, f):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] += np.uint8(hue_shift(f))                  # wraps modulo 256
    return hsv_to_rgb(hsv)


OPS = {"brightness": brightness, "contrast": contrast, "saturation": saturation, "hue": hue}


def photometric(img, ops, permutation):
    """The ops in order, then the channel permutation (`image[..., permutation, :, :]` between to_tensor and to_pil_image, the identity
    on bytes)."""
    for name, f in ops:
        img = OPS[name](img, f)
    if permutation is not None:
        img = img[..., list(permutation)]
    return img


def augment(img, params):
    """One image through its params record (`ops`, `permutation`, `zoom`, `crop`, `flip`), every stage on bytes."""
    img = photometric(np.ascontiguousarray(img), params.ops, params.permutation)
    if params.zoom is not None:
        canvas_h, canvas_w, left, top, fill = params.zoom
        canvas = np.empty((canvas_h, canvas_w, 3), np.uint8)
        canvas[:] = np.asarray(fill, np.uint8)
        canvas[top:top + img.shape[0], left:left + img.shape[1]] = img
        img = canvas
    if params.crop is not None:
        left, top, new_w, new_h = params.crop
        assert 0 <= left and 0 <= top and left + new_w <= img.shape[1] and top + new_h <= img.shape[0]
        img = img[top:top + new_h, left:left + new_w]
    if params.flip:
        img = img[:, ::-1]
    return img.copy()                                      # a copy: a one-pixel view keeps its negative stride through ascontiguousarray
