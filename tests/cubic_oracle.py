"""OpenCV's 8-bit INTER_CUBIC resize, restated from resize.cpp in a slow literal form (numpy only): the rule of include/mi355det.h
("YOLO ingest") one scalar at a time.  Neither cv2 nor skimage is installed where the tests run, so this restatement is not run against
OpenCV; tests/test_oracle_cubic.py anchors it to torch's float64 bicubic, which shares A, the half-pixel map and the index clamp.

    taps(src, dst)            [(s, (w0, w1, w2, w3))] for every output index of one axis
    resize(img, size)         uint8 [H, W, 3] or [H, W] -> uint8 [size, size, 3] (a grey image is its channel three times)
    resize(img, size, flip)   the same of the image mirrored left to right
    literal_batch / literal_targets   the reference's numpy and torch CPU operations behind the resize (dsets/transformations.py:30-50)

`last_acc_max` is the largest |accumulator| the last `resize` saw; `resize` asserts that it stays inside int32."""
import numpy as np

A = np.float32(-0.75)
COEF_BITS = 11
COEF_SCALE = np.float32(1 << COEF_BITS)
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
last_acc_max = 0


def weights(fx):
    """interpolateCubic: float32, every expression evaluated as written."""
    fx = np.float32(fx)
    one, two, three = np.float32(1), np.float32(2), np.float32(3)
    x1 = np.float32(fx + one)
    c0 = np.float32(np.float32(np.float32(np.float32(np.float32(np.float32(np.float32(A * x1) - np.float32(np.float32(5) * A)) * x1)
                                                     + np.float32(np.float32(8) * A)) * x1)) - np.float32(np.float32(4) * A))
    c1 = np.float32(np.float32(np.float32(np.float32(np.float32(np.float32(A + two) * fx) - np.float32(A + three)) * fx) * fx) + one)
    x2 = np.float32(one - fx)
    c2 = np.float32(np.float32(np.float32(np.float32(np.float32(np.float32(A + two) * x2) - np.float32(A + three)) * x2) * x2) + one)
    c3 = np.float32(np.float32(np.float32(one - c0) - c1) - c2)
    return c0, c1, c2, c3


def fixed(c):
    """saturate_cast<short>(c * 2048): a float32 product, rounded half to even, saturated to int16."""
    v = int(np.rint(np.float32(np.float32(c) * COEF_SCALE)))
    return max(-32768, min(32767, v))


def taps(src, dst):
    scale = 1.0 / (dst / float(src))
    out = []
    for d in range(dst):
        fx = np.float32((d + 0.5) * scale - 0.5)
        s = int(np.floor(fx))
        fx = np.float32(fx - np.float32(s))
        out.append((s, tuple(fixed(c) for c in weights(fx))))
    return out


def resize(img, size, flip=False):
    global last_acc_max
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    if img.ndim == 2:
        img = np.stack([img] * 3, -1)                    # cv2.cvtColor(GRAY2RGB) of the resized plane = the resize of the three planes
    if flip:
        img = img[:, ::-1]
    h, w, _ = img.shape
    src = img.astype(np.int64)
    ty, tx = taps(h, size), taps(w, size)
    out = np.empty((size, size, 3), np.uint8)
    # one output row at a time, all its pixels side by side (int64, so nothing can wrap before the int32 assertion below)
    cols = [np.array([min(max(sx - 1 + k, 0), w - 1) for sx, _ in tx]) for k in range(4)]
    wxs = [np.array([wx[k] for _, wx in tx], np.int64)[:, None] for k in range(4)]
    acc_max = 0
    for y in range(size):
        sy, wy = ty[y]
        rows = [min(max(sy - 1 + k, 0), h - 1) for k in range(4)]
        acc = np.zeros((size, 3), np.int64)
        for ky in range(4):
            hsum = np.zeros((size, 3), np.int64)
            for kx in range(4):
                hsum += wxs[kx] * src[rows[ky], cols[kx]]
            acc += wy[ky] * hsum
        acc_max = max(acc_max, int(np.abs(acc).max()))
        out[y] = np.clip((acc + (1 << (2 * COEF_BITS - 1))) >> (2 * COEF_BITS), 0, 255)      # numpy's >> of int64 is arithmetic
    assert acc_max < 2 ** 31, acc_max
    last_acc_max = acc_max
    return out


def literal_image(resized):
    """transformations.py:31-42 on the resized uint8 [S, S, 3] image: float32 [1, 3, S, S]."""
    import torch
    img = resized.transpose((2, 0, 1))
    img = img / 255.0
    img = torch.from_numpy(img).float()
    mean = torch.tensor([[MEAN]]).permute(2, 1, 0)                    # the reference's `.T` of a [1, 1, 3] tensor
    std = torch.tensor([[STD]]).permute(2, 1, 0)
    img = (img - mean) / std
    return img.unsqueeze(0)


def literal_batch(images, size, flips):
    import torch
    return torch.cat([literal_image(resize(np.asarray(i), size, f)) for i, f in zip(images, flips)])


def literal_targets(shape, target, flip):
    """transformations.py:24-28,44-50 and helper.convert2_rel_xcycwh in float64, with the flip xmin' = w - (xmin + bw) ahead of them."""
    import torch
    h, w = int(shape[0]), int(shape[1])
    img_size = torch.tensor([h, w, 3])
    bbs = torch.tensor(np.asarray(target["bbox"], dtype=np.float64).reshape(-1, 4))
    if flip:
        bbs = bbs.clone()
        bbs[:, 0] = w - (bbs[:, 0] + bbs[:, 2])
    areas = torch.tensor(np.asarray(target["area"], dtype=np.float64).reshape(-1))
    xmin, ymin = bbs[:, 0] / img_size[1], bbs[:, 1] / img_size[0]
    width, height = bbs[:, 2] / img_size[1], bbs[:, 3] / img_size[0]
    xc, yc = xmin + width / 2, ymin + height / 2
    return {"bbox": torch.stack((xc, yc, width, height)).T.float(), "img_size": img_size,
            "category_id": torch.tensor(np.asarray(target["category_id"]), dtype=torch.int64).reshape(-1),
            "area": areas / (img_size[0] * img_size[1]), "image_id": torch.tensor(target["image_id"], dtype=torch.int64)}
