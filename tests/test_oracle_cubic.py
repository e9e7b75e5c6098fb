"""tests/cubic_oracle.py (OpenCV's 8-bit INTER_CUBIC rule, restated) against torch's CPU float64 F.interpolate(mode="bicubic",
align_corners=False) of the same bytes.  Torch's float bicubic has the same A = -0.75, the same half-pixel map and the same index clamp, so
it anchors everything but the last bit: the 11-bit weights and the one rounding at the end.

"float" below is torch's result clamped to [0, 255], as the rule's last step clamps: a bicubic overshoots the byte range on hard edges, and
the unclamped difference would measure that overshoot, not the rule."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

from tests import cubic_oracle as co  # noqa: E402

CASES = [((37, 53), 64), ((64, 40), 32), ((50, 50), 96), ((120, 150), 64), ((33, 97), 32), ((1, 7), 32), ((64, 64), 64)]


def image(shape, kind, seed):
    h, w = shape
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    ramp = [255.0 * (x + y) / max(h + w - 2, 1), 255.0 * x / max(w - 1, 1), 255.0 - 255.0 * y / max(h, 1)]
    return np.stack(ramp, -1).round().astype(np.uint8)


def float_bicubic(img, size):
    x = torch.from_numpy(img.astype(np.float64)).permute(2, 0, 1)[None]
    out = F.interpolate(x, size=(size, size), mode="bicubic", align_corners=False)[0].permute(1, 2, 0).numpy()
    return np.clip(out, 0.0, 255.0)


@pytest.fixture(scope="module")
def results():
    out = {}
    for i, (shape, size) in enumerate(CASES):
        for kind in ("random", "ramp"):
            img = image(shape, kind, 100 + i)
            got = co.resize(img, size)
            out[shape, size, kind] = (img, got, float_bicubic(img, size), co.last_acc_max)
    return out


@pytest.mark.parametrize("kind", ["random", "ramp"])
@pytest.mark.parametrize("shape,size", CASES)
def test_within_one_step_of_the_float_bicubic(results, shape, size, kind):
    _img, got, ref, acc_max = results[shape, size, kind]
    assert got.dtype == np.uint8 and got.shape == (size, size, 3)
    diff = np.abs(got.astype(np.int64) - np.round(ref).astype(np.int64))
    print(shape, size, kind, "max |oracle - round(float)|", int(diff.max()), "share differing", float((diff != 0).mean()),
          "max |oracle - float|", float(np.abs(got - ref).max()), "max |acc|", acc_max)
    assert diff.max() <= 1
    assert np.abs(got.astype(np.float64) - ref).max() < 1.0
    assert (diff != 0).mean() <= 0.08
    assert acc_max < 2 ** 31                                          # the accumulators stay inside int32


@pytest.mark.parametrize("kind", ["random", "ramp"])
def test_same_size_is_the_identity(results, kind):
    img, got, _ref, _ = results[(64, 64), 64, kind]
    assert np.array_equal(got, img)
    assert all(t == (d, (0, 2048, 0, 0)) for d, t in enumerate(co.taps(64, 64)))


@pytest.mark.parametrize("kind", ["random", "ramp"])
def test_dyadic_weights_are_exact(results, kind):
    """(64, 40) -> 32: the fractions are 1/2 down and odd eighths across, every weight is a multiple of 1/2048, so the integer sum is the
    float64 sum exactly and only the rule's own rounding (add half, shift: half up) is left."""
    _img, got, ref, _ = results[(64, 40), 32, kind]
    for src in (64, 40):
        assert all(sum(w) == 2048 for _, w in co.taps(src, 32))
    assert np.array_equal(got, np.floor(ref + 0.5).astype(np.uint8))


def test_accumulator_bound():
    """The assertion inside `resize` is live: the worst the weights allow is below 2^31, and a grid of the two extreme bytes gets near it."""
    worst = max(sum(abs(v) for v in w) for src, dst in ((5, 64), (7, 96), (100, 32)) for _, w in co.taps(src, dst))
    assert worst * worst * 255 < 2 ** 31
    img = (255 * ((np.add.outer(np.arange(40), np.arange(44)) // 2) % 2)).astype(np.uint8)
    co.resize(img, 96)
    assert 255 * 2048 * 2048 <= co.last_acc_max < 2 ** 31


def test_hand_worked_row():
    """Source row [0, 255] to width 4 (scale 1/2): fractions 0.75, 0.25, 0.75, 0.25 at s = -1, 0, 0, 1.
    fx = 0.25: c = (-0.10546875, 0.87890625, 0.26171875, -0.03515625) -> w = (-216, 1800, 536, -72); fx = 0.75 is its mirror."""
    lo, hi = (-216, 1800, 536, -72), (-72, 536, 1800, -216)
    assert co.taps(2, 4) == [(-1, hi), (0, lo), (0, hi), (1, lo)]
    src = [0, 255]
    clamped = [[0, 0, 0, 1], [0, 0, 1, 1], [0, 0, 1, 1], [0, 1, 1, 1]]                # s - 1 .. s + 2, clamped to [0, 1]
    hsum = [sum(wk * src[c] for wk, c in zip(w, cols)) for (_, w), cols in zip(co.taps(2, 4), clamped)]
    assert hsum == [-216 * 255, (536 - 72) * 255, (1800 - 216) * 255, (1800 + 536 - 72) * 255]
    # one source row: every vertical tap is row 0 and the vertical weights sum to 2048 (fractions in eighths)
    assert all(sum(w) == 2048 for _, w in co.taps(1, 4))
    want = [min(max((2048 * v + (1 << 21)) >> 22, 0), 255) for v in hsum]
    assert want == [0, 58, 197, 255]
    got = co.resize(np.array([[0, 255]], np.uint8), 4)
    assert got.shape == (4, 4, 3) and all(got[y, :, c].tolist() == want for y in range(4) for c in range(3))


def test_grey_and_flip():
    img = image((9, 13), "random", 7)
    assert np.array_equal(co.resize(img[..., 0], 16), np.repeat(co.resize(img, 16)[..., :1], 3, -1))
    assert np.array_equal(co.resize(img, 16, flip=True), co.resize(np.ascontiguousarray(img[:, ::-1]), 16))
