"""The SSD augmentations on the GPU (GeneralizedRCNNTransform.ingest(augment=...): mi355det_photometric_u8, mi355det_ingest_aug_u8,
mi355det_flip_resize_boxes) against the literal route they must equal bit for bit: the images augmented on bytes by the numpy oracle
(tests/ssd_aug_oracle.py, held against Pillow by tests/test_oracle_ssd_aug.py), ToTensor's division and the flip of the boxes done on the
CPU, then `transform(list, targets)`, as tests/test_gpu_ingest.py does for the flips."""
import numpy as np
import pytest

from tests import ssd_aug_oracle as o

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
SHAPES = [(37, 53), (64, 40), (50, 50), (120, 150), (33, 97), (1, 7)]
FILL = (123, 117, 104)


def P(**kw):
    from object_detectors_amd.tvision.transforms import AugmentParams
    return AugmentParams(**kw)


def transform(min_size=64, max_size=96, **kw):
    from object_detectors_amd.tvision.transform import GeneralizedRCNNTransform
    t = GeneralizedRCNNTransform(min_size, max_size, MEAN, STD, **kw)
    t.eval()
    return t


@pytest.fixture(scope="module")
def images():
    g = torch.Generator().manual_seed(20263)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in SHAPES]


def window_boxes(windows, seed, count=3):
    """Boxes in each window's frame, as `draw` returns them: not yet flipped."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in windows:
        a, b = torch.rand(count, 2, generator=g) * 0.6, 0.05 + torch.rand(count, 2, generator=g) * 0.35
        out.append(torch.cat([a, a + b], 1) * torch.tensor([w, h, w, h], dtype=torch.float32))
    return out


def check(t, images, params, boxes=None):
    """ingest(augment=params) against the float route on the oracle's augmented images; returns the batch."""
    windows = [p.window(*img.shape[:2]) for p, img in zip(params, images)]
    if boxes is None:
        boxes = window_boxes(windows, 11)
    targets = [{"boxes": b, "labels": torch.arange(b.shape[0])} for b in boxes]
    il, tg = t.ingest(images, targets, augment=params)
    literal = [o.augment(img.numpy(), p) for img, p in zip(images, params)]
    assert [a.shape[:2] for a in literal] == windows
    floats = [torch.from_numpy(a).permute(2, 0, 1).float().div(255).contiguous().to(DEV) for a in literal]
    ref_targets = []
    for b, p, (_h, w) in zip(boxes, params, windows):
        b = b.clone()
        if p.flip:
            b[:, [0, 2]] = w - b[:, [2, 0]]                 # detection/transforms.py:37 with the window's width
        ref_targets.append({"boxes": b.to(DEV)})
    ref, rtg = t(floats, ref_targets)
    assert il.tensors.shape == ref.tensors.shape and list(il.image_sizes) == list(ref.image_sizes)
    assert il.original_image_sizes == windows
    for i in range(len(images)):
        assert torch.equal(il.tensors[i], ref.tensors[i]), i
        assert torch.equal(tg[i]["boxes"], rtg[i]["boxes"]), i
        assert tg[i]["labels"] is targets[i]["labels"] and targets[i]["boxes"] is boxes[i]
    return il.tensors


def test_each_photometric_op_alone(images):
    ops = [("brightness", 1.1), ("contrast", 0.6), ("saturation", 1.4), ("hue", 0.04), ("hue", -0.05), ("contrast", 1.45)]
    got = check(transform(), images, [P(ops=(op,)) for op in ops])
    plain = transform().ingest(images)[0].tensors
    assert all(not torch.equal(a, b) for a, b in zip(got, plain))                  # every op changed its image
    check(transform(), images, [P(ops=(op,)) for op in ops[3:] + ops[:3]])        # every image meets another op; (120, 150) has 5 blocks


def test_full_chains_permutation_and_saturating_factors(images):
    before = (("brightness", 0.9), ("contrast", 1.3), ("saturation", 0.6), ("hue", -0.031))
    after = (("brightness", 1.12), ("saturation", 1.5), ("hue", 0.05), ("contrast", 0.55))
    params = [P(ops=before, permutation=(2, 0, 1)), P(ops=after), P(permutation=(1, 0, 2)), P(ops=after, permutation=(1, 2, 0)),
              P(ops=(("brightness", 2.5), ("contrast", 1.5), ("saturation", 1.5))),      # most bytes end at 0 or 255
              P(ops=(("brightness", 0.0), ("contrast", 1.5)))]                           # black: the mean is 0
    check(transform(), images, params)
    sat = o.photometric(images[4].numpy(), params[4].ops, None)
    assert ((sat == 255) | (sat == 0)).mean() > 0.5 and (sat == 255).mean() > 0.1 and (sat == 0).mean() > 0.1


def geometry(kind, h, w, flip):
    """Explicit zoom-out and crop of an [h, w] image.  The canvas is four times the image with the image pasted at (h, w), so that a
    window of the image's size can be shifted by half an image to every side."""
    zoom = (4 * h, 4 * w, w, h, FILL)
    sy, sx = max(1, h // 2), max(1, w // 2)
    crop = {"zoom4": None,
            "left": (w - sx, h, w, h), "right": (w + sx, h, w, h), "top": (w, h - sy, w, h), "bottom": (w, h + sy, w, h),
            "corner": (w - sx, h - sy, w, h),
            "around": (w - 1, h - 1, w + 2, h + 2),                    # one pixel of fill on every side
            "fill_only": (2 * w + 1, 2 * h + 1, w, h),
            "one_pixel": (w + w // 2, h + h // 2, 1, 1),
            "one_fill_pixel": (0, 0, 1, 1),
            "crop_only": (w // 4, h // 4, max(1, w // 2), max(1, h // 2))}[kind]
    return P(zoom=None if kind == "crop_only" else zoom, crop=crop, flip=flip)


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("kind", ["zoom4", "left", "right", "top", "bottom", "corner", "around", "fill_only", "one_pixel", "one_fill_pixel",
                                  "crop_only"])
def test_zoom_out_crop_and_flip(images, kind, flip):
    got = check(transform(), images, [geometry(kind, h, w, flip) for h, w in SHAPES])
    if kind in ("fill_only", "one_fill_pixel"):              # nothing but the fill colour, normalised; at (0, 0) one tap has weight 1
        want = ((torch.tensor(FILL, dtype=torch.float32) / 255 - torch.tensor(MEAN)) / torch.tensor(STD)).to(DEV)
        assert all(torch.equal(got[i, :, 0, 0], want) for i in range(len(SHAPES)))


def test_pad_width_that_is_no_multiple_of_four(images):
    """size_divisible = 1: dword stores instead of 16-byte ones, for windows that straddle the fill and a full chain."""
    t = transform(size_divisible=1)
    params = [geometry("corner", 37, 53, True), geometry("right", 50, 50, False), geometry("crop_only", 120, 150, True)]
    params[0].ops, params[0].permutation = (("brightness", 1.1), ("contrast", 0.8), ("hue", 0.02)), (2, 1, 0)
    got = check(t, [images[0], images[2], images[3]], params)
    assert got.shape[-1] % 4 != 0


def test_identity_params_equal_the_plain_route(images):
    t = transform()
    boxes = window_boxes(SHAPES, 12)
    targets = [{"boxes": b} for b in boxes]
    il, tg = t.ingest(images, targets, augment=[P() for _ in images])
    ref, rtg = t.ingest(images, targets)
    assert torch.equal(il.tensors, ref.tensors) and il.image_sizes == ref.image_sizes and il.original_image_sizes == SHAPES
    assert all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(tg, rtg))
    flips = [True, False, True, False, True, True]
    il, tg = t.ingest(images, targets, augment=[P(flip=f) for f in flips])
    ref, rtg = t.ingest(images, targets, flips)
    assert torch.equal(il.tensors, ref.tensors) and all(torch.equal(a["boxes"], b["boxes"]) for a, b in zip(tg, rtg))
    il, tg = t.ingest(images, augment=[P() for _ in images])                       # no targets at all
    assert tg is None and torch.equal(il.tensors, t.ingest(images)[0].tensors)


def test_two_calls_in_a_row_and_device_images(images):
    """The photometric pass works in place on the call's own packed copy: a second call, and images that live on the device, give the same
    bits, and the device images are left as they were."""
    t = transform()
    chain = (("brightness", 1.1), ("contrast", 0.7), ("saturation", 1.3), ("hue", 0.03))
    params = [P(ops=chain, permutation=(1, 2, 0), zoom=geometry("left", h, w, False).zoom, crop=geometry("left", h, w, False).crop, flip=i % 2 == 0)
              for i, (h, w) in enumerate(SHAPES)]
    first = t.ingest(images, augment=params)[0].tensors
    second = t.ingest(images, augment=params)[0].tensors
    on_dev = [u.to(DEV) for u in images]
    third = t.ingest(on_dev, augment=params)[0].tensors
    one = t.ingest(on_dev[:1], augment=params[:1])[0].tensors                      # a batch of one: the packed buffer is still a copy
    assert torch.equal(first, second) and torch.equal(first, third)
    assert torch.equal(one[0], first[0, :, :one.shape[2], :one.shape[3]])
    assert all(torch.equal(a.cpu(), b) for a, b in zip(on_dev, images))
    check(t, images, params)


@pytest.mark.parametrize("seed", [0, 5, 1234])
def test_drawn_ssd_batch(images, seed):
    """One batch as `SSDAugmentation("ssd").draw` decides it.  Without the (1, 7) image: the reference's crop divides by a height of zero
    on it (tests/test_ssd_aug_host.py)."""
    from object_detectors_amd.tvision.transforms import SSDAugmentation
    shapes = SHAPES[:5]
    source = [{"boxes": b, "labels": torch.arange(3) + 1} for b in window_boxes(shapes, 13 + seed)]
    torch.manual_seed(seed)
    params, targets = SSDAugmentation("ssd").draw(shapes, source)
    check(transform(), images[:5], params, [t["boxes"] for t in targets])
    assert all(t["labels"].shape[0] == t["boxes"].shape[0] for t in targets)


def test_retinanet_trains_on_an_augmented_batch():
    from object_detectors_amd.tvision.retinanet import retinanet_resnet50_fpn
    from oracle import retina_oracle as ro
    m = retinanet_resnet50_fpn(num_classes=91, device=torch.device(DEV), min_size=160, max_size=256)
    m.load_state_dict(ro.det_state(7000))
    m.train()
    m.transform.eval()                                       # one min size: nothing to draw
    g = torch.Generator().manual_seed(8400)
    shapes = [(120, 150), (200, 100)]
    imgs = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in shapes]
    chain = (("brightness", 1.05), ("saturation", 1.2), ("hue", -0.02), ("contrast", 0.8))
    params = [P(ops=chain, permutation=(2, 0, 1), zoom=(240, 300, 60, 50, FILL), crop=(30, 20, 200, 170), flip=True), P(crop=(10, 40, 80, 120))]
    targets = [{"boxes": torch.tensor([[40.0, 35.0, 150.0, 140.0]]), "labels": torch.tensor([5])},
               {"boxes": torch.tensor([[5.0, 10.0, 70.0, 100.0], [20.0, 30.0, 60.0, 90.0]]), "labels": torch.tensor([7, 9])}]
    il, tg = m.transform.ingest(imgs, targets, augment=params)
    assert il.original_image_sizes == [(170, 200), (120, 80)]
    out = m(il, [{"boxes": t["boxes"], "labels": t["labels"].to(DEV)} for t in tg])
    assert set(out.keys()) == {"classification", "bbox_regression"} and all(bool(torch.isfinite(v)) for v in out.values())
