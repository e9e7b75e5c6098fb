"""tests/keypoint_rcnn_oracle.py against tests/golden/g18_keypoint_rcnn.npz (the reference's own keypoint functions, recorded by
tools/make_golden_keypoint.py): integer outputs exactly, floats bit for bit or within 1 ulp.  And the sub-pixel form of
ConvTranspose2d(Cin, K, 4, 2, 1) - the oracle's loop and the product's index form - against F.conv_transpose2d in float64.  CPU only."""
import os

import numpy as np
import pytest

from oracle import detrand
from tests import keypoint_rcnn_oracle as ko

torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_keypoint_rcnn.npz")
K, S = 17, 56


@pytest.fixture(scope="module")
def g():
    return dict(np.load(G, allow_pickle=False))


def within_1ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape
    bad = np.abs(a.astype(np.float64) - b.astype(np.float64)) > np.spacing(np.abs(b)).astype(np.float64)
    assert not bad.any(), (int(bad.sum()), a[bad][:4], b[bad][:4])


def _case(g):
    return ([torch.from_numpy(g[f"gt_keypoints{i}"]) for i in range(2)], [torch.from_numpy(g[f"props{i}"]) for i in range(2)],
            [torch.from_numpy(g[f"matched{i}"]) for i in range(2)])


def test_fixture_is_small_and_holds_the_cases(g):
    assert os.path.getsize(G) < 200 * 1024
    assert g["target"].shape == (24, K) and g["valid"].shape == (24, K)
    v = g["valid"]
    assert v[1].sum() == 0 and 0 < v.sum() < v.size                       # a row with none valid; some pairs outside / invisible
    assert g["target"][0, 1] % S == S - 1 and g["target"][0, 2] // S == S - 1          # on the right edge, on the bottom edge


def test_targets(g):
    kps, props, mis = _case(g)
    t, v = ko.keypoint_targets(kps, props, mis, S)
    np.testing.assert_array_equal(t.numpy(), g["target"])
    np.testing.assert_array_equal(v.numpy(), g["valid"])


def test_loss_and_gradient(g):
    kps, props, mis = _case(g)
    logits = torch.from_numpy(detrand.uniform(int(g["seeds"][0]), (24, K, S, S), -4.0, 4.0)).requires_grad_(True)
    loss = ko.keypointrcnn_loss(logits, props, kps, mis)
    loss.backward()
    within_1ulp(loss.detach().numpy(), g["loss"])
    gr = logits.grad.reshape(24 * K, S * S).numpy()
    vflat = g["valid"].reshape(-1).astype(bool)
    assert not gr[~vflat].any()
    within_1ulp(gr[np.arange(24 * K), g["target"].reshape(-1)][vflat], g["grad_at_target"])
    within_1ulp(np.abs(gr[vflat]).max(1), g["grad_absmax"])
    within_1ulp(gr[vflat][np.arange(int(vflat.sum())), g["grad_probe_index"]], g["grad_probe"])
    kp0 = [kps[0].clone()]
    kp0[0][..., 2] = 0
    assert float(ko.keypointrcnn_loss(logits[:14].detach(), props[:1], kp0, mis[:1])) == float(g["loss_all_invalid"]) == 0.0
    assert float(ko.keypointrcnn_loss(torch.zeros((0, K, S, S)), [torch.zeros((0, 4))], kps[:1], [torch.zeros(0, dtype=torch.int64)])) == \
        float(g["loss_r0"]) == 0.0


def test_heatmaps_to_keypoints(g):
    rois = torch.from_numpy(g["h2k_rois"])
    maps = torch.from_numpy(detrand.uniform(int(g["seeds"][1]), (rois.shape[0], K, S, S), -4.0, 4.0))
    xy, sc = ko.heatmaps_to_keypoints(maps, rois)
    within_1ulp(xy.numpy(), g["h2k_xy"])
    within_1ulp(sc.numpy(), g["h2k_scores"])
    assert (g["h2k_xy"][..., 2] == 1).all()
    # the RoI narrower than one pixel: a 1 x 1 map, so every keypoint sits at the box's corner + half the clamped size
    np.testing.assert_array_equal(g["h2k_xy"][0, :, 0], np.float32(0.5) * np.float32(1.0) + g["h2k_rois"][0, 0])


def test_inference_and_postprocess(g):
    boxes = [torch.from_numpy(g[f"det_boxes{i}"]) for i in range(2)]
    x = torch.from_numpy(detrand.uniform(int(g["seeds"][2]), (9, K, S, S), -4.0, 4.0))
    xy, sc = ko.keypointrcnn_inference(x, boxes)
    for i in range(2):
        within_1ulp(xy[i].numpy(), g[f"det_xy{i}"])
        within_1ulp(sc[i].numpy(), g[f"det_scores{i}"])
        post = ko.resize_keypoints(torch.from_numpy(g[f"det_xy{i}"]), tuple(g["det_image_shapes"][i]), tuple(g["det_original_sizes"][i]))
        np.testing.assert_array_equal(post.numpy(), g[f"post_xy{i}"])


def test_resize_and_flip(g):
    for j in range(3):
        h, w, nh, nw = (int(v) for v in g[f"tf_sizes{j}"])
        kp = torch.from_numpy(g[f"tf_in{j}"])
        np.testing.assert_array_equal(ko.resize_keypoints(kp, (h, w), (nh, nw)).numpy(), g[f"tf_resized{j}"])
        fl = ko.flip_coco_person_keypoints(kp.clone(), w)
        np.testing.assert_array_equal(fl.numpy(), g[f"tf_flipped{j}"])
        np.testing.assert_array_equal(ko.resize_keypoints(fl, (h, w), (nh, nw)).numpy(), g[f"tf_flipped_resized{j}"])
        assert not g[f"tf_flipped{j}"][g[f"tf_flipped{j}"][..., 2] == 0].any()
        # the product's host-side rule (tvision/transform.py: resize_keypoints) gives the same bits
        from object_detectors_amd.tvision.transform import resize_keypoints
        np.testing.assert_array_equal(resize_keypoints(kp, (h, w), (nh, nw)).numpy(), g[f"tf_resized{j}"])


@pytest.mark.parametrize("cin,k,kp", [(8, 5, 8), (16, 17, 32)])
def test_subpixel_convolution_equals_conv_transpose(cin, k, kp):
    import torch.nn.functional as F
    from object_detectors_amd.tvision import keypoint_rcnn as kr
    gen = torch.Generator().manual_seed(cin)
    x = torch.randn(2, cin, 14, 14, dtype=torch.float64, generator=gen)
    w = torch.randn(cin, k, 4, 4, dtype=torch.float64, generator=gen)
    b = torch.randn(k, dtype=torch.float64, generator=gen)
    ref = F.conv_transpose2d(x, w, b, stride=2, padding=1)
    w3 = ko.subpixel_weight(w, kp)
    assert int((w3.reshape(4, kp, cin, 9)[:, :k] != 0).any(1).any(1).sum(1).max()) == 4          # four live taps per phase
    b3 = torch.zeros(4, kp, dtype=torch.float64)
    b3[:, :k] = b
    y = ko.depth_to_space(F.conv2d(x, w3, b3.reshape(-1), padding=1), k)
    assert float((y - ref).abs().max()) <= 1e-13
    # the product's index form of the same mapping, its bias, and its inverse for the weight gradient
    assert torch.equal(kr.subpixel_weight(w, kp), w3)
    assert torch.equal(kr.subpixel_bias(b, kp), b3.reshape(-1))
    z = F.conv2d(x, w3, b3.reshape(-1), padding=1).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(kr.depth_to_space(z, k), y)
    g3 = torch.randn(4 * kp, 3, 3, cin, dtype=torch.float64, generator=gen)
    back = kr.subpixel_weight_grad(g3, cin, k)
    # d/dw of sum(w3 * g3) is the live taps of g3 scattered back to [cin, k, 4, 4]
    wl = w.clone().requires_grad_(True)
    (ko.subpixel_weight(wl, kp) * g3.permute(0, 3, 1, 2)).sum().backward()
    assert torch.equal(back, wl.grad)
    # space_to_depth is depth_to_space's inverse on the real channels
    hi = torch.randn(2, k, 28, 28, dtype=torch.float64, generator=gen)
    assert torch.equal(kr.depth_to_space(ko.space_to_depth(hi, kp), k), hi)
