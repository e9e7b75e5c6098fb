"""CPU: the restatement in tests/mask_oracle.py reproduces the reference's own mask-branch functions (tests/golden/g16_maskrcnn.npz, written by
tools/make_golden_mask.py) exactly or to 1e-6, and the nearest / bilinear index rules agree with torch's CPU F.interpolate."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import mask_oracle as mo
from object_detectors_amd.tvision.transform import resized_size

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_maskrcnn.npz")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(G, allow_pickle=False))


def _logits(g):
    seed, k = (int(v) for v in g["logits_seed_k"])
    r = sum(g[f"props{i}"].shape[0] for i in range(3))
    return np.random.default_rng(seed).normal(0, 2, (r, k, 28, 28)).astype(np.float32)


def test_targets_match_reference(g):
    t = np.concatenate([mo.project_masks_on_boxes(g[f"gt_masks{i}"], g[f"props{i}"], g[f"matched{i}"]) for i in range(3)])
    np.testing.assert_array_equal(t, g["targets"])


def test_loss_and_gradient_match_reference(g):
    labels = np.concatenate([g[f"gt_labels{i}"][g[f"matched{i}"]] for i in range(3)])
    loss, grad = mo.maskrcnn_loss(_logits(g), labels, g["targets"])
    assert abs(loss - float(g["loss"])) <= 1e-6 * max(1.0, abs(float(g["loss"])))
    np.testing.assert_allclose(grad[np.arange(len(labels)), labels], g["grad_label"], rtol=0, atol=1e-9)


def test_loss_r0(g):
    loss, grad = mo.maskrcnn_loss(np.zeros((0, 7, 28, 28), np.float32), np.zeros(0, np.int64), np.zeros((0, 28, 28), np.float32))
    assert loss == float(g["loss_r0"]) == 0.0


def test_inference_probs(g):
    x = np.random.default_rng(int(g["det_logits_seed"][0])).normal(0, 2, (9, 7, 28, 28)).astype(np.float32)
    lab = np.concatenate([g["det_labels0"], g["det_labels1"]])
    p = torch.sigmoid(torch.from_numpy(x))[torch.arange(9), torch.from_numpy(lab)][:, None].numpy()
    np.testing.assert_array_equal(p[:5], g["det_probs0"])
    np.testing.assert_array_equal(p[5:], g["det_probs1"])


def test_expand_boxes(g):
    assert float(g["expand_scale"]) == 30.0 / 28.0
    np.testing.assert_array_equal(mo.expand_boxes(g["paste_boxes"], float(g["expand_scale"])), g["expand_boxes"])


def test_paste_matches_reference(g):
    out = mo.paste_masks_in_image(g["paste_masks"], g["paste_boxes"], (32, 40))
    np.testing.assert_allclose(out, g["paste_out"], rtol=0, atol=1e-6)


def test_postprocess_paste_matches_reference(g):
    from object_detectors_amd.tvision import transform  # noqa: F401  (resize_boxes there is a GPU kernel; the scaling is restated here)
    for i, (im_s, o_s) in enumerate([((48, 64), (96, 128)), ((40, 36), (50, 45))]):
        b = g[f"det_boxes{i}"]
        rh, rw = np.float32(o_s[0]) / np.float32(im_s[0]), np.float32(o_s[1]) / np.float32(im_s[1])
        ob = np.stack([b[:, 0] * rw, b[:, 1] * rh, b[:, 2] * rw, b[:, 3] * rh], 1).astype(np.float32)
        np.testing.assert_array_equal(ob, g[f"post_boxes{i}"])
        out = mo.paste_masks_in_image(g[f"det_probs{i}"], ob, o_s)
        np.testing.assert_allclose(out, g[f"post_masks{i}"], rtol=0, atol=1e-6)


def test_resize_masks_matches_reference(g):
    for j in range(4):
        m = g[f"resize_in{j}"]
        mn, mx = (float(v) for v in g[f"resize_minmax{j}"])
        size = resized_size(m.shape[1], m.shape[2], mn, mx)
        np.testing.assert_array_equal(mo.resize_masks_nearest(m, size), g[f"resize_out{j}"])


@pytest.mark.parametrize("hw,out", [((28, 28), (13, 17)), ((30, 30), (1, 1)), ((30, 30), (97, 61)), ((7, 9), (14, 18)), ((30, 30), (30, 45))])
def test_bilinear_rule_matches_torch(hw, out):
    m = np.random.default_rng(hw[0] * 100 + out[0]).uniform(0, 1, hw).astype(np.float32)
    ref = F.interpolate(torch.from_numpy(m)[None, None], size=out, mode="bilinear", align_corners=False)[0, 0].numpy()
    np.testing.assert_allclose(mo.resize_bilinear(m, *out), ref, rtol=0, atol=1e-6)


@pytest.mark.parametrize("hw,out", [((40, 56), (81, 113)), ((33, 47), (20, 28)), ((50, 50), (100, 100)), ((64, 30), (64, 30)), ((17, 13), (800, 612))])
def test_nearest_rule_matches_torch(hw, out):
    m = mo.synth_masks(7, 2, *hw)
    ref = F.interpolate(torch.from_numpy(m)[:, None].float(), size=out)[:, 0].byte().numpy()
    np.testing.assert_array_equal(mo.resize_masks_nearest(m, out), ref)
