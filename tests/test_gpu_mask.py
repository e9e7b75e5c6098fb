"""Mask-branch kernels (csrc/mask_kernels.hip and the deconvolution on the conv kernels) against tests/mask_oracle.py and torch CPU, on the
g16 cases (tests/golden/g16_maskrcnn.npz, the reference's own outputs) and at 800-px sizes.
Bars: pooling and nearest resize bit-equal; targets equal to the reference (same float32 operation order); paste within 1e-6; the deconvolution
within 4e-3 of each value (+ 4e-3 of the mean magnitude: one bf16 rounding of the output is 2e-3 relative); loss to 1e-5 relative; the
fixed-order gradients bit-identical from run to run."""
import os

import numpy as np
import pytest

from tests import mask_oracle as mo

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_maskrcnn.npz")


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(G, allow_pickle=False))


def bf(t):
    return t.to(torch.bfloat16)


def close_of_value(a, b, tol=4e-3):
    a, b = a.double().cpu(), b.double().cpu()
    bound = tol * b.abs() + tol * float(b.abs().mean()) + 1e-12
    bad = ((a - b).abs() > bound).sum().item()
    assert bad == 0, (bad, float((a - b).abs().max()), float(b.abs().max()))


def _pyramid(n, img, seed):
    gen = torch.Generator().manual_seed(seed)
    return [bf(torch.randn(n, img // s, img // s, 256, generator=gen)).to(dev()) for s in (4, 8, 16, 32)]


def _rois(n, img, k, seed, sub_pixel=4):
    rng = np.random.default_rng(seed)
    x1, y1 = rng.uniform(-20, img, k), rng.uniform(-20, img, k)
    w, h = rng.uniform(1, img * 0.7, k), rng.uniform(1, img * 0.7, k)
    w[:sub_pixel], h[:sub_pixel] = rng.uniform(0.05, 0.9, sub_pixel), rng.uniform(0.05, 0.9, sub_pixel)
    r = np.stack([rng.integers(0, n, k), x1, y1, x1 + w, y1 + h], 1).astype(np.float32)
    return torch.from_numpy(r).to(dev())


@pytest.mark.parametrize("n,img,k", [(2, 128, 37), (4, 800, 512)])
def test_roi_pool_bit_equal_to_roi_align_nhwc(n, img, k):
    from object_detectors_amd import ops
    feats = _pyramid(n, img, 5 + img)
    rois = _rois(n, img, k, 11 + img)
    scales, kmin, kmax = [0.25, 0.125, 0.0625, 0.03125], 2, 5
    out = ops.mask_roi_pool(feats, rois, scales, kmin, kmax)
    ref = ops.roi_align_nhwc(feats, rois, 14, scales, 2, False, kmin, kmax)
    ref = bf(ref.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    # pitched output: the same values in a wider buffer
    wide = torch.zeros((k, 14, 14, 320), device=dev(), dtype=torch.bfloat16)
    ops.mask_roi_pool(feats, rois, scales, kmin, kmax, out=wide[..., :256])
    assert torch.equal(wide[..., :256].view(torch.int16), out.view(torch.int16)) and not wide[..., 256:].any()
    # backward: the same scatter as roi_align_nhwc's (fp32 atomics: order-dependent rounding only)
    grad = bf(torch.randn(k, 14, 14, 256, generator=torch.Generator().manual_seed(3))).to(dev())
    dfs = ops.mask_roi_pool_bwd(feats, rois, scales, kmin, kmax, grad)
    rfs = ops.roi_align_nhwc(feats, rois, 14, scales, 2, False, kmin, kmax, grad_out=grad.float().permute(0, 3, 1, 2).contiguous())
    for a, b in zip(dfs, rfs):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)
    # rows >= num_rois are skipped
    part = ops.mask_roi_pool_bwd(feats, rois, scales, kmin, kmax, grad, num_rois=k // 2)
    rpart = ops.mask_roi_pool_bwd(feats, rois[:k // 2].contiguous(), scales, kmin, kmax, grad[:k // 2].contiguous())
    for a, b in zip(part, rpart):
        torch.testing.assert_close(a, b, rtol=1e-5, atol=1e-5)


def _deconv_pack(seed):
    from object_detectors_amd.tvision.mask_rcnn import MaskRCNNPredictor
    torch.manual_seed(seed)
    pr = MaskRCNNPredictor(256, 256, 5).to(dev())
    with torch.no_grad():
        pr.conv5_mask.bias.uniform_(-0.2, 0.2)
    return pr


def _d2s(z):
    """sub-pixel [R, 14, 14, 4*256] -> NCHW [R, 256, 28, 28]."""
    r = z.shape[0]
    return z.reshape(r, 14, 14, 2, 2, 256).permute(0, 5, 1, 3, 2, 4).reshape(r, 256, 28, 28)


@pytest.mark.parametrize("rows", [32, 512])
def test_deconv_forward_dgrad_wgrad(rows):
    from object_detectors_amd import ops
    pr = _deconv_pack(1)
    gen = torch.Generator().manual_seed(rows)
    x = bf(torch.relu(torch.randn(rows, 14, 14, 256, generator=gen))).to(dev())
    wf, wd, b = pr._pack.get(pr.conv5_mask.weight, pr.conv5_mask.bias)
    shape = ops.conv_shape(rows, 14, 14, 256, 1024, 1, 1)
    z = torch.empty((rows, 14, 14, 1024), device=dev(), dtype=torch.bfloat16)
    ops.conv_fwd_ex(shape, x, wf, z, shift=b, relu=True)
    wt = bf(pr.conv5_mask.weight.detach()).float().cpu()
    xc = x.float().cpu().permute(0, 3, 1, 2)
    ref = torch.relu(torch.nn.functional.conv_transpose2d(xc.double(), wt.double(), pr.conv5_mask.bias.detach().cpu().double(), stride=2))
    close_of_value(_d2s(z.float().cpu()), ref)
    # data gradient with the ReLU of the layer below folded in
    dz = bf(torch.randn(rows, 14, 14, 1024, generator=gen) * 1e-3).to(dev())
    dx = torch.empty_like(x)
    ops.conv_dgrad_mask(shape, dz, wd, dx, x)
    dzn = _d2s(dz.float().cpu()).double()
    refdx = torch.nn.functional.conv2d(dzn, wt.double(), stride=2) * (xc > 0)       # the adjoint of conv_transpose2d
    close_of_value(dx.float().cpu().permute(0, 3, 1, 2), refdx)
    # weight gradient: fixed order, bit-identical from run to run
    dws = []
    for _ in range(2):
        dw = torch.zeros((1024, 256), device=dev(), dtype=torch.float32)
        ops.conv_wgrad(shape, x, dz, dw)
        dws.append(dw)
    assert torch.equal(dws[0], dws[1])
    dwt = dws[0].reshape(2, 2, 256, 256).permute(3, 2, 0, 1).cpu().double()
    xu = xc.double()
    refw = torch.zeros(256, 256, 2, 2, dtype=torch.float64)
    for di in range(2):
        for dj in range(2):
            refw[:, :, di, dj] = torch.einsum("rchw,rohw->co", xu, dzn[:, :, di::2, dj::2])
    torch.testing.assert_close(dwt, refw, rtol=2e-3, atol=2e-3 * float(refw.abs().max()))


def _loss_case(rows, valid, k, seed, targets=None):
    gen = torch.Generator().manual_seed(seed)
    feat = bf(torch.relu(torch.randn(rows, 14, 14, 1024, generator=gen)))
    w = torch.randn(k, 256, generator=gen) * 0.05
    b = torch.randn(k, generator=gen) * 0.1
    lab = torch.randint(1, k, (rows,), generator=gen)
    if targets is None:
        targets = (torch.rand(rows, 28, 28, generator=gen) > 0.5).float()
    return feat, w, b, lab, targets


def _loss_cpu(feat, w, b, lab, targets, valid):
    f = feat[:valid].double().clone().requires_grad_(True)
    wd, bd = w.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    l = lab[:valid]
    logit = (f.reshape(valid, 14, 14, 4, 256) * wd[l][:, None, None, None, :]).sum(-1) + bd[l][:, None, None, None]
    logit = logit.reshape(valid, 14, 14, 2, 2).permute(0, 1, 3, 2, 4).reshape(valid, 28, 28)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logit, targets[:valid].double())
    loss.backward()
    return float(loss.detach()), f.grad * (f > 0), wd.grad, bd.grad


@pytest.mark.parametrize("rows,k,use_g16", [(24, 7, True), (512, 91, False)])
def test_loss_and_gradients(g, rows, k, use_g16):
    from object_detectors_amd import ops
    tg = torch.from_numpy(g["targets"]) if use_g16 else None
    feat, w, b, lab, targets = _loss_case(rows, rows, k, 40 + rows, tg)
    outs = [ops.mask_loss(feat.to(dev()), w.to(dev()), b.to(dev()), lab.to(dev()), targets.to(dev()), rows) for _ in range(2)]
    loss, dz, dw, db, dbd = outs[0]
    rl, rdf, rdw, rdb = _loss_cpu(feat, w, b, lab, targets, rows)
    assert abs(float(loss) - rl) <= 1e-5 * abs(rl)
    close_of_value(dz.float().cpu(), rdf, 8e-3)
    torch.testing.assert_close(dw.cpu().double(), rdw, rtol=1e-4, atol=1e-4 * float(rdw.abs().max()))
    torch.testing.assert_close(db.cpu().double(), rdb, rtol=1e-4, atol=1e-4 * float(rdb.abs().max()))
    refbd = dz.float().cpu().double().reshape(rows, 196, 4, 256).sum((0, 1, 2))
    torch.testing.assert_close(dbd.cpu().double(), refbd, rtol=1e-4, atol=1e-4 * float(refbd.abs().max()))
    for a, c in zip(outs[0], outs[1]):                     # fixed-order: bit-identical from run to run
        assert torch.equal(a, c)


def test_loss_r0_and_padded_bucket():
    from object_detectors_amd import ops
    feat, w, b, lab, targets = _loss_case(64, 40, 9, 77)
    args = [t.to(dev()) for t in (feat, w, b, lab, targets)]
    loss, dz, dw, db, dbd = ops.mask_loss(*args, 0)
    assert float(loss) == 0.0 and not dw.any() and not db.any() and not dbd.any() and not dz.any()
    full = ops.mask_loss(*args, 40)
    cut = ops.mask_loss(*[t[:40].contiguous() if t.shape[0] == 64 else t for t in args], 40)
    for a, c in zip((full[0], full[2], full[3], full[4]), (cut[0], cut[2], cut[3], cut[4])):
        assert torch.equal(a, c)
    assert torch.equal(full[1][:40], cut[1]) and not full[1][40:].any()


def test_probs():
    from object_detectors_amd import ops
    feat, w, b, lab, _t = _loss_case(33, 33, 6, 5)
    p = ops.mask_probs(feat.to(dev()), w.to(dev()), b.to(dev()), lab.to(dev()))
    logit = (feat.double().reshape(33, 14, 14, 4, 256) * w.double()[lab][:, None, None, None]).sum(-1) + b.double()[lab][:, None, None, None]
    ref = torch.sigmoid(logit.reshape(33, 14, 14, 2, 2).permute(0, 1, 3, 2, 4).reshape(33, 28, 28))
    torch.testing.assert_close(p.cpu().double(), ref, rtol=0, atol=2e-6)


def test_targets_g16(g):
    from object_detectors_amd import ops
    rois = np.concatenate([np.concatenate([np.full((g[f"props{i}"].shape[0], 1), i, np.float32), g[f"props{i}"]], 1) for i in range(3)])
    gi = np.concatenate([g[f"matched{i}"] for i in range(3)])
    t = ops.mask_targets([torch.from_numpy(g[f"gt_masks{i}"]).to(dev()) for i in range(3)], torch.from_numpy(rois).to(dev()),
                         torch.from_numpy(gi).to(dev()))
    np.testing.assert_array_equal(t.cpu().numpy(), g["targets"])


def test_targets_800px():
    from object_detectors_amd import ops
    masks = [mo.synth_masks(900 + i, 3, 800, 1088 - 64 * i) for i in range(2)]
    rng = np.random.default_rng(9)
    rois, gi = [], []
    for i in range(2):
        for _ in range(3):
            x1, y1 = rng.uniform(-30, 900), rng.uniform(-30, 700)
            rois.append([i, x1, y1, x1 + rng.uniform(20, 160), y1 + rng.uniform(20, 160)])
            gi.append(rng.integers(0, 3))
    rois, gi = np.array(rois, np.float32), np.array(gi, np.int64)
    t = ops.mask_targets([torch.from_numpy(m).to(dev()) for m in masks], torch.from_numpy(rois).to(dev()), torch.from_numpy(gi).to(dev()))
    ref = np.concatenate([mo.project_masks_on_boxes(masks[int(r[0])], r[None, 1:], [gi[j]]) for j, r in enumerate(rois)])
    np.testing.assert_array_equal(t.cpu().numpy(), ref)


def test_resize_nearest_bit_exact(g):
    import torch.nn.functional as F
    from object_detectors_amd import ops
    from object_detectors_amd.tvision.transform import resized_size
    for j in range(4):
        m = g[f"resize_in{j}"]
        mn, mx = (float(v) for v in g[f"resize_minmax{j}"])
        out = ops.mask_resize_nearest(torch.from_numpy(m).to(dev()), resized_size(m.shape[1], m.shape[2], mn, mx))
        np.testing.assert_array_equal(out.cpu().numpy(), g[f"resize_out{j}"])
    m = mo.synth_masks(3, 5, 480, 640)
    size = resized_size(480, 640, 800.0, 1333.0)
    ref = F.interpolate(torch.from_numpy(m)[:, None].float(), size=size)[:, 0].byte()
    assert torch.equal(ops.mask_resize_nearest(torch.from_numpy(m).to(dev()), size).cpu(), ref)


def test_paste(g):
    from object_detectors_amd import ops
    out = ops.paste_masks(torch.from_numpy(g["paste_masks"]).to(dev()), torch.from_numpy(g["paste_boxes"]).to(dev()), (32, 40))
    np.testing.assert_allclose(out.cpu().numpy(), g["paste_out"], rtol=0, atol=1e-6)
    for i, o_s in enumerate([(96, 128), (50, 45)]):
        out = ops.paste_masks(torch.from_numpy(g[f"det_probs{i}"]).to(dev()), torch.from_numpy(g[f"post_boxes{i}"]).to(dev()), o_s)
        np.testing.assert_allclose(out.cpu().numpy(), g[f"post_masks{i}"], rtol=0, atol=1e-6)
    rng = np.random.default_rng(12)
    d = 20
    x1, y1 = rng.uniform(-40, 1000, d), rng.uniform(-40, 760, d)
    boxes = np.stack([x1, y1, x1 + rng.uniform(0.5, 300, d), y1 + rng.uniform(0.5, 300, d)], 1).astype(np.float32)
    masks = rng.uniform(0, 1, (d, 1, 28, 28)).astype(np.float32)
    out = ops.paste_masks(torch.from_numpy(masks).to(dev()), torch.from_numpy(boxes).to(dev()), (800, 1066))
    np.testing.assert_allclose(out.cpu().numpy(), mo.paste_masks_in_image(masks, boxes, (800, 1066)), rtol=0, atol=1e-6)
    assert ops.paste_masks(torch.zeros((0, 1, 28, 28), device=dev()), torch.zeros((0, 4), device=dev()), (10, 12)).shape == (0, 1, 10, 12)
