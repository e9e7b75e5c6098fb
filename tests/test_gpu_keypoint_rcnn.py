"""Keypoint R-CNN on the device (csrc/keypoint_kernels.hip, tvision/keypoint_rcnn.py, the keypoint parts of tvision/transform.py) against
tests/golden/g18_keypoint_rcnn.npz (the reference's own outputs), tests/keypoint_rcnn_oracle.py and torch on the CPU.

Bars.  Targets, valid flags, count, flip and resize: exact.  Loss: 1e-5 relative of the float64 value (a tree sum over 3136 terms loses
about 12 * 2^-24, the rest is margin for exp); fp32 gradient: 1e-6 absolute of the float64 gradient (which carries the 1 / N_valid); the
bf16 gradient the convolutions read is that fp32 gradient rounded, bit for bit.  Deconvolution: the yardsticks of
test_gpu_mask.py::test_deconv_forward_dgrad_wgrad.  heatmaps_to_keypoints: see test_heatmaps_to_keypoints.  End to end: see
test_training_step_matches_cpu_module."""
import os

import numpy as np
import pytest

from oracle import detrand
from tests import keypoint_rcnn_oracle as ko

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_keypoint_rcnn.npz")
K, S, KP = 17, 56, 32
PX, BS = 128, 2
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def g():
    return dict(np.load(G, allow_pickle=False))


def bf(t):
    return t.to(torch.bfloat16)


def cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def rel(a, b):
    """What `a` loses against `b`: the relative L2 error."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a - b).norm() / (b.norm() + 1e-300))


def within_1ulp(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) <= np.spacing(np.abs(b)).astype(np.float64)


def close_of_value(a, b, tol=4e-3):
    a, b = a.double().cpu(), b.double().cpu()
    bound = tol * b.abs() + tol * float(b.abs().mean()) + 1e-12
    bad = ((a - b).abs() > bound).sum().item()
    assert bad == 0, (bad, float((a - b).abs().max()), float(b.abs().max()))


# ---------------------------------------------------------------------------------------------------------------- targets
def _target_inputs(g):
    kps = [torch.from_numpy(g[f"gt_keypoints{i}"]).to(dev()) for i in range(2)]
    rois = np.concatenate([np.concatenate([np.full((g[f"props{i}"].shape[0], 1), i, np.float32), g[f"props{i}"]], 1) for i in range(2)])
    gi = np.concatenate([g[f"matched{i}"] for i in range(2)])
    return kps, torch.from_numpy(rois).to(dev()), torch.from_numpy(gi).to(dev())


def test_targets_equal_the_fixture(g):
    from object_detectors_amd import ops
    kps, rois, gi = _target_inputs(g)
    assert rois.shape[0] == 24
    t, v, c = ops.keypoint_targets(kps, rois, gi, S)
    np.testing.assert_array_equal(t.cpu().numpy(), g["target"])
    np.testing.assert_array_equal(v.cpu().numpy(), g["valid"])
    assert int(c) == int(g["valid"].sum())
    # the cases: right edge, bottom edge, both (-> 55), a row with none valid, v = 0, outside
    assert int(t[0, 1]) % S == S - 1 and int(t[0, 2]) // S == S - 1 and int(t[0, 3]) == S * S - 1 and not v[1].any()
    vis = np.concatenate([g[f"gt_keypoints{i}"][g[f"matched{i}"]][..., 2] for i in range(2)]) > 0
    assert (~vis & (g["valid"] == 0)).any() and (vis & (g["valid"] == 0)).any()
    # a padded bucket: rows past valid_rows repeat RoI 0 and are not valid
    pad = torch.cat([rois, rois[:1].expand(8, 5)]).contiguous()
    t2, v2, c2 = ops.keypoint_targets(kps, pad, torch.cat([gi, gi[:1].expand(8)]), S, valid_rows=24)
    assert torch.equal(t2[:24], t) and torch.equal(v2[:24], v) and not v2[24:].any() and not t2[24:].any() and int(c2) == int(c)


# ---------------------------------------------------------------------------------------------------------------- loss
@pytest.fixture(scope="module")
def loss_case(g):
    """The fixture's targets on 28 x 28 logits drawn by seed; the float64 CPU loss and gradient through the bilinear x2, computed once."""
    import torch.nn.functional as F
    low = torch.from_numpy(detrand.uniform(int(g["seeds"][0]) + 10, (24, K, 28, 28), -4.0, 4.0))
    target, valid = torch.from_numpy(g["target"]), torch.from_numpy(g["valid"])
    x = low.double().requires_grad_(True)
    hi = F.interpolate(x, scale_factor=2.0, mode="bilinear", align_corners=False)
    sel = torch.nonzero(valid.reshape(-1)).squeeze(1)
    loss = F.cross_entropy(hi.reshape(24 * K, S * S)[sel], target.reshape(-1)[sel])
    loss.backward()
    return dict(low=low, z=ko.space_to_depth(low, KP), target=target.int(), valid=valid.int(), loss=float(loss.detach()), grad=x.grad,
                hi=hi.detach())


def _loss_args(c, rows=None):
    z, t, v = c["z"].to(dev()), c["target"].to(dev()), c["valid"].to(dev())
    if rows is not None:                  # a padded bucket: the extra rows repeat row 0 and are not valid
        n = rows - z.shape[0]
        z = torch.cat([z, z[:1].expand(n, 14, 14, 4 * KP)]).contiguous()
        t = torch.cat([t, torch.zeros((n, K), dtype=torch.int32, device=dev())])
        v = torch.cat([v, torch.zeros((n, K), dtype=torch.int32, device=dev())])
    return z, t, v, v.sum().to(torch.int32).reshape(1)


def test_heatmaps_are_the_bilinear_x2(loss_case):
    from object_detectors_amd import ops
    hm = ops.keypoint_heatmaps(loss_case["z"].to(dev()), K)
    assert hm.shape == (24, K, S, S)
    assert float((hm.cpu().double() - loss_case["hi"]).abs().max()) <= 4 * 2.0 ** -24 * 4.0           # three roundings of values below 4


def test_loss_and_gradient(loss_case):
    from object_detectors_amd import ops
    c = loss_case
    outs = [ops.keypoint_loss(*_loss_args(c), want_f32_grad=True) for _ in range(2)]
    loss, dz, dbias, d32 = outs[0]
    err = abs(float(loss) - c["loss"]) / abs(c["loss"])
    gerr = float((d32.cpu().double() - c["grad"]).abs().max())
    print(f"keypoint_loss: loss {float(loss):.8f} float64 {c['loss']:.8f} rel {err:.3e}; gradient max abs error {gerr:.3e} "
          f"(largest gradient {float(c['grad'].abs().max()):.3e})")
    assert err <= 1e-5
    assert gerr <= 1e-6
    # what the convolutions read: that gradient rounded to bf16, in the sub-pixel layout, zeros in the padded channels
    assert torch.equal(dz.cpu().view(torch.int16), bf(ko.space_to_depth(d32.cpu(), KP)).view(torch.int16))
    ref_db = c["grad"].sum((0, 2, 3))
    torch.testing.assert_close(dbias.cpu().double(), ref_db, rtol=0, atol=1e-6 * 784)
    for a, b in zip(outs[0], outs[1]):                     # fixed order: the same bits from run to run
        assert torch.equal(a, b)


def test_loss_all_invalid_no_rows_and_padded_bucket(loss_case):
    from object_detectors_amd import ops
    c = loss_case
    z, t, v, n = _loss_args(c)
    loss, dz, dbias, d32 = ops.keypoint_loss(z, t, torch.zeros_like(v), torch.zeros_like(n), want_f32_grad=True)
    assert float(loss) == 0.0 and not dz.any() and not dbias.any() and not d32.any()
    loss, dz, dbias = ops.keypoint_loss(z[:0], t[:0], v[:0], torch.zeros_like(n))
    assert float(loss) == 0.0 and dz.shape[0] == 0 and not dbias.any()
    full = ops.keypoint_loss(z, t, v, n)
    pad = ops.keypoint_loss(*_loss_args(c, rows=32))
    assert torch.equal(full[0], pad[0]) and torch.equal(full[2], pad[2])
    assert torch.equal(pad[1][:24], full[1]) and not pad[1][24:].any()


# ---------------------------------------------------------------------------------------------------------------- deconvolution
def test_deconv_forward_dgrad_wgrad():
    """ConvTranspose2d(512, 17, 4, 2, 1) as the sub-pixel 3x3 convolution on the MFMA kernels, against nn.functional.conv_transpose2d on
    bf16-rounded inputs (the yardsticks of test_gpu_mask.py::test_deconv_forward_dgrad_wgrad)."""
    import torch.nn.functional as F
    from object_detectors_amd import ops
    from object_detectors_amd.tvision import keypoint_rcnn as kr
    rows = 32
    torch.manual_seed(1)
    pr = kr.KeypointRCNNPredictor(512, K).to(dev())
    with torch.no_grad():
        pr.kps_score_lowres.bias.uniform_(-0.2, 0.2)
    dc = pr.kps_score_lowres
    gen = torch.Generator().manual_seed(rows)
    x = bf(torch.relu(torch.randn(rows, 14, 14, 512, generator=gen))).to(dev())
    wf, wd, b = pr._pack.get(dc.weight, dc.bias)
    shape = ops.conv_shape(rows, 14, 14, 512, 4 * KP, 3, 1)
    z = torch.empty((rows, 14, 14, 4 * KP), device=dev(), dtype=torch.float32)
    ops.conv_fwd_ex(shape, x, wf, z, shift=b, out_f32=True)
    wt = bf(dc.weight.detach()).float().cpu().double()
    xc = x.float().cpu().permute(0, 3, 1, 2).double()
    ref = F.conv_transpose2d(xc, wt, dc.bias.detach().cpu().double(), stride=2, padding=1)
    close_of_value(kr.depth_to_space(z.cpu(), K), ref)
    zp = z.cpu().reshape(rows, 14, 14, 4, KP)[..., K:]
    assert not zp.any()                                                     # padded channels: zero weights and zero bias
    # data gradient with the ReLU of the layer below folded in
    dhi = torch.randn(rows, K, 28, 28, generator=gen) * 1e-3
    dz = bf(ko.space_to_depth(dhi, KP)).to(dev())
    dzn = kr.depth_to_space(dz.float().cpu(), K).double()
    dx = torch.empty_like(x)
    ops.conv_dgrad_mask(shape, dz, wd, dx, x)
    refdx = F.conv2d(dzn, wt, stride=2, padding=1) * (xc > 0)             # the adjoint of conv_transpose2d
    close_of_value(dx.float().cpu().permute(0, 3, 1, 2), refdx)
    # weight gradient, scattered back to [512, 17, 4, 4]: fixed order, bit-identical from run to run
    dws = []
    for _ in range(2):
        dw = torch.zeros((4 * KP, 9 * 512), device=dev(), dtype=torch.float32)
        ops.conv_wgrad(shape, x, dz, dw)
        dws.append(dw)
    assert torch.equal(dws[0], dws[1])
    dwt = kr.subpixel_weight_grad(dws[0].reshape(4 * KP, 3, 3, 512), 512, K).cpu().double()
    wl = wt.clone().requires_grad_(True)
    (F.conv_transpose2d(xc, wl, stride=2, padding=1) * dzn).sum().backward()
    torch.testing.assert_close(dwt, wl.grad, rtol=2e-3, atol=2e-3 * float(wl.grad.abs().max()))


# ---------------------------------------------------------------------------------------------------------------- heatmaps_to_keypoints
SIZES = [(1, 1), (3, 8), (8, 3), (56, 56), (112, 112), (57, 113), (200, 131), (333, 97), (480, 300)]       # (h, w) after the ceil


def _h2k_rois(seed):
    """Six RoIs per size; (1, 1) is built from a width and a height below 1 (clamped to 1), the others from sides in (n - 1, n]."""
    rng = np.random.default_rng(seed)
    rows = []
    for h, w in SIZES:
        for _ in range(6):
            x1, y1 = rng.uniform(-20, 600), rng.uniform(-20, 400)
            fw = rng.uniform(0.2, 0.95) if w == 1 else w - rng.uniform(0.0, 0.9)
            fh = rng.uniform(0.2, 0.95) if h == 1 else h - rng.uniform(0.0, 0.9)
            rows.append([x1, y1, x1 + fw, y1 + fh])
    return torch.from_numpy(np.array(rows, np.float32))


def _maps(kind, n, seed):
    gen = torch.Generator().manual_seed(seed)
    if kind == "normal":
        return torch.randn(n, K, S, S, generator=gen)
    yy, xx = torch.meshgrid(torch.arange(float(S)), torch.arange(float(S)), indexing="ij")
    c = torch.rand(n, K, 2, generator=gen) * S
    bump = 10 * torch.exp(-((yy - c[..., 0, None, None]) ** 2 + (xx - c[..., 1, None, None]) ** 2) / 18)
    return bump + 0.01 * torch.randn(n, K, S, S, generator=gen)


@pytest.fixture(scope="module")
def h2k_reference():
    """torch's bicubic + argmax on the CPU, once for both kinds of maps: positions, float32 maps (for the near-tie rule) and T."""
    import torch.nn.functional as F
    out = {}
    for kind, seed in (("normal", 31), ("bumps", 32)):
        rois = _h2k_rois(seed)
        maps = _maps(kind, rois.shape[0], seed + 100)
        w = (rois[:, 2] - rois[:, 0]).clamp(min=1)
        h = (rois[:, 3] - rois[:, 1]).clamp(min=1)
        big, pos, worst = [], [], 0.0
        for i in range(rois.shape[0]):
            size = (int(h[i].ceil()), int(w[i].ceil()))
            assert size == SIZES[i // 6]
            a = F.interpolate(maps[i][None], size=size, mode="bicubic", align_corners=False)[0].reshape(K, -1)
            d = F.interpolate(maps[i][None].double(), size=size, mode="bicubic", align_corners=False)[0].reshape(K, -1)
            worst = max(worst, float((a.double() - d).abs().max()))
            assert torch.equal(a.argmax(1), d.argmax(1))           # the reference alone is nowhere near a tie on these inputs
            big.append(a)
            pos.append(a.argmax(1))
        out[kind] = dict(rois=rois, maps=maps, w=w, h=h, big=big, pos=torch.stack(pos), T=2 * worst, absmax=float(maps.abs().max()))
    return out


@pytest.mark.parametrize("kind", ["normal", "bumps"])
def test_heatmaps_to_keypoints(h2k_reference, kind):
    """Against F.interpolate(..., 'bicubic') + argmax on the CPU.  A position may differ only at a near tie (the CPU map's values at the two
    positions differ by at most T) and on at most 1 % of the pairs; scores within T; x and y within 1 ulp of the CPU's wherever the position
    agrees.  T = twice the largest difference between torch's own float32 and float64 bicubic on these inputs (recomputed here)."""
    from object_detectors_amd import ops
    r = h2k_reference[kind]
    xy, sc = ops.heatmaps_to_keypoints(r["maps"].to(dev()), r["rois"].to(dev()))
    xy, sc = xy.cpu(), sc.cpu()
    n = r["rois"].shape[0]
    T = r["T"]
    print(f"heatmaps_to_keypoints[{kind}]: T = {T:.3e} = {T / r['absmax']:.3e} * max|map|")
    assert (xy[..., 2] == 1).all()
    differ = 0
    for i in range(n):
        ow, oh = int(r["w"][i].ceil()), int(r["h"][i].ceil())
        wcor, hcor = r["w"][i] / ow, r["h"][i] / oh
        # the device's position, from its x and y; checked by forming x and y again from it with the float32 rule
        xi = torch.round((xy[i, :, 0].double() - r["rois"][i, 0].double()) / wcor.double() - 0.5).long().clamp(0, ow - 1)
        yi = torch.round((xy[i, :, 1].double() - r["rois"][i, 1].double()) / hcor.double() - 0.5).long().clamp(0, oh - 1)
        x_again = (xi.float() + 0.5) * wcor + r["rois"][i, 0]
        y_again = (yi.float() + 0.5) * hcor + r["rois"][i, 1]
        assert within_1ulp(xy[i, :, 0].numpy(), x_again.numpy()).all() and within_1ulp(xy[i, :, 1].numpy(), y_again.numpy()).all(), i
        pos = yi * ow + xi
        cpu_at_cpu = r["big"][i][torch.arange(K), r["pos"][i]]
        cpu_at_dev = r["big"][i][torch.arange(K), pos]
        moved = pos != r["pos"][i]
        differ += int(moved.sum())
        assert float((cpu_at_cpu - cpu_at_dev).abs().max()) <= T, (i, "a position differs where the CPU map has no near tie")
        assert float((sc[i] - cpu_at_cpu).abs().max()) <= T, (i, float((sc[i] - cpu_at_cpu).abs().max()))
    print(f"heatmaps_to_keypoints[{kind}]: {differ} of {n * K} positions differ from the CPU's")
    assert differ <= 0.01 * n * K


def test_heatmaps_to_keypoints_constant_map_and_fixture(g):
    from object_detectors_amd import ops
    rois = _h2k_rois(5)
    w = (rois[:, 2] - rois[:, 0]).clamp(min=1)
    h = (rois[:, 3] - rois[:, 1]).clamp(min=1)
    x0 = (0.5 * (w / w.ceil()) + rois[:, 0])[:, None].expand(-1, K)
    y0 = (0.5 * (h / h.ceil()) + rois[:, 1])[:, None].expand(-1, K)
    # a map of zeros stays exactly constant under any weights: position 0 for every size, score 0
    xy, sc = ops.heatmaps_to_keypoints(torch.zeros((rois.shape[0], K, S, S), device=dev()), rois.to(dev()))
    assert torch.equal(xy[..., 0].cpu(), x0) and torch.equal(xy[..., 1].cpu(), y0) and not sc.any()
    # another constant: the bicubic weights sum to one only up to rounding, so the resized map is exactly constant only where the weights
    # are exact - the 1 x 1 RoIs (one pixel) and the 56 x 56 ones (weights 0, 1, 0, 0); the scores hold everywhere
    xy, sc = ops.heatmaps_to_keypoints(torch.full((rois.shape[0], K, S, S), 0.25, device=dev()), rois.to(dev()))
    exact = [i for i in range(rois.shape[0]) if SIZES[i // 6] in ((1, 1), (56, 56))]
    assert torch.equal(xy[exact, :, 0].cpu(), x0[exact]) and torch.equal(xy[exact, :, 1].cpu(), y0[exact])
    # (a coefficient is three float32 operations on magnitudes below 8, so it is off by at most 3 * 2^-22; four coefficients per axis,
    # two axes; the score is the LARGEST of the resized values, so it sits at that end)
    assert float((sc.cpu() - 0.25).abs().max()) <= 0.25 * 24 * 2.0 ** -22
    # the reference's own outputs (roi_heads.heatmaps_to_keypoints and keypointrcnn_inference)
    fr = torch.from_numpy(g["h2k_rois"])
    maps = torch.from_numpy(detrand.uniform(int(g["seeds"][1]), (fr.shape[0], K, S, S), -4.0, 4.0))
    xy, sc = ops.heatmaps_to_keypoints(maps.to(dev()), fr.to(dev()))
    same = within_1ulp(xy.cpu().numpy(), g["h2k_xy"]).all(-1)
    assert same.mean() >= 0.99
    assert np.abs(sc.cpu().numpy() - g["h2k_scores"]).max() <= 1e-5 * 4.0
    boxes = torch.from_numpy(np.concatenate([g["det_boxes0"], g["det_boxes1"]]))
    x = torch.from_numpy(detrand.uniform(int(g["seeds"][2]), (9, K, S, S), -4.0, 4.0))
    xy, sc = ops.heatmaps_to_keypoints(x.to(dev()), boxes.to(dev()))
    assert within_1ulp(xy.cpu().numpy(), np.concatenate([g["det_xy0"], g["det_xy1"]])).all(-1).mean() >= 0.99


# ---------------------------------------------------------------------------------------------------------------- transform / ingest
def test_ingest_flip_and_resize_equal_the_fixture_and_the_float_route(g):
    from object_detectors_amd.tvision.transform import GeneralizedRCNNTransform
    for j in range(3):
        h, w, nh, nw = (int(v) for v in g[f"tf_sizes{j}"])
        t = GeneralizedRCNNTransform(64, 2000, MEAN, STD, fixed_size=(nw, nh), keypoints=True)
        t.eval()
        img = torch.from_numpy(np.random.default_rng(j).integers(0, 256, (h, w, 3), dtype=np.uint8))
        kp = torch.from_numpy(g[f"tf_in{j}"])
        gbox = torch.tensor([[1.0, 2.0, 9.0, 8.0]]).repeat(kp.shape[0], 1)
        for flip, key in ((False, f"tf_resized{j}"), (True, f"tf_flipped_resized{j}")):
            il, tg = t.ingest([img], [{"boxes": gbox, "keypoints": kp}], flips=[flip])
            assert il.image_sizes[0] == (nh, nw)
            np.testing.assert_array_equal(tg[0]["keypoints"].cpu().numpy(), g[key])
            # the float route on the flipped float image and the flipped targets
            fimg = img.permute(2, 0, 1).float().div(255).to(dev())
            fkp = kp.clone()
            if flip:
                fimg, fkp = fimg.flip(-1), ko.flip_coco_person_keypoints(kp.clone(), w)
            il2, tg2 = t([fimg], [{"boxes": gbox.to(dev()), "keypoints": fkp.to(dev())}])
            assert torch.equal(tg2[0]["keypoints"], tg[0]["keypoints"]) and il2.image_sizes == il.image_sizes
        assert torch.equal(kp, torch.from_numpy(g[f"tf_in{j}"]))                  # the caller's tensors are not modified


def test_ingest_batch_of_three_and_refusals():
    from object_detectors_amd.tvision.transform import GeneralizedRCNNTransform
    from object_detectors_amd.tvision.transforms import SSDAugmentation
    t = GeneralizedRCNNTransform(64, 96, MEAN, STD, keypoints=True)
    t.eval()
    rng = np.random.default_rng(7)
    shapes = [(40, 60), (57, 33), (48, 48)]
    imgs = [torch.from_numpy(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in shapes]
    tg = []
    for i, (h, w) in enumerate(shapes):
        n = (3, 0, 2)[i]                                  # an image without instances in the middle
        kp = np.zeros((n, K, 3), np.float32)
        kp[..., 0], kp[..., 1], kp[..., 2] = rng.uniform(0, w, (n, K)), rng.uniform(0, h, (n, K)), rng.integers(0, 3, (n, K))
        kp[kp[..., 2] == 0] = 0
        tg.append({"boxes": torch.tensor([[1.0, 2.0, 9.0, 8.0]]).repeat(n, 1), "keypoints": torch.from_numpy(kp)})
    flips = [True, True, False]
    il, out = t.ingest(imgs, tg, flips=flips)
    for i, (h, w) in enumerate(shapes):
        ref = tg[i]["keypoints"].clone()
        if flips[i]:
            ref = ko.flip_coco_person_keypoints(ref, w)
        ref = ko.resize_keypoints(ref, (h, w), il.image_sizes[i])
        assert torch.equal(out[i]["keypoints"].cpu(), ref), i
    # a transform of a model without a keypoint branch keeps refusing them; so do the SSD policies, and augment on this route
    plain = GeneralizedRCNNTransform(64, 96, MEAN, STD)
    with pytest.raises(ValueError, match="keypoints"):
        plain.ingest(imgs[:1], tg[:1])
    with pytest.raises(ValueError, match="keypoints"):
        SSDAugmentation("ssd").draw(shapes[:1], tg[:1])
    with pytest.raises(ValueError, match="keypoints"):
        t.ingest(imgs[:1], [{"boxes": torch.zeros((1, 4)), "keypoints": torch.zeros(1, K, 2)}])
    with pytest.raises(ValueError, match="17"):
        t.ingest(imgs[:1], [{"boxes": torch.zeros((1, 4)), "keypoints": torch.zeros(1, 5, 3)}], flips=[True])
    # the C entry refuses the same on its own (public ABI): a flipped table entry beside K != 17
    import ctypes
    from object_detectors_amd._lib import IngestImage, lib, ptr, stream_ptr
    table = (IngestImage * 1)(IngestImage(0, 40, 60, 64, 96, 1, 0))
    tdev = torch.from_numpy(np.frombuffer(table, dtype=np.uint8).copy()).to(dev())
    kp5, offs = torch.zeros((1, 5, 3), device=dev()), torch.tensor([0, 1], dtype=torch.int64, device=dev())
    args = (ptr(kp5), ptr(torch.empty_like(kp5)), 1, 5, ptr(offs), ctypes.cast(table, ctypes.c_void_p), ctypes.c_void_p(tdev.data_ptr()), 1, stream_ptr())
    assert lib().mi355det_flip_resize_keypoints(*args) == -1 and b"17 keypoints" in lib().mi355det_last_error()
    table[0].flip = 0
    assert lib().mi355det_flip_resize_keypoints(*args) == 0


# ---------------------------------------------------------------------------------------------------------------- end to end
def _targets(seed):
    return [{k: torch.from_numpy(v).to(dev()) for k, v in t.items()} for t in ko.synth_persons(seed, PX, BS, K)]


def _model(cls, seed=0, **kw):
    torch.manual_seed(seed)
    m = cls(num_classes=2, device=dev(), seed=seed, min_size=PX, max_size=PX, **kw)
    m.train()
    return m


def _branch_params(model):
    return list(model.keypoint_head.convs) + [model.keypoint_predictor.kps_score_lowres]


def test_training_step_matches_cpu_module():
    """One training step at 128 px, batch 2, against the CPU module (nn.Conv2d x 8, nn.ConvTranspose2d, bilinear x2, cross entropy) in
    float64 on the same pooled features, RoIs and targets.  box_batch_size_per_image = 16 keeps the positives (at most 4 per image) and so
    the CPU module small.  The bars are not constants: the YARDSTICK is the same CPU module with its weights, the activations between its
    layers and the gradients between its layers rounded to bf16 (what the kernels store), against the float64 module; the device may lose
    twice what the yardstick loses, and no cosine falls below 0.99.
      * Gradients (9 weights, 9 biases): what is lost is the relative L2 error against the float64 gradient.
      * loss_keypoint, like for like: the kernel's per-pair loss terms (lse - logit[target], read out of its workspace) against the
        float64 terms; what is lost is their MEAN ABSOLUTE error, the device's held to twice the yardstick's.
      * loss_keypoint, the error of the mean: held to twice the yardstick terms' RMS error / sqrt(number of RoIs).  Not to the yardstick's
        own error of the mean: each device layer equals the rounded CPU layer on the same input up to 1e-4 of its values (fp32 against
        float64 accumulation flips a rounding now and then), and after eight layers 31 % of the values differ, so the device's rounding
        noise is another draw of the yardstick's distribution, and one draw's signed mean (1.0e-4 here) is no scale for another's (7.1e-4).
        The terms of one RoI share their activations, so the RoIs, not the pairs, count as the independent samples of the mean.
      * kps_score_lowres.bias: its gradient is zero in exact arithmetic (a softmax's gradient sums to zero over the map, and the bias
        shifts the whole map), so a cosine has no meaning and the L2 rule compares noise with noise.  Instead an absolute bound per
        keypoint: |dbias[k]| <= (40 + 4 max|logit|) * 2^-24 * sum |d loss / d logit| over the keypoint's 56 x 56 maps (float64).  The
        factor: a logit of the x2 carries 3 roundings and its distance to the maximum one more, each of eps * |logit|, which the exponential
        turns into a relative error of the softmax value (4 max|logit|); the exponential, the quotient, the products with 1 / N and the
        16 weighted additions of the gather add about 26 eps, the per-thread, wavefront, workgroup and row sums about 14.

    Measured on an MI355X (this test's own print), loss 28.27 on 8 RoIs and 94 pairs: see profiles/r31_keypoint_rcnn.md; the 16
    head gradients lose 4.3e-2 .. 7.7e-2 where the yardstick loses 4.3e-2 .. 8.2e-2 (bars 8.5e-2 .. 1.6e-1), cosines 0.9970 .. 0.9991;
    kps_score_lowres.weight loses 9.6e-3 (yardstick 1.0e-2, bar 2.0e-2), cosine 0.99995."""
    import torch.nn.functional as F
    from object_detectors_amd.tvision.keypoint_rcnn import KeypointRCNN
    model = _model(KeypointRCNN, box_batch_size_per_image=16)
    model.keep_keypoint_inputs = True
    x = torch.from_numpy(detrand.uniform(4242, (BS, 3, PX, PX), 0.0, 1.0)).to(dev())
    tg = _targets(3)
    for p in model.head_parameters():
        p.grad = None
    losses = model(x, tg)
    torch.cuda.synchronize()
    assert set(losses) == {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg", "loss_keypoint"}
    ki = model.last_keypoint_inputs
    r = ki["rois"].shape[0]
    assert r == model.last_keypoint_rows and 1 <= r <= 8
    rois, gt = ki["rois"].cpu(), ki["gt_index"].cpu()
    # the targets the branch used are the reference rule's on its RoIs
    kp_per_roi = torch.stack([tg[int(rr[0])]["keypoints"].cpu()[int(gi)] for rr, gi in zip(rois, gt)])
    t_ref, v_ref = ko.keypoints_to_heatmap(kp_per_roi, rois[:, 1:], S)
    assert torch.equal(ki["target"].cpu().long(), t_ref) and torch.equal(ki["valid"].cpu().long(), v_ref) and int(ki["count"]) == int(v_ref.sum())
    assert int(v_ref.sum()) > 0
    pooled = ki["pooled"].float().cpu().permute(0, 3, 1, 2).double()
    sel = torch.nonzero(v_ref.reshape(-1)).squeeze(1)
    nets = {}
    for name, rounding in (("float64", False), ("bf16", True)):
        net = ko.branch(K)
        with torch.no_grad():
            for s, d in zip(_branch_params(model), [m for m in net if hasattr(m, "weight")]):
                d.weight.copy_(s.weight.detach().cpu())
                d.bias.copy_(s.bias.detach().cpu())
        logits = ko.run_branch(net, pooled, storage_rounding=rounding)
        logits.retain_grad()
        terms = F.cross_entropy(logits.reshape(r * K, S * S)[sel], t_ref.reshape(-1)[sel], reduction="none")
        loss = terms.mean()
        loss.backward()
        nets[name] = (float(loss.detach()), [m for m in net if hasattr(m, "weight")], terms.detach(), logits.detach(), logits.grad)
    l64, ref, terms64, logits64, dlogits64 = nets["float64"]
    lbf, yard, termsbf = nets["bf16"][:3]
    lk = float(losses["loss_keypoint"])
    termsdev = ki["loss_terms"].cpu().double().reshape(-1)[sel]
    assert not ki["loss_terms"].cpu().reshape(-1)[v_ref.reshape(-1) == 0].any()
    assert abs(float(termsdev.mean()) - lk) <= 1e-6 * lk                     # the loss is the mean of those terms
    y_terms, d_terms = float((termsbf - terms64).abs().mean()) / l64, float((termsdev - terms64).abs().mean()) / l64
    y_rms = float((termsbf - terms64).pow(2).mean().sqrt()) / l64
    mean_bar, d_loss = 2 * y_rms / r ** 0.5, abs(lk - l64) / l64
    print(f"loss_keypoint: device {lk:.6f} float64 {l64:.6f} bf16 yardstick {lbf:.6f} ({len(sel)} pairs, {r} RoIs); terms: device loses "
          f"{d_terms:.3e}, yardstick {y_terms:.3e}, bar {2 * y_terms:.3e}; mean: device moved by {d_loss:.3e}, the yardstick's by "
          f"{abs(lbf - l64) / l64:.3e}, yardstick terms' RMS {y_rms:.3e}, bar {mean_bar:.3e}")
    failures = []
    if d_terms > 2 * y_terms:
        failures.append(("loss_keypoint terms", d_terms, 2 * y_terms))
    if d_loss > mean_bar:
        failures.append(("loss_keypoint mean", d_loss, mean_bar))
    dbias = model.keypoint_predictor.kps_score_lowres.bias.grad.detach().cpu().double()
    bias_bar = (40 + 4 * float(logits64.abs().max())) * 2.0 ** -24 * dlogits64.abs().sum((0, 2, 3))
    print(f"kps_score_lowres.bias gradient: largest {float(dbias.abs().max()):.3e}, smallest bar {float(bias_bar.min()):.3e} "
          f"(max|logit| {float(logits64.abs().max()):.1f})")
    if bool((dbias.abs() > bias_bar).any()):
        failures.append(("kps_score_lowres.bias", dbias.abs().tolist(), bias_bar.tolist()))
    for i, (s, d, y) in enumerate(zip(_branch_params(model), ref, yard)):
        for what in ("weight", "bias"):
            if i == 8 and what == "bias":                  # zero in exact arithmetic: held to the absolute bound above
                continue
            a, b, c = getattr(s, what).grad.detach().cpu(), getattr(d, what).grad, getattr(y, what).grad
            dev_loses, yard_loses, cs = rel(a, b), rel(c, b), cos(a, b)
            print(f"layer {i} {what}: device loses {dev_loses:.3e}, yardstick {yard_loses:.3e}, bar {2 * yard_loses:.3e}, cosine {cs:.6f}")
            if dev_loses > 2 * yard_loses or cs < 0.99:
                failures.append((i, what, dev_loses, 2 * yard_loses, cs))
    assert not failures, failures


def test_box_losses_equal_faster_rcnn():
    from object_detectors_amd.tvision.frcnn import FasterRCNN
    from object_detectors_amd.tvision.keypoint_rcnn import KeypointRCNN
    fr, kr = _model(FasterRCNN, 1), _model(KeypointRCNN, 1)
    kr.load_state_dict(fr.state_dict(), strict=False)
    x = torch.from_numpy(detrand.uniform(4243, (BS, 3, PX, PX), 0.0, 1.0)).to(dev())
    tg = _targets(5)
    torch.manual_seed(11)
    lf = fr(x, [{k: v for k, v in t.items() if k != "keypoints"} for t in tg])
    torch.manual_seed(11)
    lk = kr(x, tg)
    for k in ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"):
        assert float(lk[k]) == float(lf[k]), (k, float(lk[k]), float(lf[k]))
    assert float(lk["loss_keypoint"]) > 0


def test_step_without_positives():
    """A step whose sampler yields no positive RoI: every ground truth carries label 0, so every matched proposal is labelled background
    (an image without ground truth is refused by the inherited Faster R-CNN, as by the reference, and a ground truth with a positive label
    is itself a positive proposal).  The branch takes its r == 0 route inside the model (roi_heads.py:351-352: keypoint_logits.sum() * 0):
    loss_keypoint 0, zero gradients in every branch parameter."""
    from object_detectors_amd.tvision.keypoint_rcnn import KeypointRCNN
    model = _model(KeypointRCNN, 6)
    x = torch.from_numpy(detrand.uniform(4244, (BS, 3, PX, PX), 0.0, 1.0)).to(dev())
    tg = [dict(t, labels=torch.zeros_like(t["labels"])) for t in _targets(7)]
    for p in model.head_parameters():
        p.grad = None
    losses = model(x, tg)
    torch.cuda.synchronize()
    assert model.last_keypoint_rows == 0 and float(losses["loss_keypoint"]) == 0.0
    assert all(np.isfinite(float(v)) for v in losses.values())
    assert all(p.grad is not None and not p.grad.any() for mod in _branch_params(model) for p in mod.parameters())


def test_zero_positives_and_constructor():
    from object_detectors_amd.tvision import keypoint_rcnn as kr
    m = kr.keypointrcnn_resnet50_fpn(device=dev())
    assert m.transform.min_size == (640, 672, 704, 736, 768, 800) and m.transform.max_size == 1333 and m.num_classes == 2 and m.num_keypoints == 17
    assert tuple(m.keypoint_predictor.kps_score_lowres.weight.shape) == (512, 17, 4, 4)
    with pytest.raises(NotImplementedError):
        kr.keypointrcnn_resnet50_fpn(pretrained=True)
    with pytest.raises(NotImplementedError):
        kr.KeypointRCNNHeads(256, (256,) * 8)
    with pytest.raises(NotImplementedError):
        kr.KeypointRCNNHeads(256, (512,) * 4)
    with pytest.raises(NotImplementedError):
        kr.KeypointRCNNPredictor(256, 17)
    with pytest.raises(ValueError, match="num_keypoints"):          # an explicit K beside a predictor of another K is not ignored
        kr.KeypointRCNN(device=dev(), num_keypoints=17, keypoint_predictor=kr.KeypointRCNNPredictor(512, 5))
    assert kr.KeypointRCNN(device=dev(), num_keypoints=None, keypoint_predictor=kr.KeypointRCNNPredictor(512, 5)).num_keypoints == 5
    with pytest.raises(RuntimeError):
        m.keypoint_head(torch.zeros(1, 256, 14, 14, device=dev()))
    for p in m.head_parameters():
        p.grad = None
    m._zero_kp_grads()                                   # the r == 0 route: keypoint_logits.sum() * 0
    assert all(p.grad is not None and not p.grad.any() for mod in _branch_params(m) for p in mod.parameters())


def test_eval_list_keypoints_and_coco_evaluator():
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator, get_iou_types
    from object_detectors_amd.tvision.keypoint_rcnn import keypointrcnn_resnet50_fpn
    torch.manual_seed(2)
    model = keypointrcnn_resnet50_fpn(device=dev(), seed=2, min_size=PX, max_size=PX, box_score_thresh=0.0, box_detections_per_img=20)
    model.eval()
    model.keep_keypoint_inputs = True
    assert get_iou_types(model) == ["bbox", "keypoints"]
    seen = {}
    post = model.transform.postprocess

    def spy(result, image_shapes, original_sizes):
        seen["pre"] = [{k: v.clone() for k, v in r.items()} for r in result]
        seen["shapes"] = list(image_shapes)
        return post(result, image_shapes, original_sizes)
    model.transform.postprocess = spy
    sizes = [(100, 140), (150, 90)]
    imgs = [torch.from_numpy(detrand.uniform(4300 + i, (3, h, w), 0.0, 1.0)).to(dev()) for i, (h, w) in enumerate(sizes)]
    with torch.no_grad():
        det = model(imgs)
    torch.cuda.synchronize()
    ki = model.last_keypoint_inputs
    maps, rois = ki["maps"].cpu(), ki["rois"].cpu()
    ref_xy, ref_sc = ko.heatmaps_to_keypoints(maps, rois[:, 1:])
    o = 0
    for i, (d, pre) in enumerate(zip(det, seen["pre"])):
        n = d["boxes"].shape[0]
        assert set(d) == {"boxes", "labels", "scores", "keypoints", "keypoints_scores"}
        assert d["keypoints"].shape == (n, K, 3) and d["keypoints_scores"].shape == (n, K) and (d["keypoints"][..., 2] == 1).all()
        assert torch.equal(rois[o:o + n, 1:], pre["boxes"].cpu()) and (rois[o:o + n, 0] == i).all()
        # the reference rules on the model's own heatmaps (positions may move at near ties of an untrained head: at most 1 %)
        same = within_1ulp(pre["keypoints"].cpu().numpy(), ref_xy[o:o + n].numpy()).all(-1)
        assert same.mean() >= 0.99, same.mean()
        assert float((pre["keypoints_scores"].cpu() - ref_sc[o:o + n]).abs().max()) <= 1e-5 * float(maps.abs().max())
        back = ko.resize_keypoints(pre["keypoints"].cpu(), seen["shapes"][i], sizes[i])
        assert torch.equal(d["keypoints"].cpu(), back)
        o += n
    assert o == rois.shape[0] and o > 0
    # into the evaluator as they are
    persons = ko.synth_persons(9, 90, 2, K)
    anns = []
    for i, t in enumerate(persons):
        for b, kp in zip(t["boxes"], t["keypoints"]):
            anns.append({"id": len(anns) + 1, "image_id": i + 1, "category_id": 1, "bbox": [float(b[0]), float(b[1]), float(b[2] - b[0]), float(b[3] - b[1])],
                         "area": float((b[2] - b[0]) * (b[3] - b[1])), "iscrowd": 0, "keypoints": [float(v) for v in kp.reshape(-1)],
                         "num_keypoints": int((kp[:, 2] > 0).sum())})
    gt = {"images": [{"id": 1, "height": 100, "width": 140}, {"id": 2, "height": 150, "width": 90}], "categories": [{"id": 1, "name": "person"}],
          "annotations": anns}
    ev = CocoEvaluator(gt, ["bbox", "keypoints"])
    ev.update({1: det[0], 2: det[1]})
    ev.synchronize_between_processes()
    ev.accumulate()
    ev.summarize()
    assert ev.coco_eval["keypoints"].stats.shape == (10,) and ev.coco_eval["bbox"].stats.shape == (12,)
    assert np.isfinite(ev.coco_eval["keypoints"].stats).all()


def test_state_dict_round_trip_and_shim():
    from object_detectors_amd import shims
    from object_detectors_amd.tvision.keypoint_rcnn import KeypointRCNN
    a, b = _model(KeypointRCNN, 3), _model(KeypointRCNN, 4)
    sd = a.state_dict()
    keys = [f"roi_heads.keypoint_head.{i}.{p}" for i in range(0, 16, 2) for p in ("weight", "bias")] + \
           [f"roi_heads.keypoint_predictor.kps_score_lowres.{p}" for p in ("weight", "bias")]
    for k in keys:
        assert k in sd
    assert sum(k.startswith("roi_heads.keypoint_") for k in sd) == len(keys)
    assert tuple(sd["roi_heads.keypoint_head.0.weight"].shape) == (512, 256, 3, 3) and tuple(sd["roi_heads.keypoint_head.14.weight"].shape) == (512, 512, 3, 3)
    assert tuple(sd["roi_heads.keypoint_predictor.kps_score_lowres.weight"].shape) == (512, K, 4, 4)
    b.load_state_dict({"module." + k: v for k, v in sd.items()})
    sb = b.state_dict()
    for k in sd:
        assert torch.equal(sd[k].cpu(), sb[k].cpu()), k
    names = {id(p) for p in b.head_parameters()}
    assert all(id(p) in names for p in list(b.keypoint_head.parameters()) + list(b.keypoint_predictor.parameters()))
    shims.install()
    try:
        from tvision import keypoint_rcnn
        assert hasattr(keypoint_rcnn, "keypointrcnn_resnet50_fpn") and hasattr(keypoint_rcnn, "KeypointRCNN")
    finally:
        shims.uninstall()
