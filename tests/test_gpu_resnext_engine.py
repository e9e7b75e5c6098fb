"""ResNeXt / wide ResNet bodies in the ResNet-FPN engines: RetinaNetEngine(body="resnext50_32x4d") and FasterRCNNEngine(body="wide_resnet50_2")
against tests/golden/g17_resnext.npz (C2..C5 of the reference's own models, tools/gen_resnext_golden.py) and against fp32 autograd of a
plain-torch restatement of the bottleneck body written here (groups inferred from the weight shapes)."""
from unittest import mock

import numpy as np
import pytest

from oracle import retina_oracle as ro

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F      # noqa: E402


def dev():
    return torch.device("cuda:0")


def nchw(a):
    return a.buf.float().permute(0, 3, 1, 2).cpu()


def cos(a, b):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm() + 1e-30))


def grouped_bottleneck(x, sd, q, stride):
    """conv1 1x1 -> width, conv2 3x3 (stride, groups = channels / weight.shape[1]), conv3 1x1 -> 4 * planes, each with its frozen affine; the
    identity goes through the strided 1x1 projection where the block has one."""
    def cba(t, conv, bn, relu=True, **kw):
        w = sd[f"{q}.{conv}.weight"]
        t = ro.frozen_bn(F.conv2d(t, w, groups=t.shape[1] // w.shape[1], **kw), sd, f"{q}.{bn}")
        return F.relu(t) if relu else t
    out = cba(x, "conv1", "bn1")
    out = cba(out, "conv2", "bn2", stride=stride, padding=1)
    out = cba(out, "conv3", "bn3", relu=False)
    idn = cba(x, "downsample.0", "downsample.1", relu=False, stride=stride) if f"{q}.downsample.0.weight" in sd else x
    return F.relu(out + idn)


def restated(fn, *a, **k):
    """oracle forward with the bottleneck above in place of the groups = 1 one."""
    with mock.patch.object(ro, "bottleneck", grouped_bottleneck):
        return fn(*a, **k)


def state_for(golden, body, tail_keys):
    """det_fill over the fixture's body keys in state_dict order (seed + position, as the generator filled the reference model), then over the
    FPN / head keys."""
    g = golden("g17_resnext")
    seed = int(g["seed"])
    keys = [(str(k), tuple(int(v) for v in row if v)) for k, row in zip(g["keys_" + body], g["shapes_" + body])] + list(tail_keys)
    return {k: torch.from_numpy(np.ascontiguousarray(ro.det_fill(k, shp, seed + i))) for i, (k, shp) in enumerate(keys)}


def make(golden, model):
    from object_detectors_amd.tvision.engine import FasterRCNNEngine, RetinaNetEngine
    if model == "retinanet":
        body = "resnext50_32x4d"
        sd = state_for(golden, body, ro.fpn_keys() + ro.head_keys())
        eng = RetinaNetEngine(91, 9, 3, device=dev(), seed=0, normalize=False, body=body)
    else:
        body = "wide_resnet50_2"
        sd = state_for(golden, body, ro.frcnn_state_keys()[len(ro.body_keys()):])
        eng = FasterRCNNEngine(3, device=dev(), seed=0, normalize=False, body=body)
    eng.load_reference_state_dict(sd)
    return eng, sd, body, torch.from_numpy(golden("g17_resnext")["input"])


@pytest.fixture(scope="module")
def retina(golden):
    return make(golden, "retinanet")


@pytest.fixture(scope="module")
def frcnn(golden):
    return make(golden, "fasterrcnn")


@pytest.mark.parametrize("which", ["retina", "frcnn"])
def test_state_dict_roundtrip(which, request):
    eng, sd, _body, _x = request.getfixturevalue(which)
    out = eng.reference_state_dict()
    assert list(out.keys()) == list(sd.keys())
    for k, v in sd.items():
        assert torch.equal(out[k].cpu(), v), k


@pytest.mark.parametrize("which", ["retina", "frcnn"])
def test_forward_matches_reference_fixture(which, request, golden):
    """C2..C5 against the samples of the reference's own model at the engine tolerance of tests/test_gpu_retina_engine.py (rel < 4e-2 of the
    map's maximum)."""
    eng, _sd, body, x = request.getfixturevalue(which)
    g = golden("g17_resnext")
    eng.forward(x.to(dev()), training=False)
    torch.cuda.synchronize()
    for li, a in enumerate(eng._last_plan.body, 2):
        got, want = ro.sample(nchw(a)), g[f"c{li}_{body}"]
        r = float(np.abs(got - want).max()) / float(g[f"c{li}_max_{body}"])
        print(body, f"C{li}", "rel", r)
        assert r < 4e-2, (body, li, r)


def grads_against_autograd(eng, sd, loss_of):
    sdg = {k: v.clone() for k, v in sd.items()}
    train = [s for s in eng.specs if s.trainable]
    for s in train:
        sdg[s.name + ".weight"].requires_grad_(True)
        if s.bias:
            sdg[s.name + ".bias"].requires_grad_(True)
    loss_of(sdg).backward()
    return sdg, train


def check_grads(eng, sdg, train):
    got = eng.reference_state_dict(grads=True)
    assert "backbone.body.layer1.0.conv2.weight" not in got          # frozen at trainable_layers = 3
    worst = (2.0, None)
    for s in train:
        for suffix in ([".weight", ".bias"] if s.bias else [".weight"]):
            k = s.name + suffix
            g, r = got[k].cpu(), sdg[k].grad
            c, ratio = cos(g, r), float(g.double().norm() / (r.double().norm() + 1e-30))
            worst = min(worst, (c, k))
            assert c > 0.94 and 0.9 < ratio < 1.1, (k, c, ratio)
    print("lowest cosine", worst)


def test_backward_wiring_retinanet_resnext(retina):
    from oracle import detrand
    eng, sd, _body, x = retina
    assert any(s.groups == 32 and s.trainable for s in eng.specs) and any(s.groups == 32 and not s.trainable for s in eng.specs)
    cot = {}

    def loss_of(sdg):
        ref = restated(ro.forward, sdg, x, do_normalize=False)
        cot["c1"] = torch.from_numpy(detrand.uniform(11, tuple(ref["cls_logits"].shape), -1.0, 1.0)) * 1e-2
        cot["c2"] = torch.from_numpy(detrand.uniform(12, tuple(ref["bbox_regression"].shape), -1.0, 1.0)) * 1e-2
        return (ref["cls_logits"] * cot["c1"]).sum() + (ref["bbox_regression"] * cot["c2"]).sum()
    sdg, train = grads_against_autograd(eng, sd, loss_of)
    eng.forward(x.to(dev()), training=True)
    eng.backward(cot["c1"].to(dev()), cot["c2"].to(dev()))
    torch.cuda.synchronize()
    check_grads(eng, sdg, train)


def test_backward_wiring_fasterrcnn_wide(frcnn):
    from oracle import detrand
    eng, sd, _body, x = frcnn
    assert all(s.groups == 1 for s in eng.specs) and eng.by_name["backbone.body.layer2.0.conv2"].cin == 256
    cot = {}

    def loss_of(sdg):
        ref = restated(ro.frcnn_forward, sdg, x, do_normalize=False)
        cot["c1"] = torch.from_numpy(detrand.uniform(11, tuple(ref["objectness"].shape), -1.0, 1.0)) * 1e-2
        cot["c2"] = torch.from_numpy(detrand.uniform(12, tuple(ref["deltas"].shape), -1.0, 1.0)) * 1e-2
        cot["cf"] = [torch.from_numpy(detrand.uniform(20 + i, tuple(f.shape), -1.0, 1.0)) * 1e-3 for i, f in enumerate(ref["features"][:4])]
        return (ref["objectness"] * cot["c1"]).sum() + (ref["deltas"] * cot["c2"]).sum() + sum(
            (f * c).sum() for f, c in zip(ref["features"][:4], cot["cf"]))
    sdg, train = grads_against_autograd(eng, sd, loss_of)
    eng.forward(x.to(dev()), training=True)
    eng.backward(cot["c1"].to(dev()), cot["c2"].to(dev()), [c.to(dev()) for c in cot["cf"]])
    torch.cuda.synchronize()
    check_grads(eng, sdg, train)


def test_weight_refresh_repacks_grouped_weights(retina):
    """The optimizers update eng.params in place and signal nothing: every training forward repacks the trainable weights on its stream.  A
    grouped weight set to zero must therefore give conv2 output relu(0 * scale + shift) = relu(shift) in the very next forward."""
    eng, sd, _body, x = retina
    name = "backbone.body.layer3.1.conv2"
    s = eng.by_name[name]
    assert s.groups == 32 and s.trainable
    eng.forward(x.to(dev()), training=True)
    before = eng._last_plan.layers[name][0]["a"].buf.clone()
    eng.params[name + ".weight"].zero_()
    try:
        eng.forward(x.to(dev()), training=True)
        torch.cuda.synchronize()
        a = eng._last_plan.layers[name][0]["a"]
        want = torch.relu(eng.affine[s.bn][1]).bfloat16().view(1, 1, 1, -1).expand_as(a.buf)
        assert torch.equal(a.buf, want)
        assert not torch.equal(before, a.buf)
    finally:
        eng.load_reference_state_dict(sd)


def test_fasterrcnn_model_with_resnext_body():
    """Model layer smoke test (not parity): one training and one eval call of FasterRCNN(body="resnext50_32x4d") on two 64 x 96 images."""
    from object_detectors_amd.tvision.frcnn import FasterRCNN
    torch.manual_seed(0)
    m = FasterRCNN(num_classes=21, device=dev(), body="resnext50_32x4d", min_size=64, max_size=96, rpn_pre_nms_top_n_train=200,
                   rpn_post_nms_top_n_train=100, rpn_pre_nms_top_n_test=200, rpn_post_nms_top_n_test=50, box_batch_size_per_image=32,
                   box_score_thresh=0.0)
    imgs = [torch.rand((3, 64, 96), device=dev()) for _ in range(2)]
    t = [{"boxes": torch.tensor([[8.0, 10.0, 60.0, 50.0], [30.0, 20.0, 90.0, 60.0]], device=dev()), "labels": torch.tensor([5, 17], device=dev())}
         for _ in range(2)]
    m.train()
    losses = m(imgs, t)
    torch.cuda.synchronize()
    assert set(losses) == {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"}
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    g = m.engine.reference_state_dict(grads=True)
    assert float(g["backbone.body.layer4.2.conv2.weight"].abs().max()) > 0 and bool(torch.isfinite(m.engine.flat_g).all())
    m.eval()
    det = m(imgs)
    assert len(det) == 2 and all(set(d) == {"boxes", "labels", "scores"} for d in det)
    for d in det:
        assert d["boxes"].shape[0] == d["scores"].shape[0] == d["labels"].shape[0] <= 100
        assert bool(torch.isfinite(d["boxes"]).all()) and (d["boxes"].shape[0] == 0 or bool((d["labels"] >= 1).all()))
