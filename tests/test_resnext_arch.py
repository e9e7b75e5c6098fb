"""ResNeXt / wide ResNet bodies of the ResNet-FPN engines (tvision/engine.py arch, BODY_LAYERS, BODY_WIDTH) against the state_dict keys and
shapes of the reference's own models (tests/golden/g17_resnext.npz, written by tools/gen_resnext_golden.py).  CPU only."""
import pytest

torch = pytest.importorskip("torch")

from object_detectors_amd.tvision import engine as E      # noqa: E402
from oracle import retina_oracle as ro                    # noqa: E402

NEW_BODIES = ("resnext50_32x4d", "resnext101_32x8d", "wide_resnet50_2", "wide_resnet101_2")
BN = (".weight", ".bias", ".running_mean", ".running_var")


def body_keys_of(specs):
    """state_dict order of the body: conv weight, then its norm's four entries (the downsample pair comes after bn3 in the module,
    while arch() lists it after conv3 as well)."""
    out = []
    for s in specs:
        if s.name.startswith("backbone.body."):
            out.append(s.name + ".weight")
            out += [s.bn + k for k in BN]
    return out


def oihw(s):
    if s.name.endswith("body.conv1"):
        return (64, 3, 7, 7)
    return (s.cout, s.cin // s.groups, s.k, s.k)


@pytest.mark.parametrize("body", NEW_BODIES)
def test_arch_matches_reference_state_dict(golden, body):
    g = golden("g17_resnext")
    keys = [str(k) for k in g["keys_" + body]]
    shapes = {k: tuple(int(v) for v in row if v) for k, row in zip(keys, g["shapes_" + body])}
    specs = E.arch(body=body)
    assert body_keys_of(specs) == keys
    for s in specs:
        if s.name.startswith("backbone.body."):
            assert oihw(s) == shapes[s.name + ".weight"], s.name
            assert all(shapes[s.bn + k] == (s.cout,) for k in BN), s.name
    g32 = [s for s in specs if s.groups > 1]
    if body.startswith("resnext"):
        assert g32 and all(s.groups == 32 and s.k == 3 and s.cin == s.cout and s.name.endswith(".conv2") for s in g32)
    else:
        assert not g32


@pytest.mark.parametrize("body", NEW_BODIES)
def test_layout_params_maps_back_to_oihw(golden, body):
    """The flat fp32 buffers hold [cout, k, k, cin / groups]; _get_weight_oihw gives the reference's shape back."""
    g = golden("g17_resnext")
    shapes = {str(k): tuple(int(v) for v in row if v) for k, row in zip(g["keys_" + body], g["shapes_" + body])}
    eng = object.__new__(E.RetinaNetEngine)
    eng.device = torch.device("cpu")
    eng.specs = E.arch(body=body, trainable_layers=3)
    eng._layout_params()
    for s in eng.specs:
        if not s.name.startswith("backbone.body.") or s.name.endswith("body.conv1"):
            continue
        want = shapes[s.name + ".weight"]
        assert tuple(eng.params[s.name + ".weight"].shape) == (want[0], want[2], want[3], want[1]), s.name
        assert tuple(eng._get_weight_oihw(s, eng.params).shape) == want, s.name
        if s.groups > 1:
            wf, wd = eng.packed[s.name]
            assert wf.numel() == wd.numel() == 9 * max(32, s.cin // s.groups) * s.cin      # block-diagonal operand images
    assert tuple(eng._get_weight_oihw(eng.specs[0], eng.params).shape) == (64, 3, 7, 7)


@pytest.mark.parametrize("body", ("resnet50", "resnet101", "resnet152"))
def test_existing_bodies_unchanged(body):
    specs = E.arch(body=body)
    want = ro.body_keys(layers=E.BODY_LAYERS[body])
    assert body_keys_of(specs) == [k for k, _ in want]
    shapes = dict(want)
    for s in specs:
        if s.name.startswith("backbone.body."):
            assert oihw(s) == shapes[s.name + ".weight"] and s.groups == 1, s.name


def test_unknown_body_fails_as_before():
    with pytest.raises(KeyError):
        E.arch(body="resnext50_64x4d")
