"""Grouped 3x3 convolution (csrc/gconv_kernels.hip: mi355det_gconv_*) against torch.nn.functional.conv2d(groups=g) in fp32 on the CPU, on the
same bf16-rounded operands, and its autograd.  Tolerance of the project's conv parity tests: 2e-2 * max|ref| (tests/test_gpu_resnet.py)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F      # noqa: E402

GROUPS = 32
TOL = 2e-2
SENTINEL = 7.0


def dev():
    return torch.device("cuda:0")


def bf(t):
    return t.bfloat16().float()


def pitched(t_nhwc, ld, fill=SENTINEL):
    """[n,h,w,c] fp32 (CPU) -> bf16 device buffer [n,h,w,ld] whose first c channels hold t, the rest the sentinel."""
    n, h, w, c = t_nhwc.shape
    buf = torch.full((n, h, w, ld), fill, dtype=torch.bfloat16, device=dev())
    buf[..., :c] = t_nhwc.to(dev()).bfloat16()
    return buf


def run_case(cpg, n, h, w, stride, in_pad=0, out_pad=0, affine=False, seed=0, x=None, wt=None, dy=None, groups=GROUPS):
    """Forward, data gradient and weight gradient of one shape on the GPU and the fp32 CPU reference on the same rounded operands."""
    from object_detectors_amd import ops
    c = cpg * groups
    g = torch.Generator().manual_seed(1000 * cpg + 10 * h + stride + seed)
    if x is None:
        x = bf(torch.randn((n, c, h, w), generator=g))
    if wt is None:
        wt = bf(torch.randn((c, cpg, 3, 3), generator=g) * (2.0 / (9 * cpg)) ** 0.5)
    scale = (torch.rand(c, generator=g) + 0.5) if affine else None
    shift = (torch.rand(c, generator=g) - 0.5) if affine else None
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    z = F.conv2d(xr, wr, stride=stride, padding=1, groups=groups)
    ref_y = torch.relu(z * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)) if affine else z
    if dy is None:
        dy = bf(torch.randn(tuple(z.shape), generator=g))
    z.backward(dy)
    ho, wo = z.shape[2:]

    shp = ops.gconv_shape(n, h, w, c, stride, in_ld=c + in_pad, out_ld=c + out_pad)
    assert (shp.ho, shp.wo) == (ho, wo)
    wf, wd = ops.gconv_pack(shp, groups, wt.to(dev()))
    wf2, wd2 = ops.gconv_pack(shp, groups, wt.permute(0, 2, 3, 1).contiguous().to(dev()), ohwi=True)
    assert torch.equal(wf, wf2) and torch.equal(wd, wd2)                     # OIHW and OHWI masters give the same images
    xd = pitched(x.permute(0, 2, 3, 1), c + in_pad)
    yd = torch.full((n, ho, wo, c + out_pad), SENTINEL, dtype=torch.bfloat16, device=dev())
    ops.gconv_fwd(shp, groups, xd, wf, yd, scale.to(dev()) if affine else None, shift.to(dev()) if affine else None, relu=affine)
    dyd = pitched(dy.permute(0, 2, 3, 1), c + out_pad)
    dxd = torch.full((n, h, w, c + in_pad), SENTINEL, dtype=torch.bfloat16, device=dev())
    ops.gconv_dgrad(shp, groups, dyd, wd, dxd)
    dw = torch.full((c, 3, 3, cpg), SENTINEL, device=dev())
    dw2 = torch.full((c, 3, 3, cpg), -SENTINEL, device=dev())
    ops.gconv_wgrad(shp, groups, xd, dyd, dw)
    ops.gconv_wgrad(shp, groups, xd, dyd, dw2)
    torch.cuda.synchronize()
    return dict(shape=shp, c=c, y=yd.float().cpu(), dx=dxd.float().cpu(), dw=dw.cpu(), dw2=dw2.cpu(), ref_y=ref_y.detach().permute(0, 2, 3, 1),
                ref_dx=xr.grad.permute(0, 2, 3, 1), ref_dw=wr.grad.permute(0, 2, 3, 1), xd=xd, dyd=dyd)


def close(got, ref, what):
    err, bound = float((got - ref).abs().max()), TOL * float(ref.abs().max())
    print(what, "max err", err, "bound", bound)
    assert float(ref.abs().max()) > 0 and err <= bound, (what, err, bound)


def check_case(r):
    c = r["c"]
    close(r["y"][..., :c], r["ref_y"], "fwd")
    close(r["dx"][..., :c], r["ref_dx"], "dgrad")
    close(r["dw"], r["ref_dw"], "wgrad")
    assert torch.equal(r["dw"], r["dw2"])                                    # fixed summation order: bit-identical from call to call
    assert bool((r["y"][..., c:] == SENTINEL).all()) and bool((r["dx"][..., c:] == SENTINEL).all())      # pitch padding survives


# channels per group 4 .. 64 with 32 groups (C = 128 .. 2048); tiny maps at the wide end.  Geometry: both strides; n = 2; an odd, non-square map
# (13 x 19 -> 7 x 10 at stride 2: two tiles in both directions, partial tiles, odd sizes for the stride-2 data gradient); a map smaller than a
# tile (3 x 5); an even map at stride 2.  Pitches: dense, 16-byte aligned padding (+8 / +16), and odd padding (+3 / +5: the 2-byte path).
CASES = [
    # cpg, n, h, w, stride, in_pad, out_pad, affine
    (4, 2, 13, 19, 1, 0, 0, False),
    (4, 2, 13, 19, 2, 8, 16, True),
    (4, 1, 3, 5, 1, 3, 5, True),
    (8, 2, 13, 19, 2, 0, 0, False),
    (8, 1, 10, 34, 1, 16, 8, True),
    (8, 2, 3, 5, 2, 0, 0, False),
    (16, 1, 12, 20, 2, 3, 5, True),
    (16, 2, 9, 17, 1, 0, 0, False),
    (32, 1, 7, 7, 1, 0, 8, True),
    (32, 1, 7, 7, 2, 8, 0, False),
    (64, 1, 7, 7, 1, 0, 0, True),
    (64, 1, 7, 7, 2, 8, 8, False),
    (64, 2, 5, 18, 1, 0, 0, False),
]


@pytest.mark.parametrize("cpg,n,h,w,stride,in_pad,out_pad,affine", CASES)
def test_parity(cpg, n, h, w, stride, in_pad, out_pad, affine):
    check_case(run_case(cpg, n, h, w, stride, in_pad, out_pad, affine))


def test_workspace_one_byte_short():
    from object_detectors_amd import ops
    from object_detectors_amd._lib import lib, ptr, stream_ptr
    r = run_case(8, 1, 9, 9, 1)
    shp = r["shape"]
    need = lib().mi355det_gconv_wgrad_workspace(C.byref(shp), GROUPS)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev())
    dw = torch.full((r["c"], 3, 3, 8), SENTINEL, device=dev())
    st = lib().mi355det_gconv_wgrad(C.byref(shp), GROUPS, ptr(r["xd"]), ptr(r["dyd"]), ptr(dw), ptr(ws), need - 1, stream_ptr())
    assert st == -3                                                          # MI355DET_EWORKSPACE
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all())                                      # nothing was launched
    ops.gconv_wgrad(shp, GROUPS, r["xd"], r["dyd"], dw, workspace=ws)
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), r["dw"])


# a group in the middle of a 32-channel bundle, the last group of a bundle and the first of the next one
@pytest.mark.parametrize("cpg,group", [(4, 3), (4, 7), (4, 8), (16, 1), (16, 2), (64, 5)])
@pytest.mark.parametrize("stride", [1, 2])
def test_group_isolation_exact(cpg, group, stride):
    c = cpg * GROUPS
    n, h, w = 1, 9, 11
    g = torch.Generator().manual_seed(cpg + group)
    lo, hi = group * cpg, (group + 1) * cpg
    x = torch.zeros((n, c, h, w))
    x[:, lo:hi] = bf(torch.randn((n, cpg, h, w), generator=g))
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    dy = torch.zeros((n, c, ho, wo))
    dy[:, lo:hi] = bf(torch.randn((n, cpg, ho, wo), generator=g))
    r = run_case(cpg, n, h, w, stride, x=x, dy=dy)
    other = torch.ones(c, dtype=torch.bool)
    other[lo:hi] = False
    assert float(r["y"][..., :c][..., other].abs().max()) == 0.0 and float(r["y"][..., lo:hi].abs().max()) > 0
    assert float(r["dx"][..., :c][..., other].abs().max()) == 0.0 and float(r["dx"][..., lo:hi].abs().max()) > 0
    dwo = r["dw"].clone()
    dwo[lo:hi] = 0
    assert float(dwo.abs().max()) == 0.0 and float(r["dw"][lo:hi].abs().max()) > 0
    check_case(r)


@pytest.mark.parametrize("cpg,stride", [(4, 1), (8, 2), (16, 1), (32, 2), (64, 1)])
def test_exact_arithmetic(cpg, stride):
    """Operands in {-1, 0, 1}, sparse enough that every reference value is an integer of magnitude <= 256: exactly representable in bf16
    and every partial sum exact in fp32, so forward, dx and dw must be bit-equal to the reference in any summation order."""
    c = cpg * GROUPS
    n, h, w = 2, 7, 9
    g = torch.Generator().manual_seed(77 + cpg)

    def tern(shape, density):
        return (torch.rand(shape, generator=g) < density).float() * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
    ho, wo = (h - 1) // stride + 1, (w - 1) // stride + 1
    r = run_case(cpg, n, h, w, stride, x=tern((n, c, h, w), 0.3), wt=tern((c, cpg, 3, 3), 0.3), dy=tern((n, c, ho, wo), 0.3))
    for k in ("ref_y", "ref_dx", "ref_dw"):
        assert 0 < float(r[k].abs().max()) <= 256, (k, float(r[k].abs().max()))
    assert torch.equal(r["y"][..., :c], r["ref_y"])
    assert torch.equal(r["dx"][..., :c], r["ref_dx"])
    assert torch.equal(r["dw"], r["ref_dw"]) and torch.equal(r["dw"], r["dw2"])


def test_refusals():
    """Unsupported arguments return MI355DET_EINVAL before any launch (the output keeps its sentinel)."""
    from object_detectors_amd import _lib, ops
    from object_detectors_amd._lib import lib, ptr, stream_ptr
    L = lib()
    x = torch.zeros((1, 8, 8, 256), dtype=torch.bfloat16, device=dev())
    y = torch.full((1, 8, 8, 256), SENTINEL, dtype=torch.bfloat16, device=dev())
    wimg = torch.zeros(9 * 64 * 256, dtype=torch.bfloat16, device=dev())
    wm = torch.zeros(256 * 9 * 64, device=dev())
    dw = torch.full((256 * 9 * 64,), SENTINEL, device=dev())
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=dev())
    e0 = _lib.ConvEpilogue(None, None, None, 0, 0, 0)
    good = ops.gconv_shape(1, 8, 8, 256, 1)
    bad = [
        (good, 48),                                            # groups does not divide cin
        (good, 128),                                           # 2 channels per group
        (ops.conv_shape(1, 8, 8, 256, 256, 1, 1), 32),         # ksize 1
        (ops.conv_shape(1, 8, 8, 256, 128, 3, 1), 32),         # cin != cout
    ]
    for shp, groups in bad:
        assert L.mi355det_gconv_pack_elems(C.byref(shp), groups) == 0
        assert L.mi355det_gconv_wgrad_workspace(C.byref(shp), groups) == 0
        assert L.mi355det_gconv_pack_weights(C.byref(shp), groups, ptr(wm), 0, ptr(wimg), None, stream_ptr()) == -1
        assert L.mi355det_gconv_fwd_ex(C.byref(shp), groups, ptr(x), ptr(wimg), C.byref(e0), ptr(y), 0, stream_ptr()) == -1
        assert L.mi355det_gconv_dgrad(C.byref(shp), groups, ptr(x), ptr(wimg), ptr(y), stream_ptr()) == -1
        assert L.mi355det_gconv_wgrad(C.byref(shp), groups, ptr(x), ptr(x), ptr(dw), ptr(ws), ws.numel(), stream_ptr()) == -1
    res = _lib.ConvEpilogue(None, None, ptr(x), 256, 0, 0)
    assert L.mi355det_gconv_fwd_ex(C.byref(good), 32, ptr(x), ptr(wimg), C.byref(res), ptr(y), 0, stream_ptr()) == -1      # residual
    assert L.mi355det_gconv_fwd_ex(C.byref(good), 32, ptr(x), ptr(wimg), C.byref(e0), ptr(y), 1, stream_ptr()) == -1       # fp32 output
    assert L.mi355det_gconv_fwd_ex(C.byref(good), 32, ptr(x), ptr(wimg), C.byref(e0), ptr(y), 0, stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all())
    assert float(y.float().abs().max()) == 0.0              # only the valid call wrote: zeros from zero operands
