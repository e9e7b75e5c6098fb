"""Every tunable convolution kernel and epilogue against exact references (the cases of tests/conv_matrix.py, both storage formats).

(a) Exact-grid operands: x, dy are integers in [-8, 8] * 2^-3, w integers in [-8, 8] * 2^-5, scales powers of two, shifts / residuals on the
    2^-8 grid.  Every product is then a multiple of 2^-8 (2^-9 after a scale of 1/2) and the sums of their magnitudes stay far below 2^15,
    so fp32 accumulation is exact in ANY order: every tile order, split count and split-K form must produce the same fp32 sum, and the
    stored 16-bit value is the round-to-nearest-even of the fp64 reference, applied in the order the route's epilogue documents
    (include/mi355det.h: conv_dgrad / conv_dgrad_ws).  Outputs are compared BIT for bit.
(b) Realistic operands (Gaussian, input-channel scales over 2^+-8, borders scaled by 2^-12): per-element bound against fp64,
    |got - ref| <= u |ref| + gamma_K S (+ u (|round(acc)| + |res|) where the epilogue rounds twice), S = fp64 conv of |x| and |w|.
(c) Memory contract: pitch padding of every input holds NaN, outputs start as a NaN sentinel; every real element must be written, pad
    channels and the gaps between fp32 head images must keep the sentinel.

Strict mode (debug key 9) is on for every case: a forced configuration the launch does not honour fails instead of running another kernel.
"""
import ctypes as C
import functools
import zlib

import pytest

from tests import conv_matrix as MX

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402
from torch.nn.grad import conv2d_input, conv2d_weight  # noqa: E402

NAN16 = -1                                        # 0xFFFF: NaN in bf16 and in fp16
SENT16 = {"bf16": 0x7FC1, "fp16": 0x7E01}         # quiet NaNs with a payload: "never written"
SENT32 = 0x7FC00001
U = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
SLOPE = 0.1
EXACT_IDS = {1, 2, 3, 4, 5, 6, 15, 16, 17, 18, 19, 26, 27, 28, 29, 30, 31, 40}      # tiles of whole 128-pixel rows: per-row statistics


def dev():
    return torch.device("cuda:0")


def L(storage):
    from object_detectors_amd import _lib
    return _lib.storage_lib(storage)


def check(st, what):
    from object_detectors_amd import _lib
    assert st == 0, f"{what}: {st} {_lib.lib().mi355det_last_error().decode()}"


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def conv_shape(sh):
    from object_detectors_amd import _lib
    ho, wo = MX.out_hw(sh)
    return _lib.ConvShape(sh.n, sh.h, sh.w, sh.cin, ho, wo, sh.cout, sh.k, sh.s, (sh.k - 1) // 2, sh.cin + sh.xpad, sh.cout + sh.ypad)


def rnd16(t, storage):
    """fp64 (exactly representable in fp32) -> round to nearest even in the storage format -> fp64."""
    return t.float().to(DTYPE[storage]).double()


def bits16(t, storage):
    return t.float().to(DTYPE[storage]).view(torch.int16)


def f32mul(a, b):
    return (a.float() * torch.tensor(b, dtype=torch.float32)).double()


# ------------------------------------------------------------------------------------------------------------------------- operands
def grid_ints(shape, lo, hi, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, dtype=torch.int64).double()


def realistic(shape, seed, chan_axis, storage, border=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(shape, generator=g, dtype=torch.float64)
    sc = 2.0 ** torch.randint(-8, 9, (shape[chan_axis],), generator=g).double()
    v = v * sc.view([-1 if i == chan_axis else 1 for i in range(len(shape))])
    if border:      # NHWC: border rows and columns at 2^-12
        v[:, 0] *= 2.0 ** -12
        v[:, -1] *= 2.0 ** -12
        v[:, :, 0] *= 2.0 ** -12
        v[:, :, -1] *= 2.0 ** -12
    return rnd16(v, storage)


@functools.lru_cache(maxsize=None)
def operands(case_name, kind):
    """Exact-grid operands of a case (storage independent: every value is exact in bf16 and fp16).  NHWC activations, OIHW weights."""
    c = next(cc for cc in MX.CASES if cc.name == case_name)
    sh = c.shape
    ho, wo = MX.out_hw(sh)
    seed = zlib.crc32(case_name.encode())
    o = {"x": grid_ints((sh.n, sh.h, sh.w, sh.cin), -8, 8, seed) / 8, "w": grid_ints((sh.cout, sh.cin, sh.k, sh.k), -8, 8, seed + 1) / 32,
         "dy": grid_ints((sh.n, ho, wo, sh.cout), -8, 8, seed + 2) / 8}
    ocout = sh.cout if c.entry.startswith("fwd") else sh.cin
    o["scale"] = 2.0 ** grid_ints((ocout,), -1, 1, seed + 3)
    o["shift"] = grid_ints((ocout,), -255, 255, seed + 4) / 256
    o["bias"] = o["shift"]
    oh, ow = (ho, wo) if c.entry.startswith("fwd") else (sh.h, sh.w)
    o["res"] = grid_ints((sh.n, oh, ow, ocout), -255, 255, seed + 5) / 256
    o["act"] = grid_ints((sh.n, sh.h, sh.w, sh.cin), -3, 3, seed + 6) / 8          # zeros and negatives: the mask
    o["z"] = grid_ints((sh.n, sh.h, sh.w, sh.cin), -16, 16, seed + 7) / 8
    o["ss"] = torch.cat([2.0 ** grid_ints((sh.cin,), -1, 1, seed + 8), grid_ints((sh.cin,), -64, 64, seed + 9) / 64,
                         grid_ints((sh.cin,), -8, 8, seed + 10) / 8, 2.0 ** grid_ints((sh.cin,), -1, 1, seed + 11)])
    o["dw0"] = grid_ints((sh.cout, sh.k, sh.k, sh.cin), -4, 4, seed + 12) / 64         # dw / dbias are accumulated into (+=)
    o["db0"] = grid_ints((sh.cout,), -4, 4, seed + 13) / 64
    return o


@functools.lru_cache(maxsize=None)
def reference(case_name, kind, storage):
    """fp64 GEMM part of a case and S = the same operation on magnitudes: fwd -> [n,ho,wo,cout], dgrad -> [n,h,w,cin], wgrad -> [cout,k,k,cin]."""
    c = next(cc for cc in MX.CASES if cc.name == case_name)
    sh = c.shape
    ho, wo = MX.out_hw(sh)
    if kind == "exact":
        o = operands(case_name, kind)
    else:
        seed = zlib.crc32(case_name.encode()) + 99
        o = dict(operands(case_name, "exact"))
        o["x"] = realistic((sh.n, sh.h, sh.w, sh.cin), seed, 3, storage, border=True)
        o["dy"] = realistic((sh.n, ho, wo, sh.cout), seed + 1, 3, storage, border=True)
        o["w"] = rnd16(torch.randn((sh.cout, sh.cin, sh.k, sh.k), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64)
                       / (sh.k * (sh.cin ** 0.5)), storage)
        o["res"] = realistic(tuple(o["res"].shape), seed + 3, 3, storage)
        o["bias"] = torch.randn(o["bias"].shape, generator=torch.Generator().manual_seed(seed + 4), dtype=torch.float64).float().double()
    pad = (sh.k - 1) // 2
    x, w, dy = o["x"].permute(0, 3, 1, 2), o["w"], o["dy"].permute(0, 3, 1, 2)

    def run(x, w, dy):
        if c.entry.startswith("fwd"):
            return F.conv2d(x, w, stride=sh.s, padding=pad).permute(0, 2, 3, 1)
        if c.entry == "wgrad":
            return conv2d_weight(x, tuple(w.shape), dy, stride=sh.s, padding=pad).permute(0, 2, 3, 1)
        return conv2d_input(tuple(x.shape), w, dy, stride=sh.s, padding=pad).permute(0, 2, 3, 1)
    acc = run(x, w, dy).contiguous()
    S = run(x.abs(), w.abs(), dy.abs()).contiguous()
    return o, acc, S


def assert_premise(o, S, q):
    """(a) holds only if every product is a multiple of 2^-q and sum |products| < 2^(24-q)."""
    for k, e in (("x", 3), ("dy", 3), ("w", 5)):
        v = o[k] * 2.0 ** e
        assert torch.equal(v, v.round()), k
    assert S.max().item() < 2.0 ** (24 - q), S.max().item()


# ------------------------------------------------------------------------------------------------------------------------- buffers
def nhwc_buf(vals, ld, storage, fill=NAN16):
    """fp64 NHWC values -> device 16-bit buffer with pixel pitch ld; pad lanes hold `fill` (bits)."""
    n, h, w, c = vals.shape
    b = torch.full((n, h, w, ld), fill, dtype=torch.int16)
    b[..., :c] = bits16(vals, storage)
    return b.to(dev()).view(DTYPE[storage])


def sentinel16(shape, storage):
    return torch.full(shape, SENT16[storage], dtype=torch.int16, device=dev()).view(DTYPE[storage])


def sentinel32(shape):
    return torch.full(shape, SENT32, dtype=torch.int32, device=dev()).view(torch.float32)


def pack(Lb, cs, w, cout_pad, storage, want_dgrad=True):
    wm = w.float().contiguous().to(dev())
    wf = torch.empty(cout_pad * cs.ksize * cs.ksize * cs.cin, dtype=DTYPE[storage], device=dev())
    wd = torch.empty(Lb.mi355det_dgrad_pack_elems(C.byref(cs)), dtype=DTYPE[storage], device=dev()) if want_dgrad else None
    check(Lb.mi355det_pack_weights(C.byref(cs), vp(wm), 0, vp(wf), cout_pad, vp(wd), stream()), "pack_weights")
    return wf, wd


def dgrad_ksplit(sh):
    """conv_kernels.hip: dgrad_ksplit (> 1: mi355det_conv_dgrad_ws takes the split-K route)."""
    if sh.s != 1:
        return 0
    cin_pad = (sh.cin + 31) // 32 * 32
    if cin_pad % 128 or sh.cout % 64 or (sh.cin + sh.xpad) % 8:
        return 0
    M, K = sh.n * sh.h * sh.w, sh.k * sh.k * sh.cout
    tiles = (M + 127) // 128 * (cin_pad // 128)
    if tiles > 96 or K < 8192:
        return 0
    chunks, best = sh.cout // 64, 0
    for d in range(2, chunks + 1):
        if chunks % d == 0 and tiles * d <= 512 and chunks // d >= 4:
            best = d
    return best


def rounds_once(c):
    """Routes whose epilogue adds the residual to the fp32 sum and rounds once (include/mi355det.h: conv_dgrad / conv_dgrad_ws)."""
    return (c.entry == "dgrad" and c.opts.get("s2") == "single") or (c.entry == "dgrad_ws" and dgrad_ksplit(c.shape) >= 2)


class Knobs:
    """Strict mode + the forcing keys of a case; everything restored on exit."""

    def __init__(self, storage, c):
        self.Lb, self.c = L(storage), c

    def __enter__(self):
        Lb, o = self.Lb, self.c.opts
        Lb.mi355det_debug_set(9, 1)
        Lb.mi355det_debug_set(0, self.c.cfg)
        s2 = o.get("s2")
        Lb.mi355det_debug_set(5, {"four": 0, "cat": 1}.get(s2, -1))
        Lb.mi355det_debug_set(2, 1 if s2 in ("four", "cat") else 0)
        Lb.mi355det_debug_set(7, o.get("split", 0))
        return self

    def __exit__(self, *a):
        for k, v in ((9, 0), (0, 0), (5, -1), (2, 0), (7, 0)):
            self.Lb.mi355det_debug_set(k, v)


# ------------------------------------------------------------------------------------------------------------------------- one case
def run_case(c, storage, kind):
    """Runs case c on the GPU with the operands of `kind` ("exact" / "real").  Returns (outputs dict, operands, acc, S)."""
    sh = c.shape
    Lb = L(storage)
    cs = conv_shape(sh)
    o, acc, S = reference(c.name, kind, storage if kind == "real" else None)
    ho, wo = cs.ho, cs.wo
    fwd = c.entry.startswith("fwd")
    cp = c.opts.get("cout_pad") or MX.cout_pad_of(sh.cout)
    wf, wd = pack(Lb, cs, o["w"], cp, storage, want_dgrad=not fwd and c.entry != "wgrad")
    out = {}
    with Knobs(storage, c):
        if fwd:
            x = nhwc_buf(o["x"], cs.in_ld, storage)
            f32 = c.entry in ("fwd_f32", "fwd_ex_f32")
            img = ho * wo * cs.out_ld + (3 * cs.out_ld + 4 if c.opts.get("image_stride") else 0)
            y = sentinel32((sh.n, img)) if f32 else sentinel16((sh.n, ho, wo, cs.out_ld), storage)
            if c.entry in ("fwd", "fwd_stats", "fwd_f32"):
                stats = None
                if c.entry == "fwd_stats":
                    rows = Lb.mi355det_conv_stats_rows(C.byref(cs), cp)
                    stats = sentinel32((rows + 64, 2, cp))
                bias = o["bias"].float().to(dev()) if c.opts.get("bias") else None
                check(Lb.mi355det_conv_fwd(C.byref(cs), vp(x), vp(wf), vp(bias), vp(y), int(f32), vp(stats), cp, stream()), c.entry)
                out["stats"] = stats
            else:
                from object_detectors_amd import _lib
                sc = o["scale"].float().to(dev()) if c.opts.get("scale") else None
                sf = o["shift"].float().to(dev()) if c.opts.get("shift") else None
                res = nhwc_buf(o["res"], sh.cout + sh.rpad, storage) if c.opts.get("res") else None
                e = _lib.ConvEpilogue(vp(sc), vp(sf), vp(res), sh.cout + sh.rpad if res is not None else 0, c.opts.get("relu", 0),
                                      img if c.opts.get("image_stride") else 0, SLOPE)
                check(Lb.mi355det_conv_fwd_ex(C.byref(cs), vp(x), vp(wf), C.byref(e), vp(y), int(f32), cp, stream()), c.entry)
            out["y"] = y
        elif c.entry == "wgrad":
            x = nhwc_buf(o["x"], cs.in_ld, storage)
            dy = nhwc_buf(o["dy"], cs.out_ld, storage)
            dw = o["dw0"].reshape(sh.cout, -1).float().to(dev())
            db = o["db0"].float().to(dev()) if c.opts["dbias"] else None
            sp = c.opts["split"] & (MX.WGRAD_FORM8 - 1)
            tiles = ((sh.cout + 127) // 128) * ((sh.k * sh.k * sh.cin + 127) // 128)
            nbytes = sp * tiles * 128 * 128 * 4 if sp > 1 else 1 << 20
            ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev())       # NaN: every slab element the fold reads must be written
            check(Lb.mi355det_conv_wgrad(C.byref(cs), vp(x), vp(dy), vp(dw), vp(db), vp(ws), nbytes, stream()), "conv_wgrad")
            out["dw"], out["db"] = dw, db
        else:
            dy = nhwc_buf(o["dy"], cs.out_ld, storage)
            dx = sentinel16((sh.n, sh.h, sh.w, cs.in_ld), storage)
            rld = sh.cin + sh.rpad
            res = nhwc_buf(o["res"], rld, storage) if c.opts.get("res") else None
            if c.entry == "dgrad":
                check(Lb.mi355det_conv_dgrad(C.byref(cs), vp(dy), vp(wd), vp(dx), vp(res), rld if res is not None else 0, stream()), "dgrad")
            elif c.entry == "dgrad_ws":
                nbytes = Lb.mi355det_conv_dgrad_workspace(C.byref(cs))
                ws = torch.full((max(nbytes, 16),), 0xFF, dtype=torch.uint8, device=dev())
                check(Lb.mi355det_conv_dgrad_ws(C.byref(cs), vp(dy), vp(wd), vp(dx), vp(res), rld if res is not None else 0, vp(ws), nbytes,
                                                stream()), "dgrad_ws")
            elif c.entry == "dgrad_mask":
                act = nhwc_buf(o["act"], sh.cin + sh.xpad, storage)
                sc = o["scale"].float().to(dev()) if c.opts["mask_scale"] else None
                check(Lb.mi355det_conv_dgrad_mask(C.byref(cs), vp(dy), vp(wd), vp(dx), vp(act), sh.cin + sh.xpad, vp(sc), c.opts["mask_relu"],
                                                  stream()), "dgrad_mask")
            elif c.entry == "dgrad_bn":
                z = nhwc_buf(o["z"], sh.cin + sh.rpad, storage)
                ss = o["ss"].float().to(dev())
                rows = Lb.mi355det_conv_dgrad_bn_rows(C.byref(cs))
                cin_pad = (sh.cin + 31) // 32 * 32
                part = sentinel32((rows + 64, 2, cin_pad))
                check(Lb.mi355det_conv_dgrad_bn(C.byref(cs), vp(dy), vp(wd), vp(dx), vp(res), rld if res is not None else 0, vp(z), sh.cin + sh.rpad,
                                                vp(ss), SLOPE, vp(part), stream()), "dgrad_bn")
                sums = torch.empty(2 * sh.cin, device=dev())
                check(L("bf16").mi355det_bn_bwd_sum_partials(vp(part), rows, sh.cin, cin_pad, vp(sums), stream()), "bn_bwd_sum_partials")
                out["sums"] = sums
            out["dx"] = dx
        torch.cuda.synchronize()
    return out, o, acc, S


def expected16(c, storage, o, acc):
    """Exact-grid expectation of a 16-bit output (fp64, values as stored) in the order the route's epilogue rounds."""
    r = functools.partial(rnd16, storage=storage)
    e, op = c.entry, c.opts
    if e in ("fwd", "fwd_stats"):
        return r(acc)
    if e == "fwd_ex":
        v = acc * (o["scale"] if op.get("scale") else 1.0) + (o["shift"] if op.get("shift") else 0.0)
        if op.get("relu") == 2:
            v = torch.where(v > 0, v, f32mul(v, SLOPE))
        t = r(v)
        if op.get("res") or op.get("relu") == 1:
            t = t + (o["res"] if op.get("res") else 0.0)
            if op.get("relu") == 1:
                t = t.clamp_min(0.0)
            t = r(t)
        return t
    if e == "dgrad_mask":
        t = r(acc) * (o["scale"] if op["mask_scale"] else 1.0)
        if op["mask_relu"]:
            t = torch.where(o["act"] > 0, t, torch.zeros_like(t))
        return r(t)
    if op.get("res"):
        return r(acc + o["res"]) if rounds_once(c) else r(r(acc) + o["res"])
    return r(acc)


def expected32(c, o, acc):
    op = c.opts
    if c.entry == "fwd_f32":
        return (acc + (o["bias"] if op.get("bias") else 0.0)).float().double()
    v = acc * (o["scale"] if op.get("scale") else 1.0) + (o["shift"] if op.get("shift") else 0.0)
    if op.get("relu") == 1:
        v = v.clamp_min(0.0)
    elif op.get("relu") == 2:
        v = torch.where(v > 0, v, f32mul(v, SLOPE))
    return v


def split_out(c, y, sh):
    """Device output -> (real part [n,oh,ow,C] on the CPU, the rest that must keep the sentinel, as a flat bit tensor)."""
    ho, wo = MX.out_hw(sh)
    cs = conv_shape(sh)
    if c.entry in ("fwd_f32", "fwd_ex_f32"):
        yb = y.view(torch.int32).cpu()
        body = yb[:, :ho * wo * cs.out_ld].reshape(sh.n, ho, wo, cs.out_ld)
        rest = torch.cat([body[..., sh.cout:].reshape(-1), yb[:, ho * wo * cs.out_ld:].reshape(-1)])
        return body[..., :sh.cout].contiguous(), rest
    yb = y.view(torch.int16).cpu()
    ch = sh.cout if c.entry.startswith("fwd") else sh.cin
    return yb[..., :ch].contiguous(), yb[..., ch:].reshape(-1)


def _ids(cases):
    return [c.name for c in cases]


# ------------------------------------------------------------------------------------------------------------------------- (a) + (c)
@pytest.mark.parametrize("storage", MX.STORAGES)
@pytest.mark.parametrize("case", MX.CASES, ids=_ids(MX.CASES))
def test_exact_grid_bit_exact(case, storage):
    c, sh = case, case.shape
    out, o, acc, S = run_case(c, storage, "exact")
    if c.entry == "wgrad":
        assert_premise(o, S, 6)
        got = out["dw"].cpu().double().reshape(acc.shape)
        want = acc + o["dw0"]
        bad = (got != want)
        assert not bad.any(), f"dw: {int(bad.sum())} of {bad.numel()} differ, first {bad.nonzero()[0].tolist()}: got {got[bad][0]} want {want[bad][0]}"
        if out["db"] is not None:
            want_b = o["dy"].sum((0, 1, 2)) + o["db0"]
            assert torch.equal(out["db"].cpu().double(), want_b), "dbias"
        return
    assert_premise(o, S, 10)      # products on 2^-8, scales up to 2 / down to 1/2: 2^-9 granularity with room for a factor 2
    y = out.get("y", out.get("dx"))
    real, rest = split_out(c, y, sh)
    if c.entry in ("fwd_f32", "fwd_ex_f32"):
        sent = SENT32
        want = expected32(c, o, acc).float().view(torch.int32)
        real, want = real.masked_fill(real == -2 ** 31, 0), want.masked_fill(want == -2 ** 31, 0)      # -0 == +0
    else:
        sent = SENT16[storage]
        want = bits16(expected16(c, storage, o, acc), storage)
        real, want = real.masked_fill(real == -2 ** 15, 0), want.masked_fill(want == -2 ** 15, 0)
    assert (rest == sent).all(), f"{int((rest != sent).sum())} pad / gap elements were written (pitch padding or between images)"
    bad = real != want
    if bad.any():
        i = bad.nonzero()[0].tolist()
        unwritten = int((real == sent).sum())
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} outputs differ ({unwritten} never written); first at {i}: "
                             f"got bits {int(real[tuple(i)]) & 0xFFFFFFFF:#x} want {int(want[tuple(i)]) & 0xFFFFFFFF:#x}")
    if c.entry == "fwd_stats":
        check_stats(c, storage, out["stats"], real)
    if c.entry == "dgrad_bn":
        check_bn_sums(c, storage, o, out["sums"], real)


def check_stats(c, storage, stats, real_bits):
    sh = c.shape
    cs = conv_shape(sh)
    cp = c.opts.get("cout_pad") or MX.cout_pad_of(sh.cout)
    M = sh.n * cs.ho * cs.wo
    nrows = (M + 127) // 128
    st = stats[:nrows].cpu().double()
    assert torch.isfinite(st).all(), "a partial-statistics row or channel was not written"
    assert (st[:, :, sh.cout:] == 0).all(), "pad channels of the statistics must be zero"
    y = real_bits.view(DTYPE[storage]).double().reshape(M, sh.cout)
    s1 = st[:, 0, :sh.cout]
    if c.cfg in EXACT_IDS:       # whole 128-pixel rows: every row exact
        ref1 = torch.zeros(nrows, sh.cout, dtype=torch.float64).index_add_(0, torch.arange(M) // 128, y)
        assert torch.equal(s1, ref1), "per-row sum of the stored output"
    assert torch.equal(s1.sum(0), y.sum(0)), "sum of the stored output"
    ref2 = (y * y).sum(0)
    bound = (M + 2) * 2.0 ** -24 * ref2 + 1e-30
    assert ((st[:, 1, :sh.cout].sum(0) - ref2).abs() <= bound).all(), "sum of squares"


def check_bn_sums(c, storage, o, sums, real_bits):
    sh = c.shape
    g = real_bits.view(DTYPE[storage]).double()
    sc, sf, mu, ist = o["ss"].view(4, sh.cin)
    z = o["z"]
    yv = z * sc + sf
    dyv = torch.where(yv > 0, g, f32mul(g, SLOPE))
    xh = (z - mu) * ist
    t1, t2 = dyv, dyv * xh
    n = t1[..., 0].numel()
    got = sums.cpu().double()
    for k, t in enumerate((t1, t2)):
        ref = t.sum((0, 1, 2))
        bound = (n + 4) * 2.0 ** -24 * t.abs().sum((0, 1, 2)) + 1e-30
        err = (got[k * sh.cin:(k + 1) * sh.cin] - ref).abs()
        assert (err <= bound).all(), f"BN-backward sum {k}: max excess {(err - bound).max().item()}"


# ------------------------------------------------------------------------------------------------------------------------- (b)
REAL = [c for c in MX.CASES if c.entry in ("fwd", "fwd_f32", "dgrad") and c.opts.get("s2") in (None, "four", "cat")]


@pytest.mark.parametrize("storage", MX.STORAGES)
@pytest.mark.parametrize("case", REAL, ids=_ids(REAL))
def test_realistic_per_element_bound(case, storage):
    c, sh = case, case.shape
    out, o, acc, S = run_case(c, storage, "real")
    y = out.get("y", out.get("dx"))
    real, _ = split_out(c, y, sh)
    u = U[storage]
    K = sh.k * sh.k * (sh.cin if c.entry.startswith("fwd") else sh.cout)
    gam = K * 2.0 ** -24 / (1 - K * 2.0 ** -24)
    tiny = 2.0 ** -24 if storage == "fp16" else 0.0       # fp16 subnormal spacing
    if c.entry == "fwd_f32":
        ref = acc + o["bias"]
        got = real.view(torch.float32).double()
        bound = gam * S + 2.0 ** -24 * ref.abs()
    else:
        got = real.view(DTYPE[storage]).double()
        ref, bound = acc, u * acc.abs() + gam * S + tiny
        if c.opts.get("res"):
            ref = acc + o["res"]
            bound = u * ref.abs() + gam * S + u * (rnd16(acc, storage).abs() + o["res"].abs()) + 2 * tiny
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = bad.nonzero()[0].tolist()
        raise AssertionError(f"{int(bad.sum())} of {bad.numel()} elements out of bound; first at {i}: got {got[tuple(i)].item()} "
                             f"ref {ref[tuple(i)].item()} bound {bound[tuple(i)].item()}")


# ------------------------------------------------------------------------------------------------------------------------- strict mode
def _strict_status(storage, sh, entry, cfg=0, split=0, cout_pad=None, opts=None):
    c = MX.Case("strict", entry, sh, cfg, dict(opts or {}, split=split))
    Lb = L(storage)
    cs = conv_shape(sh)
    cp = cout_pad or MX.cout_pad_of(sh.cout)
    wf, wd = pack(Lb, cs, torch.zeros(sh.cout, sh.cin, sh.k, sh.k, dtype=torch.float64), cp, storage)
    x = torch.zeros((sh.n, sh.h, sh.w, cs.in_ld), dtype=DTYPE[storage], device=dev())
    dy = torch.zeros((sh.n, cs.ho, cs.wo, cs.out_ld), dtype=DTYPE[storage], device=dev())
    with Knobs(storage, c):
        if entry == "fwd_f32":
            y = torch.zeros((sh.n, cs.ho, cs.wo, cs.out_ld), dtype=torch.float32, device=dev())
            st = Lb.mi355det_conv_fwd(C.byref(cs), vp(x), vp(wf), None, vp(y), 1, None, cp, stream())
        elif entry == "fwd":
            y = torch.zeros((sh.n, cs.ho, cs.wo, cs.out_ld), dtype=DTYPE[storage], device=dev())
            st = Lb.mi355det_conv_fwd(C.byref(cs), vp(x), vp(wf), None, vp(y), 0, None, cp, stream())
        elif entry == "dgrad":
            st = Lb.mi355det_conv_dgrad(C.byref(cs), vp(dy), vp(wd), vp(x), None, 0, stream())
        else:
            dw = torch.zeros(sh.cout, sh.k * sh.k * sh.cin, device=dev())
            ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
            st = Lb.mi355det_conv_wgrad(C.byref(cs), vp(x), vp(dy), vp(dw), None, vp(ws), ws.numel(), stream())
        torch.cuda.synchronize()
    return st


@pytest.mark.parametrize("storage", MX.STORAGES)
def test_strict_mode_rejects_what_would_fall_back(storage):
    from object_detectors_amd import _lib
    EINVAL = -1
    bad = [
        ("17 on a 128-channel forward", MX.shp(2, 16, 16, 64, 128, 3, 1), "fwd", 17, 0, None),
        ("44 with the fp32 epilogue", MX.shp(2, 16, 16, 64, 256, 3, 1), "fwd_f32", 44, 0, None),
        ("4 on the single-launch stride-2 route", MX.shp(2, 8, 64, 64, 64, 3, 2), "dgrad", 4, 0, None),
        ("a wide id on a narrow output", MX.shp(2, 16, 16, 64, 64, 3, 1), "fwd", 1, 0, None),
        ("30 on a wide output", MX.shp(2, 16, 16, 64, 256, 3, 1), "fwd", 30, 0, None),
        ("an unknown id", MX.shp(2, 16, 16, 64, 256, 3, 1), "fwd", 77, 0, None),
        ("15 on a 1x1 convolution", MX.shp(2, 16, 16, 64, 256, 1, 1), "fwd", 15, 0, None),
        ("an invalid split count", MX.shp(2, 13, 11, 64, 200, 3, 1), "wgrad", 0, 4, None),        # 286 pixels: chunks of 128 give 3 pieces
        ("a split count beyond the workspace", MX.shp(2, 40, 40, 64, 256, 3, 1), "wgrad", 0, 10, None),     # 10 x 10 tiles x 64 KB > 1 MB
    ]
    for what, sh, entry, cfg, split, cp in bad:
        st = _strict_status(storage, sh, entry, cfg, split, cp, {"s2": "single"} if "single" in what else None)
        assert st == EINVAL, f"{what}: strict mode returned {st}"
        msg = _lib.lib().mi355det_last_error().decode()
        assert "strict" in msg and (str(cfg) in msg or str(split) in msg), msg
    # the same forced ids without strict mode: the old behaviour (a launch of another kernel)
    Lb = L(storage)
    for what, sh, entry, cfg, split, cp in bad:
        if entry == "wgrad" and split == 10:
            continue      # (the non-strict split fallback is exercised by test_gpu_conv)
        cs = conv_shape(sh)
        cpp = cp or MX.cout_pad_of(sh.cout)
        wf, wd = pack(Lb, cs, torch.zeros(sh.cout, sh.cin, sh.k, sh.k, dtype=torch.float64), cpp, storage)
        x = torch.zeros((sh.n, sh.h, sh.w, cs.in_ld), dtype=DTYPE[storage], device=dev())
        try:
            Lb.mi355det_debug_set(0, cfg)
            Lb.mi355det_debug_set(7, split)
            if entry == "wgrad":
                dy = torch.zeros((sh.n, cs.ho, cs.wo, cs.out_ld), dtype=DTYPE[storage], device=dev())
                dw = torch.zeros(sh.cout, sh.k * sh.k * sh.cin, device=dev())
                ws = torch.zeros(1 << 20, dtype=torch.uint8, device=dev())
                st = Lb.mi355det_conv_wgrad(C.byref(cs), vp(x), vp(dy), vp(dw), None, vp(ws), ws.numel(), stream())
            elif entry == "dgrad":
                dy = torch.zeros((sh.n, cs.ho, cs.wo, cs.out_ld), dtype=DTYPE[storage], device=dev())
                st = Lb.mi355det_conv_dgrad(C.byref(cs), vp(dy), vp(wd), vp(x), None, 0, stream())
            else:
                f32 = entry == "fwd_f32"
                y = torch.zeros((sh.n, cs.ho, cs.wo, cs.out_ld), dtype=torch.float32 if f32 else DTYPE[storage], device=dev())
                st = Lb.mi355det_conv_fwd(C.byref(cs), vp(x), vp(wf), None, vp(y), int(f32), None, cpp, stream())
            torch.cuda.synchronize()
        finally:
            Lb.mi355det_debug_set(0, 0)
            Lb.mi355det_debug_set(7, 0)
        assert st == 0, f"{what}: key 9 = 0 must keep the fallback ({st})"


@pytest.mark.parametrize("storage", MX.STORAGES)
def test_16bit_outputs_need_whole_8_channel_pieces(storage):
    """Regression: conv_fwd (plain / statistics epilogue) with cout % 8 != 0 and conv_dgrad with cin % 8 != 0 stored the last 8-channel piece
    whole - into the pitch padding, or with a dense pitch over the first channels of the next pixel.  Both are now MI355DET_EINVAL (as
    conv_fwd_ex already was); fp32 outputs store per channel and keep taking any cout."""
    Lb = L(storage)
    for entry, sh in (("fwd", MX.shp(2, 9, 11, 64, 324, 3, 1, ypad=0)), ("dgrad", MX.shp(2, 9, 11, 20, 64, 3, 1, xpad=0))):
        cs = conv_shape(sh)
        cp = MX.cout_pad_of(sh.cout)
        wf, wd = pack(Lb, cs, torch.zeros(sh.cout, sh.cin, sh.k, sh.k, dtype=torch.float64), cp, storage)
        a = sentinel16((sh.n, sh.h, sh.w, cs.in_ld), storage)
        b = sentinel16((sh.n, cs.ho, cs.wo, cs.out_ld), storage)
        if entry == "fwd":
            st = Lb.mi355det_conv_fwd(C.byref(cs), vp(a), vp(wf), None, vp(b), 0, None, cp, stream())
            out = b
        else:
            st = Lb.mi355det_conv_dgrad(C.byref(cs), vp(b), vp(wd), vp(a), None, 0, stream())
            out = a
        torch.cuda.synchronize()
        assert st == -1, (entry, st)
        assert (out.view(torch.int16) == SENT16[storage]).all(), "nothing may be written"
