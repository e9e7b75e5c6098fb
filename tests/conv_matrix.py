"""Coverage table of the convolution engine's tunable kernels (data only, no GPU).

Every tile configuration the plan-time tuner may pick (conv_kernels.hip: the tuned rows of the configuration table), the narrow-output
alternatives 29 / 30 / 31 and the untuned default 0 appear here with every epilogue their table row accepts, each on a shape where the id applies ("clean":
whole tiles) and on one with tails (a pixel count that is not a multiple of any tile height, an image boundary inside a tile, a partial
last channel tile).  Beside them: the stride-2 data-gradient routes, the split-K data gradient and the weight-gradient split counts.

A case is (entry point, shape, forced id, options); tests/test_gpu_conv_exact.py runs every case in both storage formats with strict mode
on (debug key 9), so a forced id that the launch would not honour is an error instead of a silent launch of configuration 1.
tests/test_conv_coverage.py checks this table against the kernel sources and the committed tune records.
"""
from collections import namedtuple

STORAGES = ("bf16", "fp16")

# the epilogue a launch runs (csrc/igemm_common.h: EPI_*)
EPI = {"STATS": 0, "F32": 1, "RES": 2, "PLAIN": 3, "AFF": 4, "BNRED": 5}

# Shape: n, h, w, cin, cout, ksize, stride; xpad / ypad / rpad = extra elements of the pixel pitch of the input / output / residual beyond
# their channel count (filled with NaN by the tests: a kernel that reads them produces NaN)
Shape = namedtuple("Shape", "n h w cin cout k s xpad ypad rpad")
Case = namedtuple("Case", "name entry shape cfg opts")

WGRAD_FORM8 = 1 << 16


def shp(n, h, w, cin, cout, k, s, xpad=8, ypad=8, rpad=16):
    return Shape(n, h, w, cin, cout, k, s, xpad, ypad, rpad)


def out_hw(sh):
    p = (sh.k - 1) // 2
    return (sh.h + 2 * p - sh.k) // sh.s + 1, (sh.w + 2 * p - sh.k) // sh.s + 1


def cout_pad_of(cout):
    """object_detectors_amd/ops.py: cout_pad_of (the engines' padding of forward outputs)."""
    if cout >= 2048:
        return (cout + 255) // 256 * 256
    return (cout + 127) // 128 * 128 if cout >= 128 or cout % 32 else cout


def gemm_cout_pad(case):
    """Padded output-channel count of the implicit GEMM the case launches (forward: cout_pad, data gradient: cin padded to 32)."""
    if case.entry.startswith("fwd"):
        return case.opts.get("cout_pad") or cout_pad_of(case.shape.cout)
    if case.opts.get("s2") == "cat":
        return 2 * case.shape.cin          # class-concatenated view: a row is the two dx pixels 2xx, 2xx + 1
    return (case.shape.cin + 31) // 32 * 32


def gemm_cout(case):
    if case.opts.get("s2") == "cat":
        return 2 * case.shape.cin
    return case.shape.cout if case.entry.startswith("fwd") else case.shape.cin


def lattice(case):
    """(images, pixels per image) of the GEMM's pixel lattice (one stride-2 parity class for the four-class data gradient)."""
    sh = case.shape
    if case.entry.startswith("fwd"):
        ho, wo = out_hw(sh)
        return sh.n, ho * wo
    if sh.s == 1:
        return sh.n, sh.h * sh.w
    return sh.n, ((sh.h + 1) // 2) * ((sh.w + 1) // 2)


def has_tails(case):
    """Pixel count not a multiple of any tile height (all are multiples of 16), an image boundary inside a tile, a partial channel tile."""
    n, hw = lattice(case)
    return (n * hw) % 16 != 0 and hw % 16 != 0 and n > 1 and gemm_cout(case) < gemm_cout_pad(case)


def epilogue(case):
    """Epilogue of the implicit-GEMM launch(es) of a case, None when no tunable implicit GEMM runs (weight gradient, split-K data gradient)."""
    e, o = case.entry, case.opts
    if e == "fwd":
        return "PLAIN"
    if e == "fwd_stats":
        return "STATS"
    if e in ("fwd_f32", "fwd_ex_f32"):
        return "F32"
    if e == "fwd_ex":
        return "AFF"
    if e == "dgrad":
        return "RES" if o.get("res") else "PLAIN"
    if e == "dgrad_mask":
        return "RES"
    if e == "dgrad_bn":
        return "BNRED"
    return None


# ---- tile configurations (conv_kernels.hip)
WIDE_IDS = (1, 2, 3, 4, 5, 6, 15, 16, 17, 18, 19, 26, 27, 28, 40, 44, 45)     # the tuned wide rows, in table order
NARROW_IDS = (29, 30, 31)                                                      # the narrow-output alternatives to the plain tile
DX_IDS = (15, 16, 17, 18, 19, 26, 27, 28)                                      # shared-pixel-tile kernel: 3x3, stride 1
ALL_EPIS = ("STATS", "F32", "RES", "PLAIN", "AFF", "BNRED")
ACCEPTS = {i: ALL_EPIS for i in WIDE_IDS + NARROW_IDS + (0,)}
ACCEPTS[40] = ("STATS", "F32", "RES", "PLAIN", "AFF")
ACCEPTS[44] = ACCEPTS[45] = ("STATS", "RES", "PLAIN", "AFF")

# ---- shapes.  Forward GEMM: output channels = cout; data gradient: output channels = cin (padded to 32), reduction = cout.
FWD_WIDE = (shp(2, 16, 16, 64, 256, 3, 1), shp(2, 13, 11, 64, 200, 3, 1))           # clean, tails (200 of 256 channels)
DGRAD_WIDE = (shp(2, 16, 16, 256, 64, 3, 1), shp(2, 13, 11, 232, 64, 3, 1))
FWD_NARROW = {     # id -> (clean, tails, cout_pad of the tails shape)
    30: (shp(2, 16, 16, 64, 64, 3, 1), shp(2, 13, 11, 64, 56, 3, 1), 64),
    29: (shp(2, 16, 16, 64, 32, 3, 1), shp(2, 13, 11, 64, 24, 3, 1), 32),
    31: (shp(2, 16, 16, 32, 64, 3, 1), shp(2, 13, 11, 32, 56, 3, 1), 64),     # 32 input channels: k-step 32
}
DGRAD_NARROW = {
    30: (shp(2, 16, 16, 64, 64, 3, 1), shp(2, 13, 11, 56, 64, 3, 1)),
    29: (shp(2, 16, 16, 32, 64, 3, 1), shp(2, 13, 11, 24, 64, 3, 1)),
    31: (shp(2, 16, 16, 64, 32, 3, 1), shp(2, 13, 11, 56, 32, 3, 1)),
}

# per shape, the entry points that run one epilogue each
FWD_ENTRIES = (
    ("fwd_stats", {}),
    ("fwd", {}),
    ("fwd_f32", {"bias": True}),
    ("fwd_ex_f32", {"relu": 2, "scale": True, "shift": True, "image_stride": True}),
    ("fwd_ex", {"relu": 1, "scale": True, "shift": True, "res": True}),
    ("fwd_ex", {"relu": 2, "scale": False, "shift": True, "res": True}),
    ("fwd_ex", {"relu": 0, "scale": True, "shift": True, "res": False}),
)
DGRAD_ENTRIES = (
    ("dgrad", {}),
    ("dgrad", {"res": True}),
    ("dgrad_mask", {"mask_relu": 1, "mask_scale": True}),
    ("dgrad_mask", {"mask_relu": 0, "mask_scale": False}),
    ("dgrad_bn", {"res": True}),
)


def _name(entry, sh, cfg, opts):
    o = ",".join(f"{k}={int(v) if isinstance(v, bool) else v}" for k, v in sorted(opts.items()))
    return f"{entry}_{sh.n}x{sh.h}x{sh.w}_{sh.cin}-{sh.cout}_k{sh.k}s{sh.s}_cfg{cfg}" + (f"_{o}" if o else "")


def _applies(cfg, case):
    """Does forced id `cfg` run on this case (conv_kernels.hip: cfg_applies on the id's table row)?  The table only keeps cases where it does:
    strict mode turns every other combination into an error."""
    ep = epilogue(case)
    if ep is None or ep not in ACCEPTS.get(cfg, ()):
        return cfg == 0 and ep is None
    sh, o = case.shape, case.opts
    cp = gemm_cout_pad(case)
    kchan = sh.cin if case.entry.startswith("fwd") else sh.cout
    if cfg == 0:
        return True
    wide = cp % 128 == 0 and kchan % 64 == 0
    if cfg in NARROW_IDS:
        if cp % 128 == 0 or kchan % 32 or sh.k != 3 or sh.s != 1:
            return False
        return {29: cp % 64 != 0 and kchan % 64 == 0, 30: cp % 64 == 0 and kchan % 64 == 0, 31: cp % 64 == 0}[cfg]
    if not wide:
        return False
    if case.entry.startswith("dgrad") and sh.s == 2 and o.get("s2") == "single":
        return False
    if cfg in (3, 6, 17, 18, 28, 40, 44, 45) and cp % 256:
        return False
    if cfg in DX_IDS and not (sh.k == 3 and sh.s == 1):
        return False
    return True


def _grid(entries, shapes, ids, cout_pad=None):
    out = []
    for sh in shapes:
        for entry, opts in entries:
            for cfg in ids:
                o = dict(opts)
                if cout_pad and entry.startswith("fwd") and sh is shapes[-1]:
                    o["cout_pad"] = cout_pad
                c = Case(_name(entry, sh, cfg, o), entry, sh, cfg, o)
                if _applies(cfg, c):
                    out.append(c)
    return out


def _build():
    cases = []
    ids = (0,) + WIDE_IDS
    cases += _grid(FWD_ENTRIES, FWD_WIDE, ids)
    cases += _grid(DGRAD_ENTRIES, DGRAD_WIDE, ids)
    for nid, (clean, tail, cp) in FWD_NARROW.items():
        cases += _grid(FWD_ENTRIES, (clean, tail), (0, nid), cout_pad=cp)
    for nid, (clean, tail) in DGRAD_NARROW.items():
        cases += _grid(DGRAD_ENTRIES, (clean, tail), (0, nid))
    fwd_some = (("fwd_stats", {}), ("fwd_ex", {"relu": 1, "scale": True, "shift": True, "res": True}),
                ("fwd_ex", {"relu": 2, "scale": True, "shift": True, "res": False}))
    # Cin = 32 on a wide output: the fixed 128 x 128 x 32 tile (no choice)
    cases += _grid(fwd_some + (("fwd", {}),), (shp(2, 13, 11, 32, 128, 3, 1), shp(2, 13, 11, 32, 72, 3, 1)), (0,))
    # cout 72 (partial 128 tile), more than 8 channel tiles (XCD-blocked tile order)
    cases += _grid(fwd_some, (shp(2, 9, 11, 64, 72, 3, 1),), (0, 1, 2, 4, 5, 16, 27))
    cases += _grid(fwd_some + (("fwd", {}),), (shp(1, 5, 7, 64, 1280, 3, 1, ypad=0, rpad=0),), (0, 1, 3, 4, 40, 44))
    # heads: fp32 epilogue with bias (YOLO 255 of 256), scale / shift / LeakyReLU and the level-concatenated image stride (RetinaNet 36 / 819)
    heads = (("fwd_f32", {"bias": True}), ("fwd_ex_f32", {"relu": 0, "scale": False, "shift": True, "image_stride": True}),
             ("fwd_ex_f32", {"relu": 1, "scale": True, "shift": True, "image_stride": False}))
    cases += _grid(heads, (shp(2, 10, 10, 256, 255, 1, 1, ypad=1),), (0, 1, 4, 40))
    cases += _grid(heads, (shp(2, 9, 11, 256, 36, 3, 1, ypad=0), shp(1, 7, 9, 128, 819, 3, 1, ypad=0)), (0, 1, 4, 5, 15, 27))
    # cout 324 (384 padded; 16-bit outputs need cout % 8 == 0 - the regression case test_16bit_outputs_need_whole_8_channel_pieces)
    cases += _grid(heads, (shp(2, 9, 11, 64, 324, 3, 1),), (0, 1, 2, 4, 5, 16, 27))
    # stride-2 forwards (affine epilogue: the RetinaNet record runs configuration 3 there), odd maps (13 -> 7), 1x1
    s2 = (("fwd_stats", {}), ("fwd", {}), ("fwd_ex", {"relu": 1, "scale": True, "shift": True, "res": True}),
          ("fwd_ex", {"relu": 0, "scale": True, "shift": True, "res": False}))
    cases += _grid(s2, (shp(2, 26, 26, 64, 256, 3, 2), shp(2, 13, 13, 64, 200, 3, 2)), (0, 1, 2, 3, 4, 5, 6, 40, 44, 45))
    cases += _grid(s2, (shp(2, 13, 13, 128, 256, 1, 1), shp(2, 13, 13, 64, 256, 1, 2)), (0, 1, 2, 3, 4, 5, 6, 40, 44, 45))
    # stride-2 data gradients: four class launches (key 5 = 0, key 2 = 1), class-concatenated (key 5 = 1: no pitch padding on dx / residual),
    # single launch (key 2 = 0), 1x1 / stride 2 (lattice fill of the three classes it never reads)
    for res in (False, True):
        o4 = {"s2": "four", "res": res}
        cases += _grid((("dgrad", o4),), (shp(2, 26, 26, 128, 128, 3, 2), shp(2, 13, 13, 120, 64, 3, 2)), (0, 1, 2, 3, 4, 5, 6, 40, 44, 45))
        cases += _grid((("dgrad", {"s2": "cat", "res": res}),), (shp(2, 26, 26, 128, 128, 3, 2, xpad=0, rpad=0),
                                                                shp(2, 14, 10, 64, 64, 3, 2, xpad=0, rpad=0)), (0, 1, 2, 3, 4, 5, 6, 40, 44, 45))
        cases += _grid((("dgrad", {"s2": "single", "res": res}),), (shp(2, 8, 64, 64, 64, 3, 2), shp(2, 6, 64, 32, 64, 3, 2)), (0,))
        cases += _grid((("dgrad", {"s2": "four", "res": res}),), (shp(2, 8, 64, 64, 64, 3, 2),), (0, 1, 4))      # the same shapes, key 2 on
        cases += _grid((("dgrad", {"res": res}),), (shp(2, 13, 13, 128, 128, 1, 2), shp(2, 13, 13, 128, 256, 1, 1)), (0, 1, 2, 4, 5, 40, 44, 45))
    cases += _grid((("dgrad_bn", {"res": False}), ("dgrad_bn", {"res": True})), (shp(2, 26, 26, 128, 128, 3, 2), shp(2, 13, 13, 120, 64, 3, 2)),
                   (0, 1, 4))
    # split-K data gradient (few pixels, deep reduction): its own tile, one rounding after the sum and the residual
    for res in (False, True):
        for sh in (shp(1, 7, 7, 128, 1024, 3, 1), shp(2, 5, 7, 120, 1024, 3, 1), shp(2, 13, 11, 128, 256, 3, 1)):
            cases.append(Case(_name("dgrad_ws", sh, 0, {"res": res}), "dgrad_ws", sh, 0, {"res": res}))
    # weight gradient: every split count of the tuner's list that is valid for the shape, both forms where the 256 x 256 kernel applies
    for sh in WGRAD_SHAPES:
        for v in wgrad_values(sh):
            for dbias in (False, True):
                o = {"split": v, "dbias": dbias}
                cases.append(Case(_name("wgrad", sh, 0, o), "wgrad", sh, 0, o))
    names = [c.name for c in cases]
    assert len(names) == len(set(names)), "duplicate case names"
    return cases


# ---- weight gradient (wgrad_kernels.hip)
WGRAD_SPLITS = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 32, 40, 48, 56, 64, 96, 128, 192, 256, 384, 512, 768, 1024)   # cands[]
WGRAD_SHAPES = (shp(2, 16, 16, 64, 256, 3, 1), shp(2, 13, 11, 64, 264, 3, 1), shp(2, 40, 40, 64, 128, 3, 1), shp(2, 13, 13, 64, 128, 3, 2),
                shp(2, 13, 13, 256, 256, 1, 1), shp(2, 13, 11, 32, 72, 3, 1), shp(1, 40, 40, 64, 264, 3, 1))


def split_valid(m, sp):
    """wgrad_kernels.hip: split_valid."""
    if sp < 1:
        return False
    chunk = ((m + sp - 1) // sp + 63) // 64 * 64
    return (m + chunk - 1) // chunk == sp


def wgrad8_applies(sh):
    """wgrad_kernels.hip: wgrad8_applicable."""
    ho, wo = out_hw(sh)
    return wo >= 4 and 64 // wo + 1 <= ho and sh.cout >= 256 and sh.k * sh.k * sh.cin >= 256 and sh.cin % 8 == 0


def wgrad_values(sh):
    ho, wo = out_hw(sh)
    m = sh.n * ho * wo
    sps = [sp for sp in WGRAD_SPLITS if split_valid(m, sp) and m // sp >= 64]
    out = list(sps)
    if wgrad8_applies(sh):
        out += [sp | WGRAD_FORM8 for sp in sps]
    return out


def wgrad_route(v):
    """What distinguishes two split counts in the kernels: the form, and which fold runs (none / wgrad_reduce_kernel / wgrad_reduce8_kernel)."""
    sp = v & (WGRAD_FORM8 - 1)
    return bool(v & WGRAD_FORM8), 0 if sp == 1 else (1 if sp < 8 else 2)


CASES = _build()
