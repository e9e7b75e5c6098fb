"""Grouped 3x3 convolution micro-benchmark (csrc/gconv_kernels.hip): the eight distinct conv2 layers of ResNeXt-50 32x4d and ResNeXt-101 32x8d
(four stages each, plus the three stride-2 first blocks) at batch 4, 800 x 1344.

    python tools/bench_gconv.py [--out profiles/NAME.md] [--iters 20]

Per layer and direction (forward, data gradient, weight gradient): device-event time after warm-up, effective GB/s over the compulsory
bytes (each activation operand once as bf16; the weight gradient also its fp32 output), beside
  torch   torch.nn.functional.conv2d(groups=32) and its autograd pieces on the same bf16 channels-last tensors
  dense   the project's dense 3x3 kernels at the same cin == cout (up to 32 x the arithmetic)."""
import argparse
import ctypes as C
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from object_detectors_amd import ops            # noqa: E402
from object_detectors_amd._lib import lib       # noqa: E402

GROUPS = 32
N, H, W = 4, 800, 1344


def layers():
    out = []
    for model, wpg in (("resnext50_32x4d", 4), ("resnext101_32x8d", 8)):
        for li, planes in enumerate((64, 128, 256, 512), 1):
            width = int(planes * wpg / 64.0) * GROUPS
            hin, win = H // (2 ** (li + 1)), W // (2 ** (li + 1))          # layer li runs at stride 4 * 2^(li-1)
            out.append((model, f"layer{li}", width, hin, win, 1))
            if li > 1:
                out.append((model, f"layer{li}.0", width, hin * 2, win * 2, 2))
    seen, uniq = set(), []
    for l in out:
        if l[2:] not in seen:
            seen.add(l[2:])
            uniq.append(l)
    return uniq


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gconv needs the GPU"
    dev = torch.device("cuda:0")
    L = lib()
    rows = ["| model | layer | C (c/g) | map | s | dir | gconv us | GB/s | torch us | dense us | gconv/torch | gconv/dense |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for model, lname, c, h, w, s in layers():
        cpg = c // GROUPS
        shp = ops.gconv_shape(N, h, w, c, s)
        ho, wo = shp.ho, shp.wo
        x = torch.randn(N, h, w, c, device=dev).bfloat16()
        dy = torch.randn(N, ho, wo, c, device=dev).bfloat16()
        wt = torch.randn(c, cpg, 3, 3, device=dev) * 0.05
        wf, wd = ops.gconv_pack(shp, GROUPS, wt)
        y, dx = torch.empty_like(dy), torch.empty_like(x)
        dw = torch.empty(c, 3, 3, cpg, device=dev)
        ws = torch.empty(max(L.mi355det_gconv_wgrad_workspace(C.byref(shp), GROUPS), 16), device=dev, dtype=torch.uint8)
        ours = {"fwd": timeit(lambda: ops.gconv_fwd(shp, GROUPS, x, wf, y), a.iters),
                "dgrad": timeit(lambda: ops.gconv_dgrad(shp, GROUPS, dy, wd, dx), a.iters),
                "wgrad": timeit(lambda: ops.gconv_wgrad(shp, GROUPS, x, dy, dw, workspace=ws), a.iters)}
        # torch on the same bf16 channels-last tensors (NCHW views of the NHWC buffers)
        xt, dyt = x.permute(0, 3, 1, 2), dy.permute(0, 3, 1, 2)
        wtt = wt.bfloat16().contiguous(memory_format=torch.channels_last)
        tor = {"fwd": timeit(lambda: F.conv2d(xt, wtt, stride=s, padding=1, groups=GROUPS), a.iters),
               "dgrad": timeit(lambda: torch.ops.aten.convolution_backward(dyt, xt, wtt, None, (s, s), (1, 1), (1, 1), False, (0, 0), GROUPS,
                                                                           (True, False, False)), a.iters),
               "wgrad": timeit(lambda: torch.ops.aten.convolution_backward(dyt, xt, wtt, None, (s, s), (1, 1), (1, 1), False, (0, 0), GROUPS,
                                                                           (False, True, False)), a.iters)}
        # the dense kernels at the same width, tuned the way a plan build tunes them
        dshp = ops.conv_shape(N, h, w, c, c, 3, s)
        dwf, dwd = ops.pack_weights(dshp, torch.randn(c, c, 3, 3, device=dev) * 0.02)
        ddw = torch.zeros(c, 9 * c, device=dev)
        dws = torch.empty(max(L.mi355det_conv_wgrad_workspace(C.byref(dshp)), 16), device=dev, dtype=torch.uint8)
        L.mi355det_conv_autotune_mode(1)
        ops.conv_fwd(dshp, x, dwf, y)
        ops.conv_dgrad(dshp, dy, dwd, dx)
        L.mi355det_conv_autotune_mode(0)
        L.mi355det_conv_wgrad_autotune(C.byref(dshp), x.data_ptr(), dy.data_ptr(), ddw.data_ptr(), dws.data_ptr(), dws.numel(), None)
        den = {"fwd": timeit(lambda: ops.conv_fwd(dshp, x, dwf, y), a.iters),
               "dgrad": timeit(lambda: ops.conv_dgrad(dshp, dy, dwd, dx), a.iters),
               "wgrad": timeit(lambda: ops.conv_wgrad(dshp, x, dy, ddw, workspace=dws), a.iters)}
        act = 2 * (N * h * w * c + N * ho * wo * c)
        byts = {"fwd": act, "dgrad": act, "wgrad": act + 4 * c * 9 * cpg}
        for d in ("fwd", "dgrad", "wgrad"):
            rows.append(f"| {model} | {lname} | {c} ({cpg}) | {h}x{w} | {s} | {d} | {ours[d]:.1f} | {byts[d] / ours[d] / 1e3:.0f} | {tor[d]:.1f} | "
                        f"{den[d]:.1f} | {ours[d] / tor[d]:.2f} | {ours[d] / den[d]:.2f} |")
            print(rows[-1], flush=True)
        del x, dy, y, dx, ws, dws
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("# Grouped 3x3 convolution, batch 4 at 800 x 1344 (tools/bench_gconv.py)\n\n"
                    "Device-event times after warm-up; GB/s over the compulsory bytes (activation operands once as bf16, the weight gradient\n"
                    "also its fp32 output).  torch = F.conv2d(groups=32) / aten.convolution_backward on the same bf16 channels-last tensors;\n"
                    "dense = the project's dense 3x3 kernels at cin == cout == C.  Ratios above 1 mean the grouped kernel is slower.\n\n")
            f.write("\n".join(rows) + "\n")


if __name__ == "__main__":
    main()
