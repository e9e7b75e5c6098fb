"""Device time of the three whole-batch tails of csrc/proposal_kernels.hip; under `rocprofv3 --kernel-trace --stats` the per-kernel split.
  --op rpn     mi355det_rpn_proposals, Faster R-CNN training shapes (4 x 159882 anchors, 5 levels, 2000 / 2000), or the composed route
  --op retina  mi355det_retina_detections at 800 px: 5 levels, 91 classes, 1000 candidates per level, 300 detections
  --op roi     mi355det_roi_detections: 1000 proposals, 91 classes, 100 detections
python tools/bench_proposals.py [--op rpn] [--batch 4] [--composed]; retina and roi need --batch (tools/bench_retina.py runs 16, tools/bench_frcnn.py 4)"""
import argparse, math, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from object_detectors_amd import ops
from object_detectors_amd.tvision.postprocess import ROI_DET_MAX_CANDIDATES, rpn_filter_proposals, rpn_proposals_fused

ap = argparse.ArgumentParser()
ap.add_argument("--op", choices=["rpn", "retina", "roi"], default="rpn")
ap.add_argument("--batch", type=int, default=None)
ap.add_argument("--pre", type=int, default=2000)
ap.add_argument("--composed", action="store_true")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
if args.batch is None:
    if args.op != "rpn":
        ap.error(f"--op {args.op} needs --batch")
    args.batch = 4
if args.composed and args.op != "rpn":
    ap.error("--composed is the route of --op rpn")
dev = torch.device("cuda:0")
N = args.batch
g = torch.Generator(device=dev).manual_seed(0)
clip = math.log(1000.0 / 16)


def boxes(rows, size):
    ctr = torch.rand(rows + (2,), device=dev, generator=g) * 800
    wh = torch.rand(rows + (2,), device=dev, generator=g) * size + 4
    return torch.cat([ctr - wh / 2, ctr + wh / 2], -1)


if args.op == "rpn":
    levels = [200 * 200 * 3, 100 * 100 * 3, 50 * 50 * 3, 25 * 25 * 3, 13 * 13 * 3]
    A = sum(levels)
    obj = torch.randn((N, A), device=dev, generator=g)
    anchors = boxes((A,), 200)
    deltas = torch.randn((N, A, 4), device=dev, generator=g) * 0.1
    shapes = [(800, 800)] * N
    what = f"{'composed' if args.composed else 'fused'} bs {N} pre {args.pre}"

    def run():
        if args.composed:
            props = ops.box_decode(deltas.reshape(-1, 4), anchors.repeat(N, 1), (1.0, 1.0, 1.0, 1.0), clip).reshape(N, -1, 4)
            return rpn_filter_proposals(props, obj, shapes, levels, args.pre, args.pre)
        return rpn_proposals_fused(deltas, obj, anchors, shapes, levels, args.pre, args.pre, xform_clip=clip)

    def kept(out):
        return [int(b.shape[0]) for b in out[0]]
else:
    lim = torch.tensor([[800.0] * 4] * N, device=dev)
    if args.op == "retina":
        hwa = [s * s * 9 for s in (100, 50, 25, 13, 7)]
        logits = [torch.randn((N, h, 91), device=dev, generator=g) for h in hwa]      # every level fills its 1000 candidates
        regs = [torch.randn((N, h, 4), device=dev, generator=g) * 0.1 for h in hwa]
        anchors = [boxes((h,), 32 * 2 ** i) for i, h in enumerate(hwa)]
        what = f"retina bs {N}"

        def run():
            return ops.retina_detections(logits, regs, anchors, lim, math.log(0.05 / 0.95), 1000, 0.5, 300, clip)
    else:
        scores = torch.softmax(torch.randn((N, 1000, 91), device=dev, generator=g) * 3, -1)
        scores[:, :, 0] = float("-inf")
        reg = torch.randn((N, 1000, 91 * 4), device=dev, generator=g) * 0.5
        props = boxes((N, 1000), 200).clamp(0, 800)
        what = f"roi bs {N}"

        def run():
            return ops.roi_detections(scores, reg, props, lim, 0.05, ROI_DET_MAX_CANDIDATES, (10.0, 10.0, 5.0, 5.0), 0.5, 100)

    def kept(out):
        return out[3][:N].tolist()

for _ in range(3):
    out = run()
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
import time
t0 = time.perf_counter()
e0.record()
for _ in range(args.reps):
    out = run()
e1.record()
torch.cuda.synchronize()
wall = (time.perf_counter() - t0) / args.reps * 1e3
print(f"{what}: {e0.elapsed_time(e1) / args.reps:.3f} ms per call (events), {wall:.3f} ms wall; kept {kept(out)}")
