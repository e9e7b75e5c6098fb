"""Writes tests/golden/g17_resnext.npz from the reference's own ResNet class (CPU only):

    python tools/gen_resnext_golden.py /path/to/object_detectors

For resnext50_32x4d, resnext101_32x8d, wide_resnet50_2 and wide_resnet101_2 the fixture holds the ordered body state_dict keys with their
shapes.  For resnext50_32x4d and wide_resnet50_2 it also holds C2..C5 (sampled like oracle.retina_oracle.sample) of an eval-mode forward
(BatchNorm2d in eval mode = FrozenBatchNorm2d at eps 1e-5) on one 1 x 3 x 64 x 96 input, which the body receives as is (no normalisation).
Parameters and buffers are oracle.retina_oracle.det_fill(key, shape, SEED + position in the state_dict), so no weight is stored;
num_batches_tracked entries are skipped (and not listed: FrozenBatchNorm2d has none).  `scale_<body>` is a factor the generator applied to
every conv2 weight on top of det_fill (1.0 = none was needed)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import detrand                      # noqa: E402
from oracle import retina_oracle as ro          # noqa: E402

SEED, INPUT_SEED = 17000, 17001
BODIES = ("resnext50_32x4d", "resnext101_32x8d", "wide_resnet50_2", "wide_resnet101_2")
FORWARD = ("resnext50_32x4d", "wide_resnet50_2")
PREFIX = "backbone.body."


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "torchvision_models"))
    from utilities import resnet
    out = {"seed": np.int64(SEED)}
    x = torch.from_numpy(detrand.uniform(INPUT_SEED, (1, 3, 64, 96), -2.0, 2.0))
    out["input"] = x.numpy()
    for body in BODIES:
        m = getattr(resnet, body)(norm_layer=torch.nn.BatchNorm2d).eval()
        sd = m.state_dict()
        keys = [k for k in sd if not k.endswith("num_batches_tracked") and not k.startswith("fc.")]
        out["keys_" + body] = np.array([PREFIX + k for k in keys])
        out["shapes_" + body] = np.array([list(sd[k].shape) + [0] * (4 - sd[k].dim()) for k in keys], dtype=np.int64)
        if body not in FORWARD:
            continue
        scale = 1.0
        with torch.no_grad():
            for i, k in enumerate(keys):
                v = torch.from_numpy(np.ascontiguousarray(ro.det_fill(PREFIX + k, tuple(sd[k].shape), SEED + i)))
                sd[k].copy_(v * scale if k.endswith("conv2.weight") else v)
            t = m.maxpool(m.relu(m.bn1(m.conv1(x))))
            for li in range(1, 5):
                t = getattr(m, f"layer{li}")(t)
                a = t.abs()
                assert float((a > 0).float().mean()) >= 0.25 and 1e-2 < float(a.max()) < 1e3, (body, li, float((a > 0).float().mean()), float(a.max()))
                out[f"c{li + 1}_{body}"] = ro.sample(t)
                out[f"c{li + 1}_max_{body}"] = np.float32(a.max())
                print(body, f"C{li + 1}", tuple(t.shape), "nonzero", float((a > 0).float().mean()), "max", float(a.max()))
        out["scale_" + body] = np.float32(scale)
    path = os.path.join(ROOT, "tests", "golden", "g17_resnext.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1_000_000
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
