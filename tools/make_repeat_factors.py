#!/usr/bin/env python3
"""The repeat factors of repeat-factor sampling (Gupta et al., LVIS 2019) for a COCO- or LVIS-format annotation file, on the GPU:
    python tools/make_repeat_factors.py --ann lvis_v1_train.json --dset lvis --out r.npy
r_i = max over image i's annotations of max(1, sqrt(t / f_c)), f_c the share of the images that hold category c (default t = 1e-3), one
float64 per listed image in ascending image-id order.  Prints how many images repeat (r > 1) and the epoch length the factors imply (the
sum of r: dataset_stats.RepeatFactorSampler draws floor(r_i) or floor(r_i) + 1 copies of image i, r_i on average).  --out writes the
factors with numpy.save; feed them to RepeatFactorSampler."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ann", required=True, help="annotation JSON (COCO or LVIS format)")
    ap.add_argument("--dset", required=True, choices=["coco", "lvis"])
    ap.add_argument("--t", type=float, default=1e-3, help="the frequency below which a category's images repeat")
    ap.add_argument("--out", default=None, help="write the factors here (numpy.save)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from object_detectors_amd import dataset_stats as ds
    r = ds.repeat_factors(args.ann, t=args.t, dset_name=args.dset, device=args.device).cpu().numpy()
    print(f"{r.size} images, t = {args.t:g}: {int((r > 1).sum())} with r > 1 (largest r {r.max():.4f})")
    print(f"epoch length the factors imply: {r.sum():.1f} images ({r.sum() / r.size:.3f} x the dataset)")
    if args.out:
        np.save(args.out, r)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
