#!/usr/bin/env python3
"""Find the YOLO anchors of a COCO- or LVIS-format annotation file on the GPU (the reference's yolo/utilities/kmeans_anchors.py without lvis,
pandas, tqdm and scikit-learn) and print the `anchors:` line of a hydra dataset file.
    python tools/make_anchors.py --ann lvis_v1_train.json --dset lvis --inp-dim 416 --extend-defaults
    python tools/make_anchors.py --ann instances_train2017.json --dset coco --inp-dim 416 --metric iou --k 9
`--metric euclid` (default) is the script's rule: the boxes with 0.2 < aspect < 5 in three area bands, k centres (default 3) of
(width, height, aspect, area) per band; `--extend-defaults` puts them in front of the stock anchors of each scale, as the reference's lvis.yaml
does.  `--metric iou` clusters (w, h) under the 1 - IoU distance into k anchors (default 9) split over the three scales.  The fitness (mean best
IoU, share of boxes with a best IoU >= 0.5) of the stock anchors and of the printed set follows."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def anchors_line(anchors):
    return "anchors: [" + ",\n          ".join("[" + ", ".join(f"[{w:.8f}, {h:.8f}]" for w, h in scale) + "]" for scale in anchors) + "]"


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ann", required=True, help="annotation JSON (COCO or LVIS format)")
    ap.add_argument("--dset", required=True, choices=["coco", "lvis"])
    ap.add_argument("--inp-dim", type=int, default=416)
    ap.add_argument("--metric", default="euclid", choices=["euclid", "iou"])
    ap.add_argument("--k", type=int, default=None, help="centres per band (euclid, default 3) or anchors in all (iou, default 9)")
    ap.add_argument("--n-init", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--extend-defaults", action="store_true", help="put the found anchors in front of the stock ones of each scale")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from object_detectors_amd import anchors as A
    feats = A.box_features(args.ann, args.dset, device=args.device)
    if args.metric == "euclid":
        found = A.reference_anchors(feats, args.dset, args.inp_dim, k=args.k or 3, n_init=args.n_init, seed=args.seed)
    else:
        found = A.iou_anchors(feats, args.dset, args.inp_dim, k=args.k or 9, n_init=args.n_init, seed=args.seed)
    new = A.extend_anchors(A.STOCK_ANCHORS, found["anchors"]) if args.extend_defaults else found["anchors"]
    print(anchors_line(new))
    wh = (feats["features"][feats["keep"]][:, :2] * args.inp_dim).contiguous()
    for name, anchors in (("stock", A.STOCK_ANCHORS), ("new", new)):
        mean, share = A.fitness(wh, anchors)
        print(f"# {name}: mean best IoU {mean:.4f}, best IoU >= 0.5 for {100 * share:.2f} % of {wh.shape[0]} boxes")
    print(f"# passes per (problem, restart): {found['n_iter'].tolist()}, winners {found['best'].tolist()}")


if __name__ == "__main__":
    main()
