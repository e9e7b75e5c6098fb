#!/usr/bin/env python3
"""Build the TF-IDF class table of a COCO- or LVIS-format annotation file on the GPU (the reference's yolo/utilities/get_idf.py without
pycocotools / lvis).
    python tools/make_idf.py --ann instances_train2017.json --dset coco --out coco_files/idf.csv
    python tools/make_idf.py --ann instances_train2017.json --dset coco --out coco_files/idf_91.csv --layout labels --num-classes 91
`--layout present` (default) writes one row per category that occurs: the file IDFTransformer / YOLOForw read as `<owd>/<dset>_files/idf.csv`.
`--layout labels` writes row k for label k, rows of ones for the background and absent labels: the `idf_{num_classes}.csv` that the
torchvision models' train.py reads."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ann", required=True, help="annotation JSON (COCO or LVIS format)")
    ap.add_argument("--dset", required=True, choices=["coco", "lvis"])
    ap.add_argument("--out", required=True, help="csv to write")
    ap.add_argument("--layout", default="present", choices=["present", "labels"])
    ap.add_argument("--num-classes", type=int, default=None, help="rows of the labels layout (default: the largest present id + 1)")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    from object_detectors_amd import dataset_stats
    table = dataset_stats.idf_table(args.ann, args.dset, device=args.device)
    dataset_stats.write_idf_csv(args.out, table, args.layout, num_classes=args.num_classes)
    print(f"{args.out}: {table['category_ids'].numel()} present categories, {table['n_images']} images, "
          f"{int(table['instance_freq'].sum())} annotations")


if __name__ == "__main__":
    main()
