"""Mirror of the class re-weighting helper of yolo/utilities/custom.py: `IDFTransformer` (:163-262).

The reference builds a table of per-class statistics (document / instance frequencies and several idf variants) from the annotation file
and caches it as `<owd>/<dset>_files/idf.csv` (shipped in the repository for COCO and LVIS); YOLOForw reads class weights / logit
multipliers from it (yolo_forw.py:35-67) and calls `forward(targets)` for the per-batch idf row when `tfidf_batch` is set (:87-91).
Both paths are provided: a cached table is read; without one the table is built from the annotation file on the GPU
(object_detectors_amd/dataset_stats.py: no pycocotools / lvis) and, when $owd is set, cached where the reference caches it."""
import csv
import os

import torch
import torch.nn as nn


class IDFTransformer(nn.Module):
    def __init__(self, annfile=None, dset_name="coco", device="cuda", reduce="sum", reduce_mini_batch=True, csv_path=None, num_classes=None):
        super().__init__()
        self.device = device
        self.idf_weights = {}
        if csv_path is None:
            owd = os.getenv("owd")
            if owd is not None:
                csv_path = os.path.join(owd, dset_name + "_files", "idf.csv")
        if csv_path is not None and os.path.exists(csv_path):
            with open(csv_path, newline="") as f:
                rows = list(csv.DictReader(f))
            for k in rows[0].keys():
                try:
                    vals = [float(r[k]) for r in rows]
                except ValueError:
                    continue                                   # string columns are skipped, as the reference does (custom.py:251-252)
                self.idf_weights[k] = torch.tensor(vals, dtype=torch.float32, device=device)
            self.num_classes = len(rows)
        elif annfile is not None and os.path.exists(self._annotation_path(annfile)):
            # custom.py:177-247: build the table (on the GPU, whatever `device` the weights are kept on) and cache it under $owd
            from ... import dataset_stats
            table = dataset_stats.idf_table(self._annotation_path(annfile), dset_name)
            for k in dataset_stats.TO_CSV_COLUMNS:
                self.idf_weights[k] = table[k].to(device=device, dtype=torch.float32)
            self.num_classes = int(table["category_ids"].numel())
            if csv_path is not None:                           # $owd is set (custom.py:247), or the caller named the file
                dataset_stats.write_idf_csv(csv_path, table, "present")
        elif num_classes is not None:
            self.num_classes = num_classes                     # per-batch idf only
        else:
            raise FileNotFoundError("IDFTransformer: no cached idf.csv (set $owd or pass csv_path) and no annotation file to build it from "
                                    f"(annfile={annfile!r})")

    @staticmethod
    def _annotation_path(annfile):
        owd = os.getenv("owd")                                 # custom.py:170: the annotation file is given relative to $owd
        return annfile if owd is None or os.path.isabs(annfile) else os.path.join(owd, annfile)

    def forward(self, targets):
        """custom.py:257-262: smoothed idf of the classes present in this mini-batch."""
        t = torch.stack([torch.bincount(x["category_id"], minlength=self.num_classes) for x in targets])
        t[t > 0] = 1
        t = t.sum(axis=0)
        return torch.log((len(targets) + 1) / (t + 1)) + 1
