"""The per-class TF-IDF table from the annotations, on the device (csrc/dstats_kernels.hip; include/mi355det.h, "Dataset statistics").

The reference builds the table that parameterises its re-weighting - `smooth`, `raw`, `prob`, `normit`, `gombit`, `base2`, `base10`, their
`_obj` twins, `img_freq` and `instance_freq` per class - with yolo/utilities/get_idf.py or the build branch of IDFTransformer
(yolo/utilities/custom.py:176-247): pycocotools / lvis to list each image's categories, then one bincount, one coo_matrix and one vstack
per image.  Here:

    arrays = dataset_arrays("instances_train.json", "coco")        # host: one (image, category) index pair per annotation
    table = idf_table(arrays)                                       # device: frequencies, compaction, the 14 columns
    write_idf_csv("coco_files/idf.csv", table, "present")           # what IDFTransformer / YOLOForw read
    write_idf_csv("coco_files/idf_91.csv", table, "labels")         # what the torchvision models' train.py reads (detection/train.py:104)

No pycocotools, no lvis, no scipy; the tensors must live on the GPU and nothing falls back to torch ops."""
import csv
import json
import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream_ptr

FAMILY = ("smooth", "raw", "prob", "normit", "gombit", "base2", "base10")
TABLE_ROWS = FAMILY + tuple(c + "_obj" for c in FAMILY)                       # the row order of mi355det_idf_table
# the column order DataFrame.to_csv gives get_idf.py's frame (get_idf.py:65-85)
TO_CSV_COLUMNS = FAMILY + ("smooth_obj", "raw_obj", "prob_obj", "normit_obj", "gombit_obj", "base2_obj", "base10_obj", "img_freq", "instance_freq")
# the column order of the label-indexed file the reference ships for the torchvision models (torchvision_models/coco_files/idf_91.csv)
LABEL_COLUMNS = ("class", "smooth", "raw", "prob", "gombit", "normit", "base2", "base10", "smooth_obj", "raw_obj", "prob_obj", "normit_obj",
                 "gombit_obj", "base2_obj", "base10_obj", "instance_freq", "img_freq", "names")


def _device_i32(t, what):
    if not (torch.is_tensor(t) and t.is_cuda):
        raise ValueError(f"{what} needs CUDA/HIP tensors (no CPU fallback)")
    if t.dtype != torch.int32 or t.dim() != 1:
        raise ValueError(f"{what}: int32 vectors expected")
    return t.contiguous()


def category_frequencies(image_index, category_index, n_images, n_categories):
    """mi355det_category_frequencies: int32 device vectors [A], one (image, category) index pair per annotation -> instance_freq, img_freq
    int32 [n_categories].  Raises ValueError if an index lies outside [0, n_images) / [0, n_categories)."""
    im, cat = _device_i32(image_index, "category_frequencies"), _device_i32(category_index, "category_frequencies")
    if im.shape != cat.shape:
        raise ValueError("category_frequencies: one category index per image index")
    n_images, n_categories = int(n_images), int(n_categories)
    dev = im.device
    L = _lib.lib()
    ws_bytes = int(L.mi355det_category_frequencies_workspace(n_images, n_categories))
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    out = torch.empty((2, max(n_categories, 0)), dtype=torch.int32, device=dev)
    errors = torch.empty(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(L.mi355det_category_frequencies(ptr(im), ptr(cat), int(im.shape[0]), n_images, n_categories, ptr(out[0]), ptr(out[1]), ptr(errors),
                                              ptr(ws), ws_bytes, stream_ptr()), "category_frequencies")
    bad = int(errors.item())
    if bad:
        raise ValueError(f"category_frequencies: {bad} annotation(s) with an image index outside [0, {n_images}) or a category index outside "
                         f"[0, {n_categories})")
    return out[0], out[1]


def idf_columns(img_freq, instance_freq, n_images):
    """mi355det_idf_table: int32 device vectors [R] of the categories that occur -> float64 [14, R], rows in TABLE_ROWS order."""
    df, nf = _device_i32(img_freq, "idf_columns"), _device_i32(instance_freq, "idf_columns")
    if df.shape != nf.shape:
        raise ValueError("idf_columns: one instance count per image count")
    R = int(df.shape[0])
    table = torch.empty((len(TABLE_ROWS), R), dtype=torch.float64, device=df.device)
    with torch.cuda.device(df.device):
        check(_lib.lib().mi355det_idf_table(ptr(df), ptr(nf), R, int(n_images), ptr(table), stream_ptr()), "idf_table")
    return table


def load_dataset(dataset):
    """An annotation dict, or the path of its JSON -> the dict."""
    if isinstance(dataset, (str, os.PathLike)):
        with open(dataset) as f:
            dataset = json.load(f)
    return dataset


def listed_annotations(dataset):
    """The walk-the-images rule shared by dataset_arrays and anchors.box_arrays: (img_ids, keep, pos) with img_ids the sorted distinct ids of
    `images`, keep a bool mask over `annotations` (False for an annotation whose image_id `images` does not list) and pos the index into
    img_ids of every kept annotation."""
    img_ids = np.unique(np.asarray([im["id"] for im in dataset.get("images") or []], dtype=np.int64))
    ann_img = np.asarray([a["image_id"] for a in dataset.get("annotations") or []], dtype=np.int64)
    if img_ids.size and ann_img.size:
        pos = np.minimum(np.searchsorted(img_ids, ann_img), img_ids.size - 1)
        keep = img_ids[pos] == ann_img
        return img_ids, keep, pos[keep]
    return img_ids, np.zeros(ann_img.size, bool), np.zeros(0, np.int64)


def dataset_arrays(dataset, dset_name="coco"):
    """A COCO or LVIS annotation dict (or the path of its JSON) -> {'image_index', 'category_index': int32 numpy [A], 'n_images',
    'n_categories', 'names': {category id: name}} by the rules of the reference's loop (custom.py:178-201):
      n_categories   last category id + 1: the last listed category for coco (pycocotools' getCatIds keeps the file's order), the largest
                     id for lvis (get_cat_ids sorts);
      n_images       every distinct id in `images`, annotated or not;
      annotations    of an image id that `images` does not list are dropped (the reference walks the images, not the annotations).
    ValueError if no annotation is left."""
    dataset = load_dataset(dataset)
    if dset_name not in ("coco", "lvis"):
        raise ValueError("dset_name must be 'coco' or 'lvis'")
    cats = dataset.get("categories") or []
    if not cats:
        raise ValueError("dataset_arrays: the dataset lists no categories")
    cat_ids = [int(c["id"]) for c in cats]
    n_categories = (cat_ids[-1] if dset_name == "coco" else max(cat_ids)) + 1
    img_ids, keep, pos = listed_annotations(dataset)
    ann_cat = np.asarray([a["category_id"] for a in dataset.get("annotations") or []], dtype=np.int64)[keep]
    if pos.size == 0:
        raise ValueError("dataset_arrays: no annotation of a listed image, nothing to count")
    if ann_cat.min() < 0 or ann_cat.max() >= n_categories:
        raise ValueError(f"dataset_arrays: category ids must lie in [0, {n_categories}) (the last category id + 1)")
    return {"image_index": pos.astype(np.int32), "category_index": ann_cat.astype(np.int32), "n_images": int(img_ids.size),
            "n_categories": int(n_categories), "names": {int(c["id"]): c.get("name", "") for c in cats}}


def idf_table(dataset_or_arrays, dset_name="coco", device="cuda"):
    """The table of the categories that occur, in ascending id order (absent ones are dropped, as `final.tocsr()[:, mask]` does):
    {column: float64 tensor [R] for the 14 columns of TABLE_ROWS, 'img_freq', 'instance_freq', 'category_ids': int64 [R], 'n_images',
    'names': [R] strings or None}, all on `device`.  Takes what dataset_arrays takes, or its result (index arrays as numpy or tensors)."""
    a = dataset_or_arrays
    if not (isinstance(a, dict) and "image_index" in a):
        a = dataset_arrays(a, dset_name)
    dev = torch.device(device)
    to_dev = lambda v: torch.as_tensor(v).to(device=dev, dtype=torch.int32)
    inst, img = category_frequencies(to_dev(a["image_index"]), to_dev(a["category_index"]), a["n_images"], a["n_categories"])
    ids = torch.nonzero(inst > 0).flatten()
    if ids.numel() == 0:
        raise ValueError("idf_table: no annotations")
    inst, img = inst[ids].contiguous(), img[ids].contiguous()
    cols = idf_columns(img, inst, a["n_images"])
    table = {name: cols[k] for k, name in enumerate(TABLE_ROWS)}
    table.update(img_freq=img.long(), instance_freq=inst.long(), category_ids=ids, n_images=int(a["n_images"]))
    names = a.get("names")
    table["names"] = None if not names else [names.get(int(i), "") for i in ids.tolist()]
    return table


# ---- long-tail baselines: the tail mask of Equalization loss v1 and repeat-factor sampling
def _arrays_and_frequencies(dataset_or_arrays, dset_name, device):
    a = dataset_or_arrays
    if not (isinstance(a, dict) and "image_index" in a):
        a = dataset_arrays(a, dset_name)
    dev = torch.device(device)
    im = torch.as_tensor(a["image_index"]).to(device=dev, dtype=torch.int32)
    cat = torch.as_tensor(a["category_index"]).to(device=dev, dtype=torch.int32)
    _inst, img = category_frequencies(im, cat, a["n_images"], a["n_categories"])
    return a, im, cat, img


def eql_tail_mask(dataset_or_arrays, lam=1.76e-3, dset_name="lvis", device="cuda"):
    """Equalization loss v1 (Tan et al., CVPR 2020): uint8 [n_categories] on `device`, 1 where the category's image frequency
    img_freq / n_images (float64) is below `lam` - a category that never occurs counts as tail - and 0 at index 0, the background column
    of the box classifier.  Takes what idf_table takes."""
    a, _im, _cat, img = _arrays_and_frequencies(dataset_or_arrays, dset_name, device)
    return tail_from_frequencies(img, a["n_images"], lam)


def tail_from_frequencies(img_freq, n_images, lam=1.76e-3):
    """eql_tail_mask's rule on a vector of image counts, on whichever device it lives: [img_freq / n_images < lam] in float64, 0 at index 0."""
    tail = (img_freq.double() / float(n_images) < float(lam)).to(torch.uint8)
    tail[0] = 0
    return tail


def repeat_factors(dataset_or_arrays, t=1e-3, dset_name="lvis", device="cuda"):
    """Repeat-factor sampling (Gupta et al., LVIS 2019): float64 [n_images] on `device`, in listed_annotations' image order (the sorted
    distinct ids of `images`): r_i = max over image i's annotations of max(1, sqrt(t / f_c)), f_c = img_freq_c / n_images; 1 for an image
    without annotations (ops.repeat_factors, mi355det_repeat_factors).  Takes what idf_table takes."""
    from . import ops
    a, im, cat, img = _arrays_and_frequencies(dataset_or_arrays, dset_name, device)
    return ops.repeat_factors(im, cat, img, a["n_images"], t)


class RepeatFactorSampler(torch.utils.data.Sampler):
    """detectron2's RepeatFactorTrainingSampler (restated from memory) on the host, one epoch per iteration: with a CPU generator seeded
    seed + epoch, image i appears floor(r_i) + (u_i < frac(r_i)) times, u = torch.rand(n_images); the list is shuffled with
    torch.randperm (unless shuffle=False), cut to a multiple of `world` and rank `rank` yields [rank::world]."""

    def __init__(self, repeat_factors, seed=0, rank=0, world=1, shuffle=True):
        r = torch.as_tensor(repeat_factors).detach().to("cpu", torch.float64).reshape(-1)
        if not bool((r >= 1).all()):
            raise ValueError("RepeatFactorSampler: repeat factors are >= 1")
        if not (0 <= int(rank) < int(world)):
            raise ValueError("RepeatFactorSampler: need 0 <= rank < world")
        self._whole = torch.floor(r)
        self._frac = r - self._whole
        self.seed, self.rank, self.world, self.shuffle, self.epoch = int(seed), int(rank), int(world), bool(shuffle), 0

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def _indices(self):
        g = torch.Generator()
        g.manual_seed(self.seed + self.epoch)
        u = torch.rand(self._whole.numel(), generator=g)
        reps = (self._whole + (u < self._frac).to(torch.float64)).to(torch.int64)
        idx = torch.repeat_interleave(torch.arange(reps.numel()), reps)
        if self.shuffle:
            idx = idx[torch.randperm(idx.numel(), generator=g)]
        idx = idx[:idx.numel() - idx.numel() % self.world]
        return idx[self.rank::self.world]

    def __iter__(self):
        return iter(self._indices().tolist())

    def __len__(self):
        return int(self._indices().numel())


def _host_columns(table, columns):
    out = {}
    for c in columns:
        v = table[c]
        out[c] = v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)
    return out


def write_idf_csv(path, table, layout="present", names=None, num_classes=None):
    """Write a table (idf_table's result, or any dict with the same columns) as the csv the reference's consumers read.
      layout="present"   one row per present category, the columns get_idf.py's to_csv writes (TO_CSV_COLUMNS), plus `names` when known:
                         `<owd>/<dset>_files/idf.csv` of IDFTransformer / YOLOForw;
      layout="labels"    row k is label k (= category id k) for k < num_classes (default: the largest present id + 1), columns
                         LABEL_COLUMNS; label 0 (the background) and every absent label are rows of ones with class -1: the
                         `idf_{num_classes}.csv` of detection/train.py:104.  Needs table['category_ids'].
    `names`: per present row, a list or a {category id: name} dict; default table['names']."""
    if layout not in ("present", "labels"):
        raise ValueError("layout must be 'present' or 'labels'")
    cols = _host_columns(table, TO_CSV_COLUMNS)
    R = len(cols["smooth"])
    ids = None if table.get("category_ids") is None else [int(i) for i in _host_columns(table, ["category_ids"])["category_ids"]]
    if names is None:
        names = table.get("names")
    if isinstance(names, dict):
        if ids is None:
            raise ValueError("write_idf_csv: names by category id need table['category_ids']")
        names = [names.get(i, "") for i in ids]
    if names is not None and len(names) != R:
        raise ValueError("write_idf_csv: one name per present category")
    cell = lambda c, r: str(int(cols[c][r])) if c in ("img_freq", "instance_freq") else repr(float(cols[c][r]))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        if layout == "present":
            header = list(TO_CSV_COLUMNS) + (["names"] if names is not None else [])
            w.writerow(header)
            for r in range(R):
                w.writerow([cell(c, r) for c in TO_CSV_COLUMNS] + ([names[r]] if names is not None else []))
            return
        if ids is None:
            raise ValueError("write_idf_csv: layout 'labels' needs table['category_ids']")
        K = max(ids) + 1 if num_classes is None else int(num_classes)
        if max(ids) >= K or min(ids) < 0:
            raise ValueError(f"write_idf_csv: category ids must lie in [0, {K})")
        row_of = {i: r for r, i in enumerate(ids)}
        w.writerow(LABEL_COLUMNS)
        for k in range(K):
            r = row_of.get(k)
            if k == 0 or r is None:
                w.writerow(["-1"] + ["1"] * (len(LABEL_COLUMNS) - 1))
            else:
                w.writerow([str(r)] + [cell(c, r) for c in LABEL_COLUMNS[1:-1]] + [names[r] if names is not None else ""])
