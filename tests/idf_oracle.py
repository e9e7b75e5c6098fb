"""The reference's TF-IDF table, restated literally for the tests (yolo/utilities/get_idf.py:19-85 = custom.py:176-247): the categories of
each image's annotations, then per image one bincount, one coo_matrix and one vstack, the column mask and the formulas on numpy matrices
with scipy.special.ndtri.  pycocotools' and lvis' index (createIndex: annotations grouped by image_id, images keyed by id) is restated in
`image_categories`.  The vstack makes the loop quadratic in the number of images: use it on small sets only."""
import numpy as np
import pandas as pd
from scipy.sparse import coo_matrix, vstack
from scipy.special import ndtri

FAMILY = ["smooth", "raw", "prob", "normit", "gombit", "base2", "base10"]
COLUMNS14 = FAMILY + [c + "_obj" for c in FAMILY]


def image_categories(dataset, dset_name):
    """ims (one list of category ids per image, in the order of the images' ids) and num_classes = last category id + 1."""
    img_to_anns = {}
    for ann in dataset.get("annotations", []):
        img_to_anns.setdefault(ann["image_id"], []).append(ann)
    imgs = {im["id"]: im for im in dataset.get("images", [])}
    cat_ids = [c["id"] for c in dataset["categories"]]
    if dset_name != "coco":
        cat_ids = sorted(cat_ids)                          # lvis.get_cat_ids sorts; pycocotools' getCatIds keeps the file's order
    num_classes = cat_ids[-1] + 1
    ims = [[a["category_id"] for a in img_to_anns.get(i, [])] for i in imgs]
    return ims, num_classes


def stacked_counts(ims, num_classes):
    """The loop of get_idf.py:44-56: `final` [images, num_classes], the newest image on top."""
    final = 0
    for k, im in enumerate(ims):
        cats = np.array(im, dtype=int)
        cats = np.bincount(cats, minlength=num_classes)
        cats = np.array([cats])
        cats = coo_matrix(cats)
        final = cats if k == 0 else vstack([cats, final])
    return final


def frequencies(ims, num_classes):
    """instance_freq, img_freq over ALL num_classes columns (before the mask), as int64 vectors."""
    final = stacked_counts(ims, num_classes).tocsr()
    return np.asarray(final.sum(axis=0))[0].astype(np.int64), np.asarray((final > 0).sum(axis=0))[0].astype(np.int64)


def formulas(doc_freq, instance_freq, n_docs):
    """get_idf.py:63-84 on 1 x R integer matrices doc_freq / instance_freq (what `.sum(axis=0)` of the sparse matrix gives)."""
    df = pd.DataFrame()
    with np.errstate(divide="ignore", invalid="ignore"):
        pobs = doc_freq / n_docs
        pobs = np.array(pobs)[0]
        df["smooth"] = (np.log((n_docs + 1) / (doc_freq + 1)) + 1).tolist()[0]
        df["raw"] = (np.log((n_docs) / (doc_freq))).tolist()[0]
        df["prob"] = (np.log((n_docs - doc_freq) / (doc_freq))).tolist()[0]
        df["normit"] = -ndtri(pobs)
        df["gombit"] = -np.log(-np.log(1 - pobs))
        df["base2"] = -np.log2(pobs)
        df["base10"] = -np.log10(pobs)
        N = instance_freq.sum()
        pobs = instance_freq / N
        pobs = np.array(pobs)[0]
        df["smooth_obj"] = (np.log((N + 1) / (instance_freq + 1)) + 1).tolist()[0]
        df["raw_obj"] = (np.log((N) / (instance_freq))).tolist()[0]
        df["prob_obj"] = (np.log((N - instance_freq) / (instance_freq))).tolist()[0]
        df["normit_obj"] = -ndtri(pobs)
        df["gombit_obj"] = -np.log(-np.log(1 - pobs))
        df["base2_obj"] = -np.log2(pobs)
        df["base10_obj"] = -np.log10(pobs)
    df["img_freq"] = doc_freq.tolist()[0]
    df["instance_freq"] = instance_freq.tolist()[0]
    return df


def reference_table(ims, num_classes):
    """get_idf.py:44-84 -> (DataFrame of the present categories, their ids)."""
    final = stacked_counts(ims, num_classes)
    mask = final.sum(axis=0) > 0
    mask = mask.tolist()[0]
    final = final.tocsr()[:, mask]
    doc_freq = (final > 0).sum(axis=0)
    instance_freq = final.sum(axis=0)
    return formulas(doc_freq, instance_freq, final.shape[0]), np.nonzero(mask)[0]


def dataset_table(dataset, dset_name):
    return reference_table(*image_categories(dataset, dset_name))


def table_from_frequencies(img_freq, instance_freq, n_images):
    return formulas(np.matrix(np.asarray(img_freq, dtype=np.int64)), np.matrix(np.asarray(instance_freq, dtype=np.int64)), int(n_images))


def float32_equal_or_neighbour(got, want):
    """Per element: float32(got) is float32(want) or one of its two neighbouring float32 values; infinities must agree exactly, NaN never
    passes.  (One float32 step is what a last-bit difference in float64 can move the float32 rounding by.)"""
    g = np.asarray(got, dtype=np.float64).astype(np.float32)
    w = np.asarray(want, dtype=np.float64).astype(np.float32)
    lo, hi = np.nextafter(w, np.float32(-np.inf)), np.nextafter(w, np.float32(np.inf))
    finite = np.isfinite(w)
    return np.where(finite, (g == w) | (g == lo) | (g == hi), g == w)


def max_relative_difference(got, want):
    g, w = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    m = np.isfinite(w) & (w != 0)
    return float(np.max(np.abs(g[m] - w[m]) / np.abs(w[m]))) if m.any() else 0.0
