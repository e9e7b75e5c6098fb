"""Host-side checks of the TF-IDF table builder (object_detectors_amd/dataset_stats.py): the restated reference loop against the table the
reference recorded, the annotation rules, the two csv layouts and the command-line tool.  No GPU."""
import csv
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import idf_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
PRESENT = os.path.join(GOLDEN, "idf_coco_present.csv")         # the reference's yolo/coco_files/idf.csv (COCO train2017)
LABELS = os.path.join(GOLDEN, "idf_coco_labels.csv")           # the reference's torchvision_models/coco_files/idf_91.csv
COCO_IMAGES = 118287
# COCO's 80 category ids: 1..90 without these ten
COCO_ABSENT = (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)


def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def fixture_table():
    rows = read_csv(PRESENT)
    t = {k: np.array([float(r[k]) for r in rows]) for k in rows[0] if k not in ("names", "class")}
    t["names"] = [r["names"] for r in rows]
    return t


def test_oracle_reproduces_the_recorded_table():
    t = fixture_table()
    assert len(t["smooth"]) == 80
    assert round(t["img_freq"][0] * np.exp(t["raw"][0])) == COCO_IMAGES and int(t["instance_freq"].sum()) == 860001
    df = idf_oracle.table_from_frequencies(t["img_freq"], t["instance_freq"], COCO_IMAGES)
    for c in idf_oracle.COLUMNS14:
        assert np.array_equal(df[c].to_numpy().astype(np.float32), t[c].astype(np.float32)), c
        assert np.abs(df[c].to_numpy() - t[c]).max() < 1e-14, c


def test_oracle_loop_on_a_hand_made_set():
    ims = [[1, 1, 3], [], [3], [1, 5, 5, 5]]
    inst, img = idf_oracle.frequencies(ims, 7)
    assert inst.tolist() == [0, 3, 0, 2, 0, 3, 0] and img.tolist() == [0, 2, 0, 2, 0, 1, 0]
    df, ids = idf_oracle.reference_table(ims, 7)
    assert ids.tolist() == [1, 3, 5] and df["img_freq"].tolist() == [2, 2, 1] and df["instance_freq"].tolist() == [3, 2, 3]
    assert df["raw"][2] == np.log(4 / 1) and df["smooth_obj"][1] == np.log(9 / 3) + 1


def test_formula_header_matches_scipy_on_the_host(tmp_path):
    """csrc/idf_formulas.h (what the kernel evaluates) compiled for the host, against the oracle's numpy / scipy formulas: ndtri agrees to
    the last bit (the same Cephes operations), the logarithms to a few float64 steps of either libm."""
    src = tmp_path / "f.cpp"
    src.write_text('#include "idf_formulas.h"\n#include <stdio.h>\nint main(){ double t, f; while (scanf("%lf %lf", &t, &f) == 2) { double o[7]; '
                   'mi355::idf_columns(t, f, o); for (int i = 0; i < 7; ++i) printf("%.17g ", o[i]); printf("\\n"); } return 0; }\n')
    exe = tmp_path / "f"
    subprocess.run(["g++", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "object_detectors_amd", "csrc"), str(src), "-o", str(exe)], check=True)
    rng = np.random.default_rng(0)
    T = COCO_IMAGES
    f = np.unique(np.concatenate([rng.integers(1, T, 3000), [1, 2, 3, T - 1, T, T // 2, 16008, 16009, 102278, 102279]]))
    out = subprocess.run([str(exe)], input="\n".join(f"{T} {x}" for x in f), capture_output=True, text=True, check=True).stdout
    got = np.array([[float(v) for v in line.split()] for line in out.splitlines()])
    want = idf_oracle.table_from_frequencies(f, f, T)            # the first family only depends on (T, f)
    for k, c in enumerate(idf_oracle.FAMILY):
        w = want[c].to_numpy()
        assert np.array_equal(np.isinf(got[:, k]), np.isinf(w)) and not np.isnan(got[:, k]).any(), c
        assert np.array_equal(np.signbit(got[:, k][np.isinf(w)]), np.signbit(w[np.isinf(w)])), c
        if c == "normit":
            assert np.array_equal(got[:, k], w)
        else:
            assert idf_oracle.max_relative_difference(got[:, k], w) < 4 * 2.0 ** -52, c
    assert np.isneginf(got[-1, [2, 3, 4]]).all()                  # f == T: p = 1


# ---- dataset_arrays
def coco_dict():
    return {"images": [{"id": 10}, {"id": 7}, {"id": 99}, {"id": 3}],                              # 99 has no annotation
            "categories": [{"id": 2, "name": "b"}, {"id": 5, "name": "e"}, {"id": 9, "name": "i"}],
            "annotations": [{"id": 1, "image_id": 10, "category_id": 5}, {"id": 2, "image_id": 10, "category_id": 5},
                            {"id": 3, "image_id": 7, "category_id": 2}, {"id": 4, "image_id": 1234, "category_id": 9},   # unknown image
                            {"id": 5, "image_id": 3, "category_id": 5}, {"id": 6, "image_id": 3, "category_id": 2}]}


def lvis_dict():
    d = coco_dict()
    d["categories"] = [{"id": 9, "name": "i", "frequency": "r"}, {"id": 2, "name": "b", "frequency": "f"}, {"id": 5, "name": "e", "frequency": "c"}]
    for im in d["images"]:
        im["neg_category_ids"], im["not_exhaustive_category_ids"] = [], []
    return d


def counts_of(a):
    inst = np.bincount(a["category_index"], minlength=a["n_categories"])
    pairs = np.unique(a["image_index"].astype(np.int64) * a["n_categories"] + a["category_index"])
    return inst, np.bincount(pairs % a["n_categories"], minlength=a["n_categories"])


@pytest.mark.parametrize("make, kind", [(coco_dict, "coco"), (lvis_dict, "lvis")])
def test_dataset_arrays_follow_the_reference(make, kind, tmp_path):
    from object_detectors_amd import dataset_stats
    d = make()
    a = dataset_stats.dataset_arrays(d, kind)
    ims, num_classes = idf_oracle.image_categories(d, kind)
    assert a["n_categories"] == num_classes == 10 and a["n_images"] == len(ims) == 4
    assert a["image_index"].dtype == np.int32 and a["category_index"].dtype == np.int32 and len(a["image_index"]) == 5
    inst, img = counts_of(a)
    o_inst, o_img = idf_oracle.frequencies(ims, num_classes)
    assert np.array_equal(inst, o_inst) and np.array_equal(img, o_img)
    assert inst[9] == 0                                           # its only annotation belongs to an image that is not listed
    assert a["names"] == {2: "b", 5: "e", 9: "i"}
    import json
    p = tmp_path / "ann.json"
    p.write_text(json.dumps(d))
    b = dataset_stats.dataset_arrays(str(p), kind)
    assert np.array_equal(a["image_index"], b["image_index"]) and np.array_equal(a["category_index"], b["category_index"])


def test_dataset_arrays_coco_takes_the_last_listed_category():
    from object_detectors_amd import dataset_stats
    d = coco_dict()
    d["categories"] = [{"id": 9, "name": "i"}, {"id": 2, "name": "b"}, {"id": 5, "name": "e"}]
    d["annotations"] = [a for a in d["annotations"] if a["category_id"] != 9]
    assert dataset_stats.dataset_arrays(d, "coco")["n_categories"] == 6 == idf_oracle.image_categories(d, "coco")[1]
    assert dataset_stats.dataset_arrays(d, "lvis")["n_categories"] == 10 == idf_oracle.image_categories(d, "lvis")[1]


def test_dataset_arrays_without_annotations_raises():
    from object_detectors_amd import dataset_stats
    d = coco_dict()
    d["annotations"] = []
    with pytest.raises(ValueError):
        dataset_stats.dataset_arrays(d, "coco")
    d = coco_dict()
    d["annotations"] = [a for a in d["annotations"] if a["image_id"] == 1234]
    with pytest.raises(ValueError):
        dataset_stats.dataset_arrays(d, "coco")
    with pytest.raises(ValueError):
        dataset_stats.dataset_arrays(coco_dict(), "voc")


# ---- csv layouts
def test_both_layouts_round_trip_through_idftransformer(tmp_path):
    import torch
    from object_detectors_amd import dataset_stats
    from object_detectors_amd.yolo.utilities.custom import IDFTransformer
    t = fixture_table()
    t["category_ids"] = [k for k in range(1, 91) if k not in COCO_ABSENT]
    p = str(tmp_path / "a" / "idf.csv")
    dataset_stats.write_idf_csv(p, t, "present")
    assert read_csv(p)[0].keys() == set(dataset_stats.TO_CSV_COLUMNS) | {"names"}
    assert list(read_csv(p)[0].keys())[:16] == list(dataset_stats.TO_CSV_COLUMNS)
    idf = IDFTransformer(csv_path=p, device="cpu")
    assert idf.num_classes == 80 and set(idf.idf_weights) == set(dataset_stats.TO_CSV_COLUMNS)
    for k in dataset_stats.TO_CSV_COLUMNS:
        assert torch.equal(idf.idf_weights[k], torch.tensor(t[k], dtype=torch.float32)), k
    t2 = dict(t, names=None)
    dataset_stats.write_idf_csv(p, t2, "present")
    assert list(read_csv(p)[0].keys()) == list(dataset_stats.TO_CSV_COLUMNS)
    q = str(tmp_path / "idf_91.csv")
    dataset_stats.write_idf_csv(q, t, "labels", num_classes=91)
    idf = IDFTransformer(csv_path=q, device="cpu")
    assert idf.num_classes == 91
    present = torch.tensor(t["category_ids"])
    for k in dataset_stats.TO_CSV_COLUMNS:
        assert torch.equal(idf.idf_weights[k][present], torch.tensor(t[k], dtype=torch.float32)), k
        assert float(idf.idf_weights[k][0]) == 1.0 and float(idf.idf_weights[k][12]) == 1.0
    # the way detection/train.py:104-135 reads it
    import pandas as pd
    df = pd.read_csv(q)
    assert len(df) == 91 and df["smooth"][0] == 1 and df["instance_freq"][1] == 262465 and df["names"][1] == "person"
    with pytest.raises(ValueError):
        dataset_stats.write_idf_csv(q, t, "labels", num_classes=90)
    with pytest.raises(ValueError):
        dataset_stats.write_idf_csv(q, t, "wide")


def test_labels_layout_reproduces_the_recorded_file(tmp_path):
    """The recorded idf_91.csv, from the recorded present table.  The labels a row of ones stands at are read from the recorded file: they are
    0 and COCO's absent ids, except that the file leaves label 11 empty and has `fire hydrant` (COCO id 11) at 12."""
    from object_detectors_amd import dataset_stats
    want = read_csv(LABELS)
    assert len(want) == 91
    ones = [k for k, r in enumerate(want) if r["class"] == "-1"]
    assert ones == [0, 11] + list(COCO_ABSENT[1:])
    t = fixture_table()
    t["category_ids"] = [k for k in range(91) if k not in ones]
    q = str(tmp_path / "idf_91.csv")
    dataset_stats.write_idf_csv(q, t, "labels", num_classes=91)
    got = read_csv(q)
    assert list(got[0].keys()) == list(want[0].keys()) and len(got) == 91
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["class"] == w["class"] and g["names"] == w["names"], k
        for c in dataset_stats.TO_CSV_COLUMNS:
            assert float(g[c]) == float(w[c]), (k, c)
    assert open(q).read() == open(LABELS).read()


def test_idftransformer_without_csv_or_annotations_raises(tmp_path, monkeypatch):
    from object_detectors_amd.yolo.utilities.custom import IDFTransformer
    monkeypatch.delenv("owd", raising=False)
    with pytest.raises(FileNotFoundError):
        IDFTransformer()
    with pytest.raises(FileNotFoundError):
        IDFTransformer(annfile=str(tmp_path / "missing.json"), dset_name="coco")
    monkeypatch.setenv("owd", str(tmp_path))
    with pytest.raises(FileNotFoundError):
        IDFTransformer(annfile="missing.json", dset_name="coco")
    assert IDFTransformer(num_classes=5, device="cpu").num_classes == 5


def test_device_entry_points_refuse_cpu_tensors():
    import torch
    from object_detectors_amd import dataset_stats
    z = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError):
        dataset_stats.category_frequencies(z, z, 2, 2)
    with pytest.raises(ValueError):
        dataset_stats.idf_columns(z, z, 2)


def test_make_idf_help_parses():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_idf.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--layout" in r.stdout and "--num-classes" in r.stdout
