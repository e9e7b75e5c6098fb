"""The TF-IDF class table on the device (object_detectors_amd/dataset_stats.py, csrc/dstats_kernels.hip) against the restated reference loop
(tests/idf_oracle.py) and the table the reference recorded for COCO train2017 (tests/golden/idf_coco_present.csv).

Frequencies are integers and must be equal.  The 14 columns are float64 from the device's log / log2 / log10 and the restated ndtri, which may
differ from numpy's in the last float64 bit; every consumer casts to float32, so a column passes if its float32 value is the expected float32
value or one of its two neighbours (idf_oracle.float32_equal_or_neighbour), infinities and their signs exactly, never NaN."""
import csv
import json
import os

import numpy as np
import pytest

from tests import idf_oracle

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT = os.path.join(ROOT, "tests", "golden", "idf_coco_present.csv")
COCO_IMAGES = 118287
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_counts(im, cat, n_images, n_cats):
    from object_detectors_amd import dataset_stats
    inst, img = dataset_stats.category_frequencies(T(im.astype(np.int32)), T(cat.astype(np.int32)), n_images, n_cats)
    return inst, img


def oracle_counts(im, cat, n_images, n_cats):
    ims = [[] for _ in range(n_images)]
    for i, c in zip(im.tolist(), cat.tolist()):
        ims[i].append(c)
    return idf_oracle.frequencies(ims, n_cats)


def check_counts(im, cat, n_images, n_cats):
    inst, img = device_counts(im, cat, n_images, n_cats)
    o_inst, o_img = oracle_counts(im, cat, n_images, n_cats)
    assert inst.dtype == torch.int32 and img.dtype == torch.int32 and tuple(inst.shape) == tuple(img.shape) == (n_cats,)
    assert np.array_equal(inst.cpu().numpy(), o_inst), (n_images, n_cats, len(im))
    assert np.array_equal(img.cpu().numpy(), o_img), (n_images, n_cats, len(im))
    return inst, img


def lds_limit():
    from object_detectors_amd import _lib
    return int(_lib.lib().mi355det_category_frequencies_lds_categories())


@pytest.fixture(scope="module")
def recorded():
    with open(PRESENT, newline="") as f:
        rows = list(csv.DictReader(f))
    return {k: np.array([float(r[k]) for r in rows]) for k in rows[0] if k not in ("names", "class")}


# ---------------------------------------------------------------------------------------------------------------- frequencies
@pytest.mark.parametrize("n_cats", [1, 32, 33, 64, 65])
def test_frequencies_at_the_bitmap_word_edges(n_cats):
    """Every n_images x A for this n_categories; the first annotations sit on ids 31, 32, 63 and 64 (those that exist), in image 0 and in the
    last image, so both sides of each bitmap word edge are set in the first and in the last bitmap row."""
    edges = [c for c in (31, 32, 63, 64) if c < n_cats]
    for n_images in (1, 3, 70):
        for A in (1, 63, 64, 65, 257, 1000):
            rng = np.random.default_rng(1000 * n_cats + 10 * n_images + A)
            im, cat = rng.integers(0, n_images, A), rng.integers(0, n_cats, A)
            k = min(len(edges), A // 2)
            cat[:k], im[:k] = edges[:k], 0
            cat[k:2 * k], im[k:2 * k] = edges[:k], n_images - 1
            check_counts(im, cat, n_images, n_cats)


def test_repeated_pairs_inside_and_across_wavefronts_and_workgroups():
    """A = 1000 over 3 images and 5 categories: 15 distinct pairs, each about 67 times - within one wavefront, in different wavefronts of a
    workgroup (256 threads) and in different workgroups.  Every image count is at most 3."""
    rng = np.random.default_rng(5)
    im, cat = rng.integers(0, 3, 1000), rng.integers(0, 5, 1000)
    inst, img = check_counts(im, cat, 3, 5)
    assert int(inst.sum()) == 1000 and img.tolist() == [3] * 5
    # the same pair in every slot
    inst, img = check_counts(np.full(1000, 2), np.full(1000, 4), 3, 5)
    assert inst.tolist() == [0, 0, 0, 0, 1000] and img.tolist() == [0, 0, 0, 0, 1]


def test_absent_category_empty_image_and_a_single_category():
    rng = np.random.default_rng(6)
    im = rng.choice([0, 1, 3, 4], 300)                       # image 2 has no annotation
    cat = rng.choice([0, 1, 2, 4, 5, 6], 300)                # category 3 has none
    inst, img = check_counts(im, cat, 5, 7)
    assert int(inst[3]) == 0 and int(img[3]) == 0 and int(img.max()) <= 4
    inst, img = check_counts(rng.integers(0, 70, 500), np.full(500, 17), 70, 40)      # all annotations in one category
    assert int(inst[17]) == 500 and int(inst.sum()) == 500


def test_lvis_category_count_and_both_sides_of_the_lds_limit():
    """1204 categories (LVIS v1: the LDS path), the largest count the LDS path takes, and one more (the global path), A = 2000."""
    limit = lds_limit()
    assert limit >= 1204
    for n_cats in (1204, limit, limit + 1):
        rng = np.random.default_rng(n_cats)
        im, cat = rng.integers(0, 70, 2000), rng.integers(0, n_cats, 2000)
        cat[:4], im[:4] = [0, n_cats - 1, 0, n_cats - 1], [0, 0, 69, 69]
        cat[4:300] = 7                                        # one heavy category among the many
        check_counts(im, cat, 70, n_cats)


def test_out_of_range_indices_raise_and_are_not_counted():
    from object_detectors_amd import dataset_stats
    rng = np.random.default_rng(8)
    for n_cats in (5, lds_limit() + 1):
        for bad_im, bad_cat in ((3, 0), (-1, 0), (0, n_cats), (0, -1), (2 ** 31 - 1, 2 ** 31 - 1)):
            im, cat = rng.integers(0, 3, 200), rng.integers(0, n_cats, 200)
            im[77], cat[77] = bad_im, bad_cat
            with pytest.raises(ValueError):
                device_counts(im, cat, 3, n_cats)
    torch.cuda.synchronize()
    check_counts(rng.integers(0, 3, 200), rng.integers(0, 5, 200), 3, 5)          # and the device is fine afterwards
    with pytest.raises(ValueError):
        dataset_stats.category_frequencies(T(np.zeros(3, np.int64)), T(np.zeros(3, np.int64)), 2, 2)      # int32 only


def test_two_runs_are_equal():
    rng = np.random.default_rng(9)
    im, cat = rng.integers(0, 70, 5000), rng.integers(0, 1204, 5000)
    a, b = device_counts(im, cat, 70, 1204), device_counts(im, cat, 70, 1204)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---------------------------------------------------------------------------------------------------------------------- table
def device_table(img_freq, instance_freq, n_images):
    from object_detectors_amd import dataset_stats
    t = dataset_stats.idf_columns(T(np.asarray(img_freq, np.int32)), T(np.asarray(instance_freq, np.int32)), n_images)
    assert t.dtype == torch.float64 and tuple(t.shape) == (14, len(img_freq))
    return {c: t[k].cpu().numpy() for k, c in enumerate(dataset_stats.TABLE_ROWS)}


def check_table(got, want, where=""):
    worst = 0.0
    for c in idf_oracle.COLUMNS14:
        g, w = np.asarray(got[c], np.float64), np.asarray(want[c], np.float64)
        assert not np.isnan(g).any(), (where, c)
        assert np.array_equal(np.isinf(g), np.isinf(w)) and np.array_equal(np.signbit(g[np.isinf(g)]), np.signbit(w[np.isinf(w)])), (where, c)
        ok = idf_oracle.float32_equal_or_neighbour(g, w)
        assert ok.all(), (where, c, g[~ok], w[~ok])
        worst = max(worst, idf_oracle.max_relative_difference(g, w))
    return worst


def test_table_reproduces_the_recorded_columns(recorded):
    got = device_table(recorded["img_freq"], recorded["instance_freq"], COCO_IMAGES)
    worst = check_table(got, recorded, "recorded")
    exact = sum(int(np.array_equal(got[c].astype(np.float32), recorded[c].astype(np.float32))) for c in idf_oracle.COLUMNS14)
    print(f"idf_table vs recorded COCO table: largest float64 relative difference {worst:.3e}; {exact} of 14 columns float32-equal")
    want = idf_oracle.table_from_frequencies(recorded["img_freq"], recorded["instance_freq"], COCO_IMAGES)
    check_table(got, want, "oracle")


def test_table_infinities_where_p_is_one():
    """4 images; set one: category 2 is in every image (p = 1 in the image family only); set two: a single category (p = 1 in both families,
    R = 1)."""
    one = [[2, 2, 5], [2], [2, 7, 7, 7], [5, 2]]
    two = [[3], [3, 3], [3], [3]]
    for name, ims in (("every image", one), ("single category", two)):
        df, ids = idf_oracle.reference_table(ims, 9)
        got = device_table(df["img_freq"].to_numpy(), df["instance_freq"].to_numpy(), len(ims))
        check_table(got, df, name)
        r = ids.tolist().index(2 if name == "every image" else 3)
        for c in ("prob", "normit", "gombit"):
            assert np.isneginf(got[c][r]), (name, c)
        assert got["raw"][r] == 0.0 and got["base2"][r] == 0.0
    assert len(got["smooth"]) == 1 and np.isneginf(got["prob_obj"][0]) and np.isneginf(got["normit_obj"][0]) and np.isneginf(got["gombit_obj"][0])


def test_table_with_65_rows_and_more_than_one_workgroup():
    for R in (65, 600):
        rng = np.random.default_rng(R)
        img = rng.integers(1, 5000, R)
        inst = img + rng.integers(0, 20000, R)
        img[0] = inst[0] = 1
        img[R - 1] = 5000
        check_table(device_table(img, inst, 5000), idf_oracle.table_from_frequencies(img, inst, 5000), f"R={R}")


# ----------------------------------------------------------------------------------------------------------------- end to end
def synthetic_dataset():
    """70 images (ids shuffled, three without annotations), category ids 1..65 of which 13 and 40 never occur, one annotation of an image that
    is not listed."""
    rng = np.random.default_rng(70)
    image_ids = (rng.permutation(70) * 3 + 11).tolist()
    cats = [{"id": k, "name": f"cat {k}"} for k in range(1, 66)]
    anns = []
    for i in image_ids[:-3]:
        for c in rng.choice([k for k in range(1, 66) if k not in (13, 40)], int(rng.integers(1, 30))).tolist():
            anns.append({"id": len(anns) + 1, "image_id": i, "category_id": c, "bbox": [1, 2, 3, 4]})
    anns += [{"id": len(anns) + 1, "image_id": image_ids[0], "category_id": 65, "bbox": [1, 2, 3, 4]},
             {"id": len(anns) + 2, "image_id": 5, "category_id": 13, "bbox": [1, 2, 3, 4]}]
    return {"images": [{"id": i} for i in image_ids], "categories": cats, "annotations": anns}


@pytest.fixture(scope="module")
def synthetic(tmp_path_factory):
    d = synthetic_dataset()
    root = tmp_path_factory.mktemp("idf")
    ann = root / "train.json"
    ann.write_text(json.dumps(d))
    df, ids = idf_oracle.dataset_table(d, "coco")
    csvp = root / "oracle_idf.csv"
    df.to_csv(csvp, index=False)
    return d, str(ann), df, ids, str(csvp), root


def test_idf_table_matches_the_oracle_end_to_end(synthetic):
    from object_detectors_amd import dataset_stats
    d, ann, df, ids, _csvp, _root = synthetic
    for source in (d, ann):
        t = dataset_stats.idf_table(source, "coco", device=DEV)
        assert t["category_ids"].tolist() == ids.tolist() and 13 not in ids and 40 not in ids and len(ids) == 63 and t["n_images"] == 70
        assert t["img_freq"].tolist() == df["img_freq"].tolist() and t["instance_freq"].tolist() == df["instance_freq"].tolist()
        check_table({c: t[c].cpu().numpy() for c in idf_oracle.COLUMNS14}, df, "end to end")
        assert t["names"] == [f"cat {k}" for k in ids.tolist()]
    t2 = dataset_stats.idf_table(dataset_stats.dataset_arrays(d, "coco"), device=DEV)
    assert all(torch.equal(t[c], t2[c]) for c in idf_oracle.COLUMNS14)


def test_idftransformer_builds_from_the_annotation_file(synthetic, monkeypatch):
    from object_detectors_amd.yolo.utilities.custom import IDFTransformer
    _d, ann, df, _ids, csvp, root = synthetic
    monkeypatch.delenv("owd", raising=False)
    want = IDFTransformer(csv_path=csvp, device="cpu")
    got = IDFTransformer(annfile=ann, dset_name="coco", device="cpu")
    assert got.num_classes == want.num_classes == 63 and set(got.idf_weights) == set(want.idf_weights) == set(df.columns)
    for k, w in want.idf_weights.items():
        g = got.idf_weights[k]
        assert g.dtype == torch.float32 and g.device.type == "cpu"
        assert idf_oracle.float32_equal_or_neighbour(g.numpy(), w.numpy()).all(), k
    assert torch.equal(got.idf_weights["img_freq"], want.idf_weights["img_freq"])
    # with $owd set the annotation file is relative to it and the table is cached as <owd>/<dset>_files/idf.csv, which the next call reads
    monkeypatch.setenv("owd", str(root))
    built = IDFTransformer(annfile="train.json", dset_name="coco", device="cpu")
    cached = os.path.join(str(root), "coco_files", "idf.csv")
    assert os.path.exists(cached)
    again = IDFTransformer(annfile="does_not_exist.json", dset_name="coco", device="cpu")
    assert set(again.idf_weights) == set(built.idf_weights) and all(torch.equal(again.idf_weights[k], built.idf_weights[k]) for k in built.idf_weights)


def test_yoloforw_builds_from_the_annotation_file_alone(synthetic, monkeypatch):
    from object_detectors_amd.yolo.nets.yolo_forw import YOLOForw
    _d, ann, df, _ids, _csvp, _root = synthetic
    monkeypatch.delenv("owd", raising=False)
    anchors = [[(116, 90), (156, 198), (373, 326)], [(30, 61), (62, 45), (59, 119)], [(10, 13), (16, 30), (33, 23)]]
    cfg = {"yolo": {"classes": 63, "img_size": 128, "tfidf": [1, 1]}, "dataset": {"anchors": anchors, "train_annotations": ann, "dset_name": "coco"}}
    m = YOLOForw(cfg).to(DEV)
    for row in (m.class_weights, m.idf_logits):
        assert idf_oracle.float32_equal_or_neighbour(row.cpu().numpy(), df["smooth"].to_numpy()).all()


def test_make_idf_writes_what_the_consumers_load(synthetic, tmp_path):
    """tools/make_idf.py (its main(), in this process; --help in a process of its own is in test_idf_host.py)."""
    import importlib.util
    import pandas as pd
    from object_detectors_amd.yolo.utilities.custom import IDFTransformer
    _d, ann, df, ids, _csvp, _root = synthetic
    spec = importlib.util.spec_from_file_location("make_idf", os.path.join(ROOT, "tools", "make_idf.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = str(tmp_path / "idf.csv")
    tool.main(["--ann", ann, "--dset", "coco", "--out", out])
    idf = IDFTransformer(csv_path=out, device="cpu")
    assert idf.num_classes == 63 and idf.idf_weights["instance_freq"].tolist() == [float(v) for v in df["instance_freq"]]
    out = str(tmp_path / "idf_66.csv")
    tool.main(["--ann", ann, "--dset", "coco", "--out", out, "--layout", "labels", "--num-classes", "66"])
    lab = pd.read_csv(out)                                   # detection/train.py:104-107
    values = torch.tensor(lab["smooth"], dtype=torch.float).unsqueeze(0)
    assert tuple(values.shape) == (1, 66) and float(values[0, 0]) == 1.0 and float(values[0, 13]) == 1.0 and float(values[0, 40]) == 1.0
    assert idf_oracle.float32_equal_or_neighbour(values[0, ids.tolist()].numpy(), df["smooth"].to_numpy()).all()


# ------------------------------------------------------------------------------------------- the recorded table at full size
def test_recorded_coco_table_at_full_size(recorded):
    """An index pair with exactly the recorded img_freq and instance_freq of COCO train2017: per category img_freq[c] distinct images out of
    118 287, one instance each and the rest spread over them; shuffled.  860 001 annotations."""
    from object_detectors_amd import dataset_stats
    rng = np.random.default_rng(2017)
    img_freq, inst_freq = recorded["img_freq"].astype(np.int64), recorded["instance_freq"].astype(np.int64)
    ids = np.array([k for k in range(1, 91) if k not in (12, 26, 29, 30, 45, 66, 68, 69, 71, 83)])
    ims, cats = [], []
    for c, (nf, ni) in enumerate(zip(img_freq, inst_freq)):
        chosen = rng.choice(COCO_IMAGES, int(nf), replace=False)
        ims += [chosen, chosen[rng.integers(0, nf, int(ni - nf))]]
        cats.append(np.full(int(ni), ids[c]))
    im, cat = np.concatenate(ims), np.concatenate(cats)
    perm = rng.permutation(len(im))
    im, cat = im[perm].astype(np.int32), cat[perm].astype(np.int32)
    assert len(im) == 860001
    inst, img = dataset_stats.category_frequencies(T(im), T(cat), COCO_IMAGES, 91)
    assert inst[ids].tolist() == inst_freq.tolist() and img[ids].tolist() == img_freq.tolist()
    assert int(inst.sum()) == 860001 and int(img.sum()) == int(img_freq.sum())
    t = dataset_stats.idf_table({"image_index": im, "category_index": cat, "n_images": COCO_IMAGES, "n_categories": 91}, device=DEV)
    assert t["category_ids"].tolist() == ids.tolist() and t["names"] is None
    check_table({c: t[c].cpu().numpy() for c in idf_oracle.COLUMNS14}, recorded, "full size")


# ------------------------------------------------------------------------------------------------------------------ RetinaNet
def test_retinanet_mini_batch_tfidf():
    """retinanet.py:125-133: with tfidf['mini_batch'] the training losses are those of the batch's own row (minibatch_tfidf with tfidf_norm),
    whatever `values` the constructor got; inference keeps the constructor's values.  The engine shapes of test_gpu_retina_engine.py.
    Model b is given that row as `values`, so both models run the same kernels on the same operands; the losses are float32 sums that may
    be added in another order from launch to launch, hence a relative 1e-6 (8 float32 steps) and not torch.equal."""
    from oracle import detrand
    from oracle import retina_oracle as ro
    from object_detectors_amd.tvision.retinanet import retinanet_resnet50_fpn
    from object_detectors_amd.tvision.roi_heads import minibatch_tfidf
    dev = torch.device(DEV)
    sd = ro.det_state(7000)
    x = torch.from_numpy(detrand.uniform(4242, (2, 3, 128, 128), 0.0, 1.0)).to(dev)
    targets = [{"boxes": torch.tensor([[10.0, 12.0, 70.0, 90.0], [40.0, 30.0, 100.0, 120.0]], device=dev), "labels": torch.tensor([5, 17], device=dev)},
               {"boxes": torch.tensor([[20.0, 8.0, 90.0, 60.0]], device=dev), "labels": torch.tensor([5], device=dev)}]
    values = torch.linspace(0.5, 1.5, 91, device=dev).reshape(1, -1)
    row = minibatch_tfidf(targets, 91, 2).float().reshape(1, -1)
    assert float(row[0, 5]) < float(row[0, 17]) < float(row[0, 0])            # in both images, in one, in none
    a = retinanet_resnet50_fpn(num_classes=91, device=dev, tfidf={"values": values, "num_classes": 91, "mini_batch": True, "tfidf_norm": 2})
    b = retinanet_resnet50_fpn(num_classes=91, device=dev, tfidf={"values": row, "num_classes": 91, "mini_batch": False, "tfidf_norm": 2})
    a.load_state_dict(sd)
    b.load_state_dict(sd)
    a.eval()
    before = a(x)
    a.train(), b.train()
    la, lb = a(x, targets), b(x, targets)
    torch.cuda.synchronize()
    for k in ("classification", "bbox_regression"):
        assert bool(torch.isfinite(la[k])) and float(la[k]) > 0
        torch.testing.assert_close(la[k], lb[k], rtol=1e-6, atol=0)
    assert torch.equal(a.tfidf, row) and torch.equal(a.tfidf_post, values) and torch.equal(b.tfidf, row)
    a.eval()
    after = a(x)                                                              # the batch's row did not reach inference
    assert sum(int(d["scores"].numel()) for d in before) > 0
    for d0, d1 in zip(before, after):
        for k in ("boxes", "scores", "labels"):
            assert torch.equal(d0[k], d1[k]), k
    b.eval()
    other = b(x)                                                              # and another row does change the detections
    assert any(d0["scores"].shape != d2["scores"].shape or not torch.equal(d0["scores"], d2["scores"]) for d0, d2 in zip(before, other))
