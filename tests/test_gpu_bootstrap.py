"""Bootstrap replicates on the device (object_detectors_amd/csrc/bootstrap_kernels.hip, COCOEval.bootstrap, LVISEval.bootstrap) against the two
restatements of tests/bootstrap_oracle.py.  The cells (ap_sum, recall) are float64 results of the same correctly rounded operations in the
same order on both sides and are compared with ==.  The statistics are means over the cells, summed on the device in another order than the
restatement's np.mean: each is a sum of n < 10^4 terms in [0, 1] (the precision values regrouped), so two orders differ by at most
n u = 10^4 x 2^-53 = 1.1e-12; the bound used is ten times that, 1e-11."""
import io

import numpy as np
import pytest
import torch

from tests import bootstrap_oracle as bo
from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo
from tests.test_gpu_cocoeval import _with_segmentation, make_bbox_set, make_segm_set
from tests.test_gpu_lviseval import make_set as make_lvis_set

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
TOL = 1e-11
ALMOST_ONE = 1 / (1 + np.spacing(1))


def _coco(dataset, results, iou_type="bbox"):
    from object_detectors_amd.cocoeval import COCOEval
    e = COCOEval(dataset, iou_type)
    e.add_results(results)
    return e.evaluate()


def _check(e, ev, W, kind="coco", literal=()):
    """bootstrap() of every row of W: cells == the closed form, == the literally replicated data set for the rows in `literal`; statistics
    within TOL.  -> (stats, ap_sum, recall, the closed form)."""
    W = np.asarray(W)
    stats, (ap, rc) = e.bootstrap(W, return_cells=True)
    want = bo.weighted(ev, W, kind)
    assert ap.dtype == torch.float64 and ap.is_cuda and tuple(ap.shape) == want["ap_sum"].shape == tuple(rc.shape)
    ap, rc = ap.cpu().numpy(), rc.cpu().numpy()
    assert np.array_equal(rc, want["recall"]) and np.array_equal(ap, want["ap_sum"])
    assert stats.dtype == np.float64 and stats.shape == want["stats"].shape
    assert np.array_equal(stats == -1, want["stats"] == -1) and np.abs(stats - want["stats"]).max() <= TOL
    for b in literal:
        precision, recall = bo.replicated(ev, W[b], kind)
        assert np.array_equal(rc[b], recall) and np.array_equal(ap[b], bo.ap_sum_of(precision, recall)), b
    return stats, ap, rc, want


@pytest.fixture(scope="module")
def bbox_sets():
    out = {}
    for grid in (True, False):
        dataset, results = make_bbox_set(grid, 5 if grid else 6)
        e = _coco(dataset, results).accumulate()
        e.summarize(file=io.StringIO())
        out[grid] = (e, co.evaluate(dataset, results))
    return out


@pytest.mark.parametrize("grid", [True, False])
def test_unit_weights_are_the_evaluation(bbox_sets, grid):
    e, _ev = bbox_sets[grid]
    precision, recall, before = e.precision.copy(), e.recall.copy(), e.stats.copy()
    stats, (ap, rc) = e.bootstrap(np.ones((1, len(e.img_ids)), np.int32), return_cells=True)
    assert tuple(ap.shape) == (1, 10, 3, 4, 3) and stats.shape == (1, 12)
    assert np.array_equal(rc[0].cpu().numpy(), recall)
    assert np.array_equal(ap[0].cpu().numpy(), bo.ap_sum_of(precision, recall))
    assert np.array_equal((ap[0] == -1).cpu().numpy(), recall == -1) and (recall == -1).any() and (recall > 0).any()
    assert np.abs(stats[0] - before).max() <= TOL and np.array_equal(stats[0] == -1, before == -1)
    assert np.array_equal(e.precision, precision) and np.array_equal(e.stats, before)               # untouched
    assert np.array_equal(e.bootstrap(torch.ones((1, len(e.img_ids)), dtype=torch.int64, device=DEV)), stats)       # a device tensor, another integer type


@pytest.mark.parametrize("grid", [True, False])
def test_mixed_rows(bbox_sets, grid):
    """Three resamples, no image at all, one image alone, every image twice, every image once.  The grid set has equal scores inside groups,
    where the literally replicated data set is another rule (tests/test_oracle_bootstrap.py); the other set is compared against it too."""
    e, ev = bbox_sets[grid]
    I = len(e.img_ids)
    one = np.zeros((1, I), np.int64)
    one[0, e.img_ids.index(17)] = 3
    W = np.concatenate([np.random.RandomState(3).multinomial(I, [1 / I] * I, size=3), np.zeros((1, I), np.int64), one, np.full((1, I), 2), np.ones((1, I), np.int64)])
    stats, ap, rc, want = _check(e, ev, W, literal=() if grid else range(len(W)))
    assert (ap[3] == -1).all() and (rc[3] == -1).all() and (stats[3] == -1).all()
    assert (ap[4] > 0).any() and (ap[4] == -1).sum() >= (ap[6] == -1).sum()                # image 17 alone
    # every image twice against every image once: tests/test_oracle_bootstrap.py::test_all_twos_against_all_ones
    assert np.array_equal(rc[5], rc[6])
    ones = want["precision"][6]
    assert np.array_equal(ap[5], bo.ap_sum_of(np.where(ones == ALMOST_ONE, 1.0, ones), rc[6]))
    assert np.abs(ap[5] - ap[6]).max() <= 101 * np.spacing(1)


def _edge_set(n):
    """tests/test_gpu_cocoeval.py::test_accumulate_chunk_edges: one category with one detection on each of n images (a second one on 32 of
    them for n = 130), so that the category's slots just miss, fill and exceed the 64 slots the wave loads at a time; n = 0: none."""
    rng = np.random.RandomState(n)
    images = list(range(1, max(n, 2) + 1))
    anns = [{"id": i, "image_id": i, "category_id": 1, "bbox": [0., 0., 10., 10.], "area": 100., "iscrowd": 0} for i in images]
    results = []
    for i in images[:n]:
        hit, miss = [0., 0., 10., float(rng.randint(4, 11))], [50., 50., 5., 5.]
        results.append({"image_id": i, "category_id": 1, "bbox": hit if rng.rand() < .7 else miss, "score": float(rng.randint(1, 11)) / 10})
    for i in images[:32] if n == 130 else []:
        results.append({"image_id": i, "category_id": 1, "bbox": [0., 0., 10., 10.], "score": 0.05})
    return {"images": [{"id": i} for i in images], "categories": [{"id": 1}], "annotations": anns}, results


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_slot_chunk_edges(n):
    dataset, results = _edge_set(n)
    assert len(results) == {0: 0, 1: 1, 63: 63, 64: 64, 65: 65, 130: 162}[n]
    e, ev = _coco(dataset, results), co.evaluate(dataset, results)
    I = len(e.img_ids)
    W = np.random.RandomState(n + 1).multinomial(I, [1 / I] * I, size=9)
    W[0] = 1
    W[1, :] = 0
    W[1, -1] = 2                                           # the last image alone
    _check(e, ev, W, literal=range(5))


# two categories, 6 images, 31 detections.  Category 1: image 1 holds the best-scored detection (a hit), image 2's best is a miss, image 3's
# best lies on a crowd (ignored); category 2 has ground truth in image 6 only and false positives elsewhere.
def _planted_set():
    rng = np.random.RandomState(77)
    hit, miss = [0., 0., 10., 10.], [50., 50., 5., 5.]
    anns, results = [], []

    def gt(img, cat, box, crowd=0):
        anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": box, "area": box[2] * box[3], "iscrowd": crowd})

    def dt(img, cat, box, score):
        results.append({"image_id": img, "category_id": cat, "bbox": box, "score": score})
    for img in range(1, 6):
        gt(img, 1, hit)
    gt(3, 1, [100., 100., 20., 20.], crowd=1)
    dt(1, 1, hit, .99)
    dt(2, 1, miss, .98)
    dt(3, 1, [100., 100., 20., 20.], .97)
    for img in range(1, 6):
        for s in rng.permutation(np.arange(1, 19))[:4]:
            dt(img, 1, [0., 0., 10., float(rng.randint(4, 11))] if rng.rand() < .5 else miss, float(s) / 20)
    gt(6, 2, hit)
    gt(6, 2, [200., 0., 40., 40.])
    for img, box, s in ((6, hit, .9), (6, [200., 0., 40., 30.], .5), (6, miss, .7), (1, miss, .8), (2, hit, .6), (4, miss, .3), (6, miss, .1), (5, miss, .65)):
        dt(img, 2, box, s)
    return {"images": [{"id": i} for i in range(1, 7)], "categories": [{"id": 1}, {"id": 2}], "annotations": anns}, results


@pytest.fixture(scope="module")
def planted():
    dataset, results = _planted_set()
    assert len(results) == 31
    ev = co.evaluate(dataset, results)
    g = ev["groups"]
    assert g[(0, 0)]["dt_match"][0, 0, 0] != 0 and not g[(0, 0)]["dt_ignore"][0, 0, 0]                  # image 1: a hit in front
    assert g[(0, 1)]["dt_match"][0, 0, 0] == 0 and not g[(0, 1)]["dt_ignore"][0, 0, 0]                  # image 2: a miss in front
    assert g[(0, 2)]["dt_ignore"][0, 0, 0] == 1                                                         # image 3: ignored in front
    return _coco(dataset, results), ev


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_replicate_chunk_edges(planted, B):
    """Replicates that just miss, fill and exceed the 64 lanes of a wave.  Rows 0..3 are planted: the best-scored detection has weight 0 and
    the first kept one is a false positive; then the first kept one is ignored; then category 2's only ground truths sit in an image of
    weight 0 (-1) while its detections elsewhere stay; then nothing but that image."""
    e, ev = planted
    rows = np.asarray([[0, 1, 1, 1, 1, 1], [0, 0, 2, 1, 1, 1], [1, 2, 1, 1, 1, 0], [0, 0, 0, 0, 0, 3]], np.int64)
    W = rows[:1] if B == 1 else np.concatenate([rows, np.random.RandomState(B).multinomial(6, [1 / 6] * 6, size=B - 4)])
    assert len(W) == B
    _stats, ap, _rc, _want = _check(e, ev, W, literal=range(min(B, 5)))
    if B > 1:
        assert (ap[2][:, 1] == -1).all() and (ap[2][:, 0, 0] > 0).any() and (ap[3][:, 0] == -1).all() and (ap[3][:, 1, 0] > 0).all()
        assert (W[4:, 0] == 0).any() and (W[4:, 5] == 0).any()


def test_budget_chunks_and_repeatability(bbox_sets):
    e, _ev = bbox_sets[False]
    I = len(e.img_ids)
    W = np.random.RandomState(9).multinomial(I, [1 / I] * I, size=70).astype(np.int32)
    per_replicate = 2 * 8 * 10 * 3 * 4 * 3
    whole, (ap, rc) = e.bootstrap(W, return_cells=True)
    again, (ap2, rc2) = e.bootstrap(W, return_cells=True)
    assert torch.equal(ap, ap2) and torch.equal(rc, rc2) and whole.tobytes() == again.tobytes()
    for budget in (1, per_replicate, 64 * per_replicate):               # one replicate per launch (twice), 64 per launch
        stats, (ap3, rc3) = e.bootstrap(W, return_cells=True, cell_budget_bytes=budget)
        assert torch.equal(ap, ap3) and torch.equal(rc, rc3) and stats.tobytes() == whole.tobytes()
    assert e.bootstrap(W[:0]).shape == (0, 12)


def test_lvis():
    from object_detectors_amd.lviseval import LVISEval
    dataset, results = make_lvis_set()
    ev, precision, recall, res, _text = lo.run(dataset, results)
    e = LVISEval(dataset, results).evaluate()
    I = len(e.img_ids)
    rare = sorted(e._cat_index[c["id"]] for c in dataset["categories"] if c["frequency"] == "r")
    assert e.freq_groups[0] == rare
    no_rare = np.ones(I, np.int64)
    for a in dataset["annotations"]:
        if a["category_id"] in e._cat_index and e._cat_index[a["category_id"]] in rare:
            no_rare[e._img_index[a["image_id"]]] = 0
    assert 0 < no_rare.sum() < I
    W = np.concatenate([np.random.RandomState(4).multinomial(I, [1 / I] * I, size=3), no_rare[None], np.ones((1, I), np.int64)])
    stats, ap, rc, want = _check(e, ev, W, "lvis")
    assert stats.shape == (5, 13) and ap.shape == (5, 10, 6, 4, 1)
    assert stats[3, 6] == -1 and (stats[4, 6:9] > 0).all()                                              # APr: no rare ground truth is left
    assert np.array_equal(rc[4][..., 0], recall) and np.array_equal(ap[4][..., 0], bo.ap_sum_of(precision[..., None], recall[..., None])[..., 0])
    assert np.abs(stats[4] - np.asarray(list(res.values()))).max() <= TOL
    assert e.precision is None and not e.results                                                        # evaluate() alone, nothing else set


def test_segm():
    dataset, results = make_segm_set(21)
    ev = co.evaluate(dataset, results, "segm")
    rows = [{k: v for k, v in r.items() if k != "mask"} for r in results]
    e = _coco(_with_segmentation(dataset, "string"), rows, "segm")
    I = len(e.img_ids)
    W = np.concatenate([np.random.RandomState(5).multinomial(I, [1 / I] * I, size=2), np.ones((1, I), np.int64)])
    stats, _ap, _rc, _want = _check(e, ev, W)
    assert stats[2, 0] > 0


def _tool():
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "compare_models.py")
    spec = importlib.util.spec_from_file_location("compare_models", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _files(tmp_path, dataset, a, b):
    import json
    paths = []
    for name, obj in (("gt", dataset), ("a", a), ("b", b)):
        paths.append(str(tmp_path / f"{name}.json"))
        with open(paths[-1], "w") as f:
            json.dump(obj, f)
    return ["--gt", paths[0], "--results", paths[1], paths[2]]


def test_compare_models_bootstrap_block(bbox_sets, tmp_path, capsys):
    """tools/compare_models.py --bootstrap: the output without the flag, byte for byte, then one block whose numbers are those of the API."""
    from object_detectors_amd import compare
    from object_detectors_amd.cocoeval import COCOEval
    dataset, results = make_bbox_set(False, 6)
    other = [dict(r, score=r["score"] * (0.5 if j % 3 == 0 else 1.0)) for j, r in enumerate(results)]
    args = _files(tmp_path, dataset, results, other)
    tool = _tool()
    tool.main(args)
    plain = capsys.readouterr().out
    tool.main(args + ["--bootstrap", "40", "--seed", "3"])
    out = capsys.readouterr().out
    assert out.startswith(plain) and "bootstrap" not in plain
    block = out[len(plain):].splitlines()
    assert block[0].startswith("== bootstrap: 40 resamples of 7 images, seed 3, 95% percentile intervals") and len(block) == 1 + 3 * 3
    w = compare.bootstrap_weights(7, 40, 3)
    ea, eb = bbox_sets[False][0], COCOEval(dataset)
    eb.add_results(other)
    a, b = ea.bootstrap(w), eb.evaluate().bootstrap(w)
    i, p = compare.interval(a[:, 1]), compare.paired_bootstrap(a, b)
    assert block[4].split()[0] == "AP50" and f"{i['mean']:8.4f} [{i['lo']:.4f}, {i['hi']:.4f}] ({i['n_used']} used)" in block[4]
    assert f"{p['delta_mean'][2]:+8.4f} [{p['lo'][2]:+.4f}, {p['hi'][2]:+.4f}] p={p['p'][2]:.4f}" in block[9] and "difference" in block[9]


def test_compare_models_bootstrap_block_lvis(tmp_path, capsys):
    dataset, results = make_lvis_set()
    other = [dict(r, score=r["score"] * (0.5 if j % 3 == 0 else 1.0)) for j, r in enumerate(results)]
    _tool().main(_files(tmp_path, dataset, results, other) + ["--bootstrap", "10", "--lvis"])
    out = capsys.readouterr().out
    block = out[out.index("== bootstrap"):].splitlines()
    assert "(LVIS rules)" in block[0] and len(block) == 1 + 6 * 3
    assert [line.split()[0] for line in block[1::3]] == ["AP", "AP50", "AP75", "APr", "APc", "APf"]


def test_refusals_and_stray_image_indices(bbox_sets):
    from object_detectors_amd import ops
    from object_detectors_amd.cocoeval import REC_THRS, category_order
    e, _ev = bbox_sets[False]
    I = len(e.img_ids)
    for bad in (torch.ones((2, I), dtype=torch.float64, device=DEV), -torch.ones((2, I), dtype=torch.int32, device=DEV),
                torch.ones((2, I + 1), dtype=torch.int32, device=DEV)):
        with pytest.raises(ValueError, match="weights"):
            e.bootstrap(bad)
    order = category_order(e.cat_dt_offsets, e.dt_score)
    rec = torch.from_numpy(REC_THRS).to(DEV)
    w = torch.from_numpy(np.random.RandomState(1).multinomial(I, [1 / I] * I, size=5).astype(np.int32)).to(DEV).t().contiguous()
    call = lambda max_dets=(1, 10, 100), rec=rec, dt_image=e.dt_image, gt_image=e.gt_image, w=w: ops.coco_bootstrap(
        e.cat_dt_offsets, e.cat_gt_offsets, order, e.dt_rank, e.dt_match, e.dt_ignore, e.gt_ignore, list(max_dets), rec, dt_image, gt_image, w)
    with pytest.raises(ValueError):
        call(max_dets=range(1, 10))
    with pytest.raises(ValueError):
        call(rec=torch.linspace(0, 1, 4097, dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError):
        call(w=w.to(torch.int64))
    with pytest.raises(ValueError):
        call(dt_image=e.dt_image[:-1])
    # an image index outside the table is weight 0 and reads nothing: the same bits as an extra image of weight 0
    stray_dt, stray_gt = e.dt_image.clone(), e.gt_image.clone()
    stray_dt[::3], stray_gt[::4] = I, I
    extra = torch.cat([w, torch.zeros((1, 5), dtype=torch.int32, device=DEV)]).contiguous()
    want = call(dt_image=stray_dt, gt_image=stray_gt, w=extra)
    stray_dt[::6], stray_gt[::8] = -1, 2 ** 31 - 1
    got = call(dt_image=stray_dt, gt_image=stray_gt)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and (got[0] != call()[0]).any()
