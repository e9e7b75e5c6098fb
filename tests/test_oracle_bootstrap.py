"""Bootstrap replicates on the CPU: the two restatements of tests/bootstrap_oracle.py against each other, hand-checked numbers, the host
statistics of object_detectors_amd/compare.py and the refusals that need no GPU."""
import numpy as np
import pytest
import torch

from tests import bootstrap_oracle as bo
from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo

EPS = np.spacing(1)                      # 2^-52
ALMOST_ONE = 1 / (1 + EPS)               # accumulate()'s precision of one true positive and nothing else: 1 - 2^-52, not 1


# ---------------------------------------------------------------------------------------------------------------- seeded sets
def _box(rng):
    side = [6.0, 20.0, 50.0, 120.0][rng.randint(0, 4)]              # areas in all of small / medium / large
    x, y = rng.randint(0, 40, 2).astype(np.float64)
    return [float(x), float(y), side + float(rng.randint(0, 6)), side + float(rng.randint(0, 6))]


def _near(rng, box):
    x, y, w, h = box
    return [x + float(rng.randint(-2, 3)), y + float(rng.randint(-2, 3)), max(w + float(rng.randint(-3, 4)), 1.0), max(h + float(rng.randint(-3, 4)), 1.0)]


def _group_scores(rng, n, grid):
    """n scores without a tie INSIDE the group; on the grid of 1/20 they tie across images."""
    if grid:
        return [float(s) / 20 for s in rng.permutation(np.arange(1, 21))[:n]]
    return [float(s) for s in rng.rand(n)]


def make_coco_set(seed, grid):
    """9 images, 3 categories, crowds, ground truths in every area range; no equal scores inside a group."""
    rng = np.random.RandomState(1000 + seed)
    anns, results = [], []
    for img in range(1, 10):
        for cat in (1, 2, 3):
            if rng.rand() < 0.25:
                continue
            boxes = [_box(rng) for _ in range(rng.randint(0, 4))]
            dets = [_near(rng, b) for b in boxes if rng.rand() < 0.8] + [_box(rng) for _ in range(rng.randint(0, 3))]
            for b in boxes:
                anns.append({"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": b, "area": b[2] * b[3], "iscrowd": int(rng.rand() < 0.2)})
            for b, s in zip(dets, _group_scores(rng, len(dets), grid)):
                results.append({"image_id": img, "category_id": cat, "bbox": b, "score": s})
    return {"images": [{"id": i} for i in range(1, 10)], "categories": [{"id": c} for c in (1, 2, 3)], "annotations": anns}, results


def make_lvis_set(seed):
    """6 images, 4 categories (r, r, c, f), negative and not-exhaustive lists, ignore flags; scores on the grid, no tie inside a group."""
    rng = np.random.RandomState(2000 + seed)
    cats = [(1, "r"), (2, "r"), (3, "c"), (4, "f")]
    anns, results, images = [], [], []
    for img in range(1, 7):
        positive = [c for c, _f in cats if rng.rand() < 0.6]
        negative = [c for c, _f in cats if c not in positive and rng.rand() < 0.6]
        images.append({"id": img, "neg_category_ids": negative, "not_exhaustive_category_ids": [c for c in positive if rng.rand() < 0.3]})
        for cat in positive:
            boxes = [_box(rng) for _ in range(rng.randint(1, 4))]
            for b in boxes:
                a = {"id": len(anns) + 1, "image_id": img, "category_id": cat, "bbox": b, "area": b[2] * b[3]}
                if rng.rand() < 0.2:
                    a["ignore"] = 1
                anns.append(a)
            dets = [_near(rng, b) for b in boxes if rng.rand() < 0.8] + [_box(rng) for _ in range(rng.randint(0, 2))]
            for b, s in zip(dets, _group_scores(rng, len(dets), True)):
                results.append({"image_id": img, "category_id": cat, "bbox": b, "score": s})
        for cat in negative:
            for s in _group_scores(rng, rng.randint(0, 3), True):
                results.append({"image_id": img, "category_id": cat, "bbox": _box(rng), "score": s})
    return {"images": images, "categories": [{"id": c, "frequency": f} for c, f in cats], "annotations": anns}, results


def _rows(rng, n, multinomial=3):
    return np.concatenate([rng.multinomial(n, [1 / n] * n, size=multinomial), np.ones((1, n), np.int64)]).astype(np.int64)


def _no_tie_inside_a_group(ev):
    return all(len(set(g["scores"].tolist())) == len(g["scores"]) for g in ev["groups"].values())


@pytest.mark.parametrize("seed", range(24))
def test_closed_form_is_the_replicated_data_set_coco(seed):
    """Sets 12..23 have scores on a grid: ties across images (the stable order over the copies decides), none inside a group."""
    grid = seed >= 12
    dataset, results = make_coco_set(seed, grid)
    ev = co.evaluate(dataset, results)
    assert _no_tie_inside_a_group(ev)
    if grid:
        scores = np.concatenate([g["scores"] for g in ev["groups"].values()])
        assert len(set(scores.tolist())) < len(scores)
    W = _rows(np.random.RandomState(seed), 9)
    got = bo.weighted(ev, W)
    for b, w in enumerate(W):
        precision, recall = bo.replicated(ev, w)
        assert np.array_equal(got["precision"][b], precision) and np.array_equal(got["recall"][b], recall), (seed, b)
    precision, recall, _scores = co.accumulate(ev)                          # the all-ones row is the plain evaluation
    assert np.array_equal(got["precision"][-1], precision) and np.array_equal(got["stats"][-1], co.summarize(precision, recall))
    assert (got["recall"] == -1).any() and (got["recall"] > 0).any()


@pytest.mark.parametrize("seed", range(8))
def test_closed_form_is_the_replicated_data_set_lvis(seed):
    dataset, results = make_lvis_set(seed)
    ev = lo.evaluate(dataset, results)
    assert _no_tie_inside_a_group(ev)
    W = _rows(np.random.RandomState(seed), 6, multinomial=2)
    got = bo.weighted(ev, W, "lvis")
    assert got["precision"].shape == (3, 10, 101, 4, 4, 1) and got["stats"].shape == (3, 13)
    for b, w in enumerate(W):
        precision, recall = bo.replicated(ev, w, "lvis")
        assert np.array_equal(got["precision"][b], precision) and np.array_equal(got["recall"][b], recall), (seed, b)
    _ev, precision, recall, res, _text = lo.run(dataset, results)
    assert np.array_equal(got["precision"][-1, ..., 0], precision) and np.array_equal(got["stats"][-1], np.asarray(list(res.values())))


# ---------------------------------------------------------------------------------------------------------------- on paper
HIT = [0., 0., 10., 10.]                 # every ground truth is this box (area 100: small), every hit has IoU 1, every miss IoU 0
MISS = [50., 50., 5., 5.]


def _paper_set(dets):
    """3 images with one ground truth each, one category; dets = [(image, box, score)]."""
    anns = [{"id": i, "image_id": i, "category_id": 1, "bbox": HIT, "area": 100., "iscrowd": 0} for i in (1, 2, 3)]
    results = [{"image_id": i, "category_id": 1, "bbox": b, "score": s} for i, b, s in dets]
    return co.evaluate({"images": [{"id": i} for i in (1, 2, 3)], "categories": [{"id": 1}], "annotations": anns}, results)


def test_hand_case():
    """Weights [2, 0, 1].  In score order: image 2 hits at .95 (weight 0: not in the replicate), image 1 hits at .9 (twice), image 1 misses at
    .7 (twice), image 3 hits at .6 (once).  npig = 2 + 0 + 1 = 3.
        maxDets 10 / 100:  tp 2 2 3, fp 0 2 2 -> rc 2/3 2/3 1, pr 2/(2 + 2^-52) = 1 (2 + 2^-52 rounds to 2), 2/4, 3/5 -> envelope 1, .6, .6.
                           The 67 thresholds 0 .. 0.66 are reached by the first slot (1), the 34 thresholds 0.67 .. 1 by the third (.6):
                           ap_sum = 34 x .6 added first, then 67 x 1; AP = that / 101 = 0.86534...; recall 1.
        maxDets 1:         the miss is second in its group and leaves: tp 2 3, fp 0 0 -> pr 1, 1 -> ap_sum 101, recall 1.
    The ground truths are small: `all` and `small` agree, `medium` and `large` have none (-1).  Hits are exact, so all ten IoU thresholds agree."""
    ev = _paper_set([(1, HIT, .9), (2, HIT, .95), (1, MISS, .7), (3, HIT, .6)])
    w = [2, 0, 1]
    got = bo.weighted(ev, w)
    want = 0.0
    for _ in range(34):
        want += 3 / 5
    for _ in range(67):
        want += 1.0
    assert abs(want / 101 - 0.86534) < 1e-5
    for a in (0, 1):
        assert (got["ap_sum"][0, :, 0, a, 1:] == want).all() and (got["ap_sum"][0, :, 0, a, 0] == 101.0).all()
        assert (got["recall"][0, :, 0, a, :] == 1.0).all()
        assert (got["precision"][0, :, :67, 0, a, 2] == 1.0).all() and (got["precision"][0, :, 67:, 0, a, 2] == 3 / 5).all()
    assert (got["ap_sum"][0, :, 0, 2:] == -1).all() and (got["recall"][0, :, 0, 2:] == -1).all() and (got["precision"][0, :, :, 0, 2:] == -1).all()
    stats = got["stats"][0]
    assert stats[0] == np.mean(got["precision"][0, :, :, 0, 0, 2]) and abs(stats[0] - want / 101) < 1e-12 and stats[4] == -1 and stats[8] == 1.0
    precision, recall = bo.replicated(ev, w)
    assert np.array_equal(got["precision"][0], precision) and np.array_equal(got["recall"][0], recall)


def test_a_tie_inside_a_group_with_different_flags_pins_the_closed_form():
    """Image 1, weight 2, holds a hit and a miss with EQUAL scores, the hit first.  The closed form keeps each detection's copies adjacent:
    hit hit miss miss -> tp 2 2, fp 0 2, npig 2, rc 1 1: every threshold is reached by the first slot, precision 2/(2 + 2^-52) = 1.  The
    replicated data set interleaves them: hit miss hit miss -> rc .5 .5 1 1, pr 1/(1 + 2^-52), 1/2, 2/3, 2/4 -> the thresholds above .5 get
    2/3.  The closed form is the definition."""
    ev = _paper_set([(1, HIT, .5), (1, MISS, .5)])
    w = [2, 0, 0]
    got = bo.weighted(ev, w)
    assert (got["precision"][0, :, :, 0, 0, 2] == 1.0).all() and (got["ap_sum"][0, :, 0, 0, 2] == 101.0).all()
    precision, _recall = bo.replicated(ev, w)
    assert (precision[:, :51, 0, 0, 2] == ALMOST_ONE).all() and (precision[:, 51:, 0, 0, 2] == 2 / 3).all()
    # without the tie the two agree
    ev = _paper_set([(1, HIT, .5), (1, MISS, .4)])
    assert np.array_equal(bo.weighted(ev, w)["precision"][0], bo.replicated(ev, w)[0])


def test_all_twos_against_all_ones():
    """Doubling every weight doubles tp, fp and npig, and every quotient is that of the unit weights - except the one place where
    accumulate()'s 2^-52 is not absorbed: a lone true positive has pr = 1/(1 + 2^-52) = 1 - 2^-52, its two copies end at 2/(2 + 2^-52) =
    2/2 = 1 (so does the literally replicated data set: its second copy has tp 2, fp 0).  From tp + fp = 2 on, x + 2^-52 rounds to x and
    the quotients of 2tp, 2fp are those of tp, fp.  So: recall cells equal, the -1 pattern equal, and the precision of all twos is the
    precision of all ones with 1 - 2^-52 replaced by 1, bit for bit.  (The shorter statement "all weights 2 give the cells of all weights
    1 exactly" holds in every cell without such a value and in no other: 34 and 49 of the 360 cells of the two sets of
    tests/test_gpu_cocoeval.py differ, by at most 1.5e-14.)"""
    differing = 0
    for seed in (0, 5, 13, 20):
        dataset, results = make_coco_set(seed, seed >= 12)
        ev = co.evaluate(dataset, results)
        got = bo.weighted(ev, np.stack([np.ones(9, np.int64), 2 * np.ones(9, np.int64)]))
        assert np.array_equal(got["recall"][0], got["recall"][1])
        ones = got["precision"][0]
        assert np.array_equal(got["precision"][1], np.where(ones == ALMOST_ONE, 1.0, ones))
        assert np.array_equal(got["precision"][1], bo.replicated(ev, 2 * np.ones(9, np.int64))[0])
        differing += int((got["ap_sum"][0] != got["ap_sum"][1]).sum())
        assert np.abs(got["ap_sum"][0] - got["ap_sum"][1]).max() <= 101 * EPS
    assert differing > 0


# ---------------------------------------------------------------------------------------------------------------- compare.py
def test_bootstrap_weights():
    from object_detectors_amd.compare import bootstrap_weights
    w = bootstrap_weights(37, 50, 7)
    assert w.dtype == np.int32 and w.shape == (50, 37) and (w.sum(1) == 37).all() and (w >= 0).all()
    assert np.array_equal(w, bootstrap_weights(37, 50, 7)) and not np.array_equal(w, bootstrap_weights(37, 50, 8))
    assert np.array_equal(w, np.random.default_rng(7).multinomial(37, [1 / 37] * 37, size=50))
    assert bootstrap_weights(3, 0, 0).shape == (0, 3)
    with pytest.raises(ValueError):
        bootstrap_weights(0, 5, 0)


def test_interval():
    from object_detectors_amd.compare import interval
    v = np.asarray([0.1, 0.2, -1.0, 0.3, 0.4, 0.5, -1.0])
    got = interval(v, 0.9)
    kept = np.asarray([0.1, 0.2, 0.3, 0.4, 0.5])
    assert got["n_used"] == 5 and got["mean"] == kept.mean()
    assert [got["lo"], got["hi"]] == list(np.quantile(kept, [(1 - 0.9) / 2, 1 - (1 - 0.9) / 2]))
    assert abs(got["lo"] - 0.12) < 1e-15 and abs(got["hi"] - 0.48) < 1e-15          # linear interpolation between the order statistics
    assert abs(interval(kept)["lo"] - 0.11) < 1e-15 and abs(interval(kept)["hi"] - 0.49) < 1e-15
    none = interval([-1.0, -1.0])
    assert none["n_used"] == 0 and all(np.isnan(none[k]) for k in ("mean", "lo", "hi"))
    with pytest.raises(ValueError):
        interval(v, 1.0)


def test_paired_bootstrap():
    from object_detectors_amd.compare import paired_bootstrap
    a = np.asarray([[0.50, 0.2, -1.0], [0.52, 0.2, -1.0], [0.48, -1.0, -1.0], [0.51, 0.2, 0.3]])
    b = np.asarray([[0.53, 0.2, 0.5], [0.54, 0.1, 0.5], [0.52, 0.3, 0.5], [-1.0, 0.3, -1.0]])
    got = paired_bootstrap(a, b, 0.9)
    # column 0: the last pair is dropped, d = .03 .02 .04, all > 0: p = min(1, 2 * min((0 + 1) / 4, (3 + 1) / 4)) = .5
    d = np.asarray([0.53 - 0.50, 0.54 - 0.52, 0.52 - 0.48])
    assert got["n_used"][0] == 3 and got["delta_mean"][0] == d.mean() and got["p"][0] == 0.5
    assert [got["lo"][0], got["hi"][0]] == list(np.quantile(d, [(1 - 0.9) / 2, 1 - (1 - 0.9) / 2]))
    # column 1: the third pair is dropped, d = 0 -.1 .1: #(d <= 0) = 2, #(d >= 0) = 2 -> 2 * 3/4 -> 1
    assert got["n_used"][1] == 3 and got["p"][1] == 1.0 and abs(got["delta_mean"][1]) < 1e-16
    # column 2: no pair is left
    assert got["n_used"][2] == 0 and got["p"][2] == 1.0 and all(np.isnan(got[k][2]) for k in ("delta_mean", "lo", "hi"))
    one = paired_bootstrap(a[:, 0], b[:, 0], 0.9)
    assert one["p"].shape == (1,) and one["p"][0] == 0.5
    # 99 replicates, b always better: p = 2 * 1 / 100
    assert paired_bootstrap(np.zeros(99), np.full(99, 0.01))["p"][0] == 0.02
    with pytest.raises(ValueError):
        paired_bootstrap(a, b[:3])


# ---------------------------------------------------------------------------------------------------------------- refusals without a GPU
def test_ops_refuse_cpu_tensors():
    from object_detectors_amd import ops
    i64, i32 = (lambda *s: torch.zeros(s, dtype=torch.int64)), (lambda *s: torch.zeros(s, dtype=torch.int32))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.coco_bootstrap(i64(2), i64(2), i64(3), i32(3), torch.zeros((4, 10, 3), dtype=torch.int32), torch.zeros((4, 10, 3), dtype=torch.uint8),
                           torch.zeros((4, 2), dtype=torch.uint8), [1, 10, 100], torch.linspace(0, 1, 101, dtype=torch.float64), i32(3), i32(2),
                           i32(5, 8))


def test_entry_refuses_bad_arguments_before_any_launch():
    """mi355det_coco_bootstrap validates on the host: every refusal below returns MI355DET_EINVAL without a launch."""
    import ctypes as C
    from object_detectors_amd._lib import lib
    L = lib()
    buf = (C.c_int64 * 4)()
    p = C.cast(buf, C.c_void_p)                           # never dereferenced on the host
    md = (C.c_int32 * 9)(*range(1, 10))

    def call(**change):
        a = dict(num_cats=1, cdo=p, cgo=p, num_dt=1, num_gt=1, order=p, rank=p, match=p, dt_ignore=p, gt_ignore=p, num_thrs=10, num_areas=4, md=md,
                 num_md=3, rec=p, num_recs=101, dt_image=p, gt_image=p, weights=p, num_images=5, num_replicates=8, ap_sum=p, recall=p, stream=None)
        assert set(change) <= set(a)
        a.update(change)
        return L.mi355det_coco_bootstrap(*a.values())
    for name in ("cdo", "cgo", "order", "rank", "match", "dt_ignore", "gt_ignore", "md", "rec", "dt_image", "gt_image", "weights", "ap_sum", "recall"):
        assert call(**{name: None}) == -1, name
    for name in ("num_cats", "num_thrs", "num_areas", "num_md", "num_recs", "num_images", "num_replicates"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1, name
    assert call(num_dt=-1) == -1 and call(num_gt=-1) == -1
    assert call(num_recs=4097) == -1 and call(num_md=9) == -1


def _evaluators():
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISEval
    return [COCOEval(make_coco_set(0, False)[0]), LVISEval(make_lvis_set(0)[0])]


def test_bootstrap_needs_evaluate_first():
    for e, n in zip(_evaluators(), (9, 6)):
        with pytest.raises(RuntimeError, match="evaluate"):
            e.bootstrap(np.ones((2, n), np.int32))


def test_bootstrap_refuses_bad_weights():
    for e, n in zip(_evaluators(), (9, 6)):
        for bad in (np.ones((2, n + 1), np.int32), np.ones(n, np.int32), np.ones((2, n), np.float64), torch.ones((2, n), dtype=torch.float32),
                    -np.ones((2, n), np.int64), torch.tensor([[1] * (n - 1) + [-1]]), np.ones((2, n), bool)):
            with pytest.raises(ValueError, match="weights"):
                e.bootstrap(bad)
