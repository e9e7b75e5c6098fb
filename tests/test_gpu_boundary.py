"""Boundary IoU on the device (csrc/boundary_kernels.hip, ops.rle_boundary, RLEBatch.boundary, ops.coco_boundary_iou, COCOEval and
LVISSegmEval with iou_type "boundary") against the literal form of the rule (tests/boundary_oracle.py).  Run lengths, areas and boxes are
integers and every IoU is one float64 quotient of two pixel counts taken once on both sides: every comparison is exact."""
import numpy as np
import pytest
import torch

from tests import boundary_oracle as bd
from tests import bootstrap_oracle as bo
from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo
from tests import lvissegm_oracle as so
from tests import rle_oracle as ro

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
MATCH = ("iou", "dt_match", "dt_ignore", "gt_match", "gt_ignore")


def _host(t):
    return t.cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def _ellipse(h, w, cy, cx, ry, rx):
    y, x = np.mgrid[0:h, 0:w]
    return ((((y - cy) / ry) ** 2 + ((x - cx) / rx) ** 2) <= 1).astype(np.uint8)


def _cases():
    """[(mask, d)]: every shape the kernel treats differently, at sizes that are no multiple of its 64-row words and 64 / 256-column steps."""
    out = []
    rng = np.random.default_rng(2)

    def add(m, d=None):
        m = np.ascontiguousarray(m, np.uint8)
        out.append((m, bd.dilation(*m.shape) if d is None else d))
    add(np.zeros((30, 40)))                                          # the empty mask
    add(np.ones((30, 40)))                                           # the full image: a frame of width d
    add(np.ones((4, 60)), 2)                                         # min(h, w) <= 2d: the whole mask
    add(np.ones((100, 150)))                                         # d = 4, two words per column
    for d in (1, 2, 4):
        m = np.zeros((70, 90))
        m[20:20 + 2 * d + 1, 30:30 + 2 * d + 1] = 1                  # the (2d+1)^2 square: a one-pixel hole
        add(m, d)
        m = np.zeros((70, 90))
        m[3:3 + 2 * d, 5:85] = 1                                     # a 2d x large bar: its own boundary
        add(m, d)
        m = np.zeros((90, 70))
        m[5:85, 60:60 + 2 * d] = 1
        add(m, d)
    for cy, cx in ((0, 30), (44, 30), (20, 0), (20, 59), (0, 0), (44, 59)):     # blobs on each border and in two corners
        add(_ellipse(45, 60, cy, cx, 12, 15))
    m = _ellipse(100, 150, 50, 70, 40, 60)
    m[50, 70] = 0                                                    # a big blob with a one-pixel hole
    add(m)
    m = np.zeros((45, 60))
    m[:, 3:12] = 1                                                   # full-height columns: one run across many columns
    m[:, 20:22] = 1
    m[10:, 30] = 1
    m[:30, 31] = 1
    add(m)
    m = _ellipse(45, 60, 5, 5, 9, 9)
    m[0, 0] = 1                                                      # the first count is 0
    add(m)
    m = _ellipse(45, 60, 40, 55, 9, 9)
    m[44, 59] = 1                                                    # ends in ones
    add(m)
    add(np.ones((45, 60)), 3)                                        # both at once, every column full
    for h in (31, 32, 33, 64, 65, 70):                               # around the 64-row word
        add(_ellipse(h, 50, h / 2, 25, h / 2 + 1, 20), 2)
        m = (rng.random((h, 37)) < 0.9)
        add(m, 1)
    for d in (1, 3):
        for w in (1, 2 * d, 2 * d + 1):                              # widths around the window
            add(np.ones((40, w)), d)
            m = np.ones((70, w))
            m[rng.integers(0, 70), rng.integers(0, w)] = 0
            add(m, d)
    add(_ellipse(45, 60, 22, 30, 18, 25), 5)                         # a dilation that is not the default one
    add(_ellipse(30, 300, 15, 150, 14, 148))                         # more than 256 columns, one word each (d = 6)
    m = _ellipse(480, 640, 250, 300, 200, 280)
    m[100:140, 200:260] = 0
    m[:, 630:] = 1
    add(m)                                                           # 480 x 640 at d = 16
    return out


@pytest.fixture(scope="module")
def batch():
    """The mixed-size batch as run lengths, and what the rule gives for each mask: computed once."""
    cases = _cases()
    assert cases[-1][1] == 16
    src = [ro.encode(m) for m, _d in cases]
    want = [bd.boundary(m, d) for m, d in cases]
    enc = [ro.encode(b) for b in want]
    return {"cases": cases, "counts": torch.from_numpy(np.concatenate(src).astype(np.int32)).to(DEV),
            "runs": np.concatenate([[0], np.cumsum([c.size for c in src])]).astype(np.int64),
            "sizes": np.asarray([m.shape for m, _d in cases], np.int32), "dil": np.asarray([d for _m, d in cases], np.int32),
            "boxes": np.asarray([ro.bbox(m) for m, _d in cases], np.int32), "want": want, "enc": enc,
            "want_counts": np.concatenate(enc), "want_runs": np.concatenate([[0], np.cumsum([c.size for c in enc])]),
            "want_area": np.asarray([int(b.sum()) for b in want], np.int64), "want_box": np.asarray([ro.bbox(b) for b in want], np.int32)}


def _check(got, b, order=None):
    counts, runs, area, box = got
    order = np.arange(len(b["enc"])) if order is None else order
    assert counts.dtype == torch.int32 and area.dtype == torch.int64 and box.dtype == torch.int32 and runs.dtype == np.int64
    enc = [b["enc"][j] for j in order]
    assert np.array_equal(runs, np.concatenate([[0], np.cumsum([c.size for c in enc])]))
    c = _host(counts)
    for n, j in enumerate(order):
        assert np.array_equal(c[runs[n]:runs[n + 1]], enc[n]), (n, b["cases"][j][0].shape, b["cases"][j][1])
    assert np.array_equal(_host(area), b["want_area"][order]) and np.array_equal(_host(box), b["want_box"][order])


def test_rle_boundary_against_the_rule(batch):
    """(a): counts, offsets, area and box of the whole mixed batch; the boxes as a host table and as a device tensor; an index."""
    from object_detectors_amd import ops
    b = batch
    assert any(w.sum() == 0 for w in b["want"]) and any(np.array_equal(w, m) and m.sum() for w, (m, _d) in zip(b["want"], b["cases"]))
    got = ops.rle_boundary(b["counts"], b["runs"], b["sizes"], b["dil"], b["boxes"])
    _check(got, b)
    _check(ops.rle_boundary(b["counts"], torch.from_numpy(b["runs"]).to(DEV), b["sizes"], torch.from_numpy(b["dil"]).to(DEV),
                            torch.from_numpy(b["boxes"]).to(DEV)), b)
    order = np.random.default_rng(0).permutation(len(b["cases"]))[:20]
    _check(ops.rle_boundary(b["counts"], b["runs"], b["sizes"][order], b["dil"][order], b["boxes"][order], index=order), b, order)
    # a box that holds the mask but is not tight gives the same boundary
    loose = b["boxes"].copy()
    loose[:, :2] = 0
    loose[:, 2], loose[:, 3] = b["sizes"][:, 1], b["sizes"][:, 0]
    _check(ops.rle_boundary(b["counts"], b["runs"], b["sizes"], b["dil"], loose), b)


def test_rle_batch_boundary(batch):
    """RLEBatch.boundary: the masks of one size, the default dilation of that size."""
    from object_detectors_amd import ops
    masks = [m for m, d in batch["cases"] if m.shape == (45, 60) and d == 2]
    assert len(masks) >= 8
    rb = ops.mask_rle_dense(torch.from_numpy(np.stack(masks).astype(np.float32)).to(DEV), 0.5).boundary()
    want = [bd.boundary(m, 2) for m in masks]
    assert rb.size == (45, 60) and len(rb) == len(masks)
    for n, w in enumerate(want):
        assert np.array_equal(rb.counts_of(n), ro.encode(w)), n
    assert np.array_equal(_host(rb.area), [int(w.sum()) for w in want]) and np.array_equal(_host(rb.bbox), [ro.bbox(w) for w in want])
    assert np.array_equal(rb.decode().numpy(), np.stack(want))
    other = ops.mask_rle_dense(torch.from_numpy(np.stack(masks).astype(np.float32)).to(DEV), 0.5).boundary(0.07)      # d = 5
    assert np.array_equal(other.decode().numpy(), np.stack([bd.boundary(m, 5) for m in masks]))


def test_chunks_and_runs_give_the_same_bits(batch):
    """(b): a budget of one byte puts every mask into a chunk of its own, 16 KiB makes chunks of several masks; a second run."""
    from object_detectors_amd import ops
    b = batch
    first = ops.rle_boundary(b["counts"], b["runs"], b["sizes"], b["dil"], b["boxes"])
    for budget in (1, 16 << 10, 1 << 20):
        again = ops.rle_boundary(b["counts"], b["runs"], b["sizes"], b["dil"], b["boxes"], budget_bytes=budget)
        assert np.array_equal(again[1], first[1])
        for x, y in zip((first[0], first[2], first[3]), (again[0], again[2], again[3])):
            assert torch.equal(x, y)
    _check(ops.rle_boundary(b["counts"], b["runs"], b["sizes"], b["dil"], b["boxes"], budget_bytes=1), b)


def test_coco_boundary_iou(batch):
    """(c): min(mask IoU, boundary IoU) with crowd flags on some ground truths."""
    from object_detectors_amd import ops
    masks = [m for m, d in batch["cases"] if m.shape == (45, 60) and d == 2]
    dt, gt = masks[:6], masks[3:]
    crowd = [j % 2 for j in range(len(gt))]
    enc = lambda ms: ops.mask_rle_dense(torch.from_numpy(np.stack(ms).astype(np.float32)).to(DEV), 0.5)
    got = ops.coco_boundary_iou(enc(dt), enc(gt), crowd)
    want = bd.combined_iou(dt, gt, crowd)
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(dt), len(gt)) and np.array_equal(_host(got), want)
    assert (want < co.mask_iou(dt, gt, crowd)).any() and (want == 1).any() and (want == 0).any()
    assert np.array_equal(_host(ops.coco_boundary_iou(enc(dt), enc(gt), crowd, 0.07)), bd.combined_iou(dt, gt, crowd, 0.07))


# ---- (d) the evaluators
def _flatten(ev, lvis):
    keys = sorted(ev["groups"])
    groups = [ev["groups"][k] for k in keys]
    I = len(ev["img_ids"])
    A, T = len(co.AREA_RNG), len(co.IOU_THRS)
    none = {"dt_match": np.zeros((A, T, 0)), "dt_ignore": np.zeros((A, T, 0)), "gt_match": np.zeros((A, T, 0)), "gt_ignore": np.zeros((A, 0))}
    cat = lambda name, axis, dtype: np.concatenate([g[name] for g in groups] + [none[name]], axis).astype(dtype)
    flat = {"group_keys": np.asarray([k * I + i for k, i in keys], np.int64),
            "iou": np.concatenate([g["iou"].reshape(-1) for g in groups] + [np.zeros(0)]),
            "dt_offsets": np.cumsum([0] + [len(g["dt"]) for g in groups]), "gt_offsets": np.cumsum([0] + [len(g["gt"]) for g in groups]),
            "iou_offsets": np.cumsum([0] + [len(g["dt"]) * len(g["gt"]) for g in groups]),
            "dt_area": np.concatenate([g["dt_area"] for g in groups] + [np.zeros(0)]),
            "dt_boxes": np.concatenate([g["dt_box"] for g in groups] + [np.zeros((0, 4), np.int64)]).astype(np.float64),
            "dt_score": np.concatenate([g["scores"] for g in groups] + [np.zeros(0)]),
            "gt_area": np.asarray([a["area"] for g in groups for a in g["gt"]], np.float64),
            "dt_match": cat("dt_match", 2, np.int32), "dt_ignore": cat("dt_ignore", 2, np.uint8), "gt_match": cat("gt_match", 2, np.int32),
            "gt_ignore": cat("gt_ignore", 1, np.uint8)}
    if lvis:
        flat["group_not_exhaustive"] = np.asarray([g["not_exhaustive"] for g in groups], np.uint8)
    return flat


@pytest.fixture(scope="module")
def sets():
    """The seeded data set in its two forms, its results as a results file holds them, and what the rules give: computed once."""
    dataset, results = bd.make_set()
    with_polygons, _same = bd.make_set(polygons=True)
    ev, precision, recall, stats = bd.run_coco(dataset, results)
    lev, lprecision, lrecall, lres = bd.run_lvis(with_polygons, results)
    return {"dataset": dataset, "polygons": with_polygons, "results": results, "rows": [so.to_result(r) for r in results],
            "coco": {"flat": _flatten(ev, False), "precision": precision, "recall": recall, "stats": stats},
            "lvis": {"flat": _flatten(lev, True), "precision": lprecision, "recall": lrecall, "res": lres}}


@pytest.fixture(scope="module")
def coco_evaluated(sets):
    from object_detectors_amd.cocoeval import COCOEval
    e = COCOEval(sets["dataset"], "boundary")
    e.add_results(sets["rows"])
    e.evaluate().accumulate().summarize()
    return e


@pytest.fixture(scope="module")
def lvis_evaluated(sets):
    from object_detectors_amd.lviseval import LVISSegmEval
    return LVISSegmEval(sets["polygons"], sets["rows"], iou_type="boundary").run()


def _against(e, want):
    flat = want["flat"]
    for name, w in flat.items():
        got = _host(getattr(e, name))
        assert np.array_equal(got, w), name
        if name in MATCH:
            assert got.dtype == w.dtype, name
    for name in ("precision", "recall"):
        got = getattr(e, name)
        assert got.dtype == np.float64 and got.shape == want[name].shape and np.array_equal(got, want[name]), name


def test_coco_evaluator_against_the_rules(sets, coco_evaluated):
    e = coco_evaluated
    assert e.iou_type == "boundary" and e.num_added == len(sets["rows"])
    _against(e, sets["coco"])
    assert e.stats.dtype == np.float64 and np.array_equal(e.stats, sets["coco"]["stats"])
    assert np.array_equal(e.summarize_per_category().shape, (len(e.cat_ids), 12))


def test_lvis_evaluator_against_the_rules(sets, lvis_evaluated):
    e = lvis_evaluated
    assert e.iou_type == "boundary" and e.num_added == len(sets["rows"])
    _against(e, sets["lvis"])
    got = e.get_results()
    assert list(got) == list(lo.KEYS)
    for k in lo.KEYS:
        assert got[k] == sets["lvis"]["res"][k], k
    import io
    buf = io.StringIO()
    e.print_results(file=buf)
    assert len(buf.getvalue().splitlines()) == 13


def test_boundary_differs_from_segm_on_the_device(sets, coco_evaluated, lvis_evaluated):
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISSegmEval
    segm = COCOEval(sets["dataset"], "segm")
    segm.add_results(sets["rows"])
    segm.evaluate().accumulate().summarize()
    assert torch.equal(segm.dt_area, coco_evaluated.dt_area) and torch.equal(segm.dt_boxes, coco_evaluated.dt_boxes)
    assert bool((coco_evaluated.iou <= segm.iou).all()) and bool((coco_evaluated.iou < segm.iou).any())
    assert not torch.equal(segm.dt_match, coco_evaluated.dt_match) and not np.array_equal(segm.stats, coco_evaluated.stats)
    lsegm = LVISSegmEval(sets["polygons"], sets["rows"]).run()
    assert lsegm.iou_type == "segm" and not torch.equal(lsegm.dt_match, lvis_evaluated.dt_match)
    assert list(lsegm.get_results().values()) != list(lvis_evaluated.get_results().values())


def _same_bits(a, b, names):
    for name in names + MATCH:
        x, y = _host(getattr(a, name)), _host(getattr(b, name))
        assert x.dtype == y.dtype and np.array_equal(x, y), name
    assert np.array_equal(a.precision, b.precision) and np.array_equal(a.recall, b.recall)


def test_detection_forms_agree(sets, coco_evaluated, lvis_evaluated):
    """Strings (the fixtures), RLEBatch and dense probabilities per image: the same bits."""
    from object_detectors_amd import ops
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISSegmEval
    results = sets["results"]
    names = ("group_keys", "dt_offsets", "gt_offsets", "iou_offsets", "dt_score", "dt_boxes", "dt_area", "gt_boxes", "gt_area", "gt_flag")
    evs = [COCOEval(sets["dataset"], "boundary"), COCOEval(sets["dataset"], "boundary"),
           LVISSegmEval(sets["polygons"], iou_type="boundary"), LVISSegmEval(sets["polygons"], iou_type="boundary")]
    for i in sorted(set(r["image_id"] for r in results)):
        rows = [r for r in results if r["image_id"] == i]
        cats = torch.tensor([r["category_id"] for r in rows], device=DEV)
        scores = torch.tensor([r["score"] for r in rows], dtype=torch.float32, device=DEV)
        probs = torch.from_numpy(np.stack([r["mask"] for r in rows]).astype(np.float32)).to(DEV)
        for n, e in enumerate(evs):
            e.add(i, cats, scores, masks=probs[:, None] if n % 2 else ops.mask_rle_dense(probs, 0.5))
    for e in evs[:2]:
        e.evaluate().accumulate()
        _same_bits(e, coco_evaluated, names)
        assert np.array_equal(e.summarize(), coco_evaluated.stats)
    for e in evs[2:]:
        _same_bits(e.run(), lvis_evaluated, names + ("group_not_exhaustive",))
        assert list(e.get_results().items()) == list(lvis_evaluated.get_results().items())


def test_bootstrap_with_unit_weights_reproduces_the_summary(coco_evaluated, lvis_evaluated):
    for e, n, want in ((coco_evaluated, 12, coco_evaluated.stats), (lvis_evaluated, 13, np.asarray(list(lvis_evaluated.get_results().values())))):
        stats, (ap, rc) = e.bootstrap(np.ones((2, len(e.img_ids)), np.int64), return_cells=True)
        assert stats.shape == (2, n) and np.array_equal(stats[0], stats[1])
        precision = e.precision if e.precision.ndim == 5 else e.precision[..., None]
        recall = e.recall if e.recall.ndim == 4 else e.recall[..., None]
        assert np.array_equal(_host(rc[0]), recall) and np.array_equal(_host(ap[0]), bo.ap_sum_of(precision, recall))
        # the statistics are means of those cells, summed in another order than numpy's: the last bits may differ
        assert np.array_equal(stats[0] == -1, want == -1) and np.allclose(stats[0], want, rtol=0, atol=1e-12)


def test_refusals(sets):
    from object_detectors_amd import ops
    from object_detectors_amd.cocoeval import COCOEval
    from object_detectors_amd.lviseval import LVISEval, LVISSegmEval
    from object_detectors_amd.rle import RLEBatch
    from object_detectors_amd.tide import ErrorBreakdown
    m = np.zeros((30, 40), np.uint8)
    m[5:20, 5:30] = 1
    c = torch.from_numpy(ro.encode(m).astype(np.int32))
    n = int(c.shape[0])
    args = lambda counts, **kw: dict(dict(counts=counts, runs=[0, n], sizes=[[30, 40]], dilation=1, boxes=[[5, 5, 25, 15]]), **kw)
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.rle_boundary(**args(c))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.rle_boundary(**args(c.to(DEV), boxes=torch.tensor([[5, 5, 25, 15]])))
    with pytest.raises(ValueError, match="CUDA/HIP"):
        RLEBatch((30, 40), c, [0, n]).boundary()
    with pytest.raises(ValueError, match="CUDA/HIP"):
        ops.coco_boundary_iou(RLEBatch((30, 40), c, [0, n]), RLEBatch((30, 40), c, [0, n]), [0])
    for bad in (dict(dilation=0), dict(boxes=[[5, 5, 36, 15]]), dict(boxes=[[-1, 5, 25, 15]]), dict(sizes=[[0, 40]]),
                dict(sizes=[[1 << 16, 1 << 15]]), dict(runs=[0, n + 1]), dict(index=[1])):
        with pytest.raises(ValueError, match="rle_boundary"):
            ops.rle_boundary(**args(c.to(DEV), **bad))
    # what the emit pass says of the numbers read back from the count pass, word for word (refused before any launch)
    from object_detectors_amd import _lib
    plan = ops.BoundaryPlan(**args(c.to(DEV)))
    offs, buf = plan.count(), torch.zeros(64, dtype=torch.int32, device=DEV)
    (first, num), = plan.chunks
    emit = lambda total=5, counts=_lib.ptr(buf), cap=5: _lib.lib().mi355det_rle_boundary_emit(
        *plan._tables, first, num, _lib.ptr(offs), total, counts, cap, None, None, _lib.ptr(plan.ws), plan.nbytes, _lib.stream_ptr())
    for kw, text in ((dict(cap=4), "rle_boundary_emit: capacity 4 is smaller than the 5 counts"),
                     (dict(total=0), "rle_boundary_emit: total_runs 0 is below one count per mask"),
                     (dict(counts=None), "rle_boundary_emit: missing operand")):
        assert emit(**kw) == -1, kw
        assert _lib.lib().mi355det_last_error().decode() == text
    for ratio in (0, -0.02):
        with pytest.raises(ValueError, match="dilation ratio"):
            COCOEval(sets["dataset"], "boundary", dilation_ratio=ratio)
        with pytest.raises(ValueError, match="dilation ratio"):
            LVISSegmEval(sets["polygons"], iou_type="boundary", dilation_ratio=ratio)
        with pytest.raises(ValueError, match="dilation ratio"):
            RLEBatch((30, 40), c.to(DEV), [0, n]).boundary(ratio)
    with pytest.raises(NotImplementedError, match="LVISSegmEval"):
        LVISEval(sets["polygons"], iou_type="boundary")
    with pytest.raises(ValueError, match="keypoints"):
        COCOEval(sets["dataset"], "keypoints")
    with pytest.raises(ValueError, match="bbox"):
        LVISSegmEval(sets["polygons"], iou_type="bbox")
    with pytest.raises(NotImplementedError):                          # polygons: as for segm, converted first
        COCOEval(sets["polygons"], "boundary")
    with pytest.raises(NotImplementedError, match="only bbox"):
        ErrorBreakdown(COCOEval(sets["dataset"], "boundary"))


def test_coco_evaluator_of_the_reference_takes_boundary(sets, coco_evaluated):
    """tvision CocoEvaluator(["segm", "boundary"]): the boundary numbers are COCOEval's."""
    from object_detectors_amd.tvision.coco_eval import CocoEvaluator
    ce = CocoEvaluator(sets["dataset"], ["segm", "boundary"])
    results = [r for r in sets["results"] if r["image_id"] != 1000]
    for i in sorted(set(r["image_id"] for r in results)):
        rows = [r for r in results if r["image_id"] == i]
        masks = torch.from_numpy(np.stack([r["mask"] for r in rows]).astype(np.float32)).to(DEV)[:, None]
        ce.update({i: {"boxes": torch.zeros((len(rows), 4), device=DEV), "scores": torch.tensor([r["score"] for r in rows], device=DEV),
                       "labels": torch.tensor([r["category_id"] for r in rows], device=DEV), "masks": masks}})
    ce.accumulate()
    ce.summarize()
    assert np.array_equal(ce.coco_eval["boundary"].stats, coco_evaluated.stats)
    assert not np.array_equal(ce.coco_eval["segm"].stats, coco_evaluated.stats)
