"""AP-pool and AP-fixed on the device (csrc/pooled_kernels.hip, evalcore.GroupedEval.accumulate_pooled, the cut arguments of LVISEval) against
tests/pooled_oracle.py.  Both sides perform the same correctly rounded float64 operations on integers below 2^53, so every comparison is exact."""
import io

import numpy as np
import pytest
import torch

from tests import cocoeval_oracle as co
from tests import lviseval_oracle as lo
from tests import pooled_oracle as po
from tests import test_gpu_lviseval as tgl

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
REC = np.linspace(0, 1, 101)


def _dev(x, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype))).to(DEV)


def _pooled(lists, npig, score, match, ignore, rec=REC):
    """ops.pooled_accumulate on host arrays -> three numpy arrays."""
    from object_detectors_amd import ops
    offsets = np.cumsum([0] + [len(l) for l in lists]).astype(np.int64)
    order = np.concatenate([np.asarray(l, np.int64) for l in lists] + [np.zeros(0, np.int64)])
    got = ops.pooled_accumulate(_dev(order, np.int64), _dev(offsets), _dev(npig, np.int64), _dev(score, np.float64), _dev(match, np.int32),
                                _dev(ignore, np.uint8), _dev(rec, np.float64))
    return [g.cpu().numpy() for g in got]


def _same(got, want):
    for name, g, w in zip(("precision", "recall", "scores"), got, want):
        assert g.dtype == np.float64 and g.shape == w.shape and np.array_equal(g, w), name


def _random_case(A, T, seed):
    """Pools of every length at which the tiling changes path, their lists drawn from a random permutation of more slots than they use."""
    from object_detectors_amd import ops
    L = ops.pooled_tile()
    rng = np.random.RandomState(seed)
    lens = [0, 1, 63, 64, 65, L - 1, L, L + 1, 2 * L + 1, 3 * L + 5]
    nd = sum(lens) + 77
    perm = rng.permutation(nd)
    edges = np.cumsum([0] + lens)
    lists = [perm[edges[j]:edges[j + 1]] for j in range(len(lens))]
    score = rng.randint(1, 2001, nd) / 2000.0
    match = ((rng.rand(A, T, nd) < rng.uniform(.05, .6, (A, T, 1))) * rng.randint(1, 50, (A, T, nd))).astype(np.int32)
    ignore = (rng.rand(A, T, nd) < rng.uniform(0, .3, (A, T, 1))).astype(np.uint8)
    # npig: none, fewer than the true positives (rc passes 1), about as many, far more (a tail of thresholds is never reached)
    npig = [[[0, max(n // 20, 1), max(n // 3, 1), 2 * n + 3][(s + a) % 4] for a in range(A)] for s, n in enumerate(lens)]
    return lists, npig, score, match, ignore


@pytest.mark.parametrize("A, T", [(4, 10), (1, 1), (4, 16)])
def test_direct_calls_equal_the_rules_and_coco_accumulate(A, T):
    from object_detectors_amd import ops
    from object_detectors_amd.evalcore import NO_CUT
    lists, npig, score, match, ignore = _random_case(A, T, 100 + A * T)
    got = _pooled(lists, npig, score, match, ignore)
    want = po.pooled_vectorised(lists, npig, score, match, ignore, REC)
    _same(got, want)
    assert (want[0] == -1).any() and (want[0] == 0).any() and (want[0] > 0).any()
    # every pool is coco_accumulate on one category that holds the pool's slots
    nd = len(score)
    d_score, d_match, d_ignore, d_rec = _dev(score, np.float64), _dev(match, np.int32), _dev(ignore, np.uint8), _dev(REC, np.float64)
    rank = torch.zeros(nd, dtype=torch.int32, device=DEV)
    for s, order in enumerate(lists):
        G = max(npig[s])
        gt_ignore = (np.arange(G)[None, :] >= np.asarray(npig[s])[:, None]).astype(np.uint8).reshape(A, G)
        p, r, sc = ops.coco_accumulate(_dev([0, len(order)], np.int64), _dev([0, G], np.int64), _dev(order if len(order) else [0], np.int64), rank, d_score, d_match, d_ignore,
                                       _dev(gt_ignore), [NO_CUT], d_rec)
        one = (p[:, :, 0, :, 0].cpu().numpy(), r[:, 0, :, 0].cpu().numpy(), sc[:, :, 0, :, 0].cpu().numpy())
        _same([got[0][:, :, s], got[1][:, s], got[2][:, :, s]], one)


def test_two_runs_are_bit_identical():
    case = _random_case(4, 10, 7)
    first, second = _pooled(*case), _pooled(*case)
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def test_lists_that_cross_tiles():
    from object_detectors_amd import ops
    L = ops.pooled_tile()
    lens = [3 * L, L + 3, 2 * L + 9, 70, L + 1]
    edges = np.cumsum([0] + lens)
    nd = int(edges[-1])
    lists = [np.arange(edges[j], edges[j + 1]) for j in range(len(lens))]
    match, ignore = np.zeros((1, 1, nd), np.int32), np.zeros((1, 1, nd), np.uint8)
    score = 1.0 - np.arange(nd) / (2.0 * nd)
    match[0, 0, edges[0] + 2 * L:edges[1]] = 1            # pool 0: 2L false positives, then L true positives; npig = L
    match[0, 0, edges[1] + L] = 1                         # pool 1: its only true positive is the first slot of the second tile; npig = 1
    match[0, 0, edges[2]:edges[3]:3] = 1                  # pool 2: every third a true positive, npig four times their number
    tp2 = len(range(0, lens[2], 3))
    match[0, 0, edges[3]:edges[4]:2] = 1                  # pool 3: npig == 0 ...
    match[0, 0, edges[4]:edges[5]:2] = 1                  # ... beside pool 4, the same flags with ground truth
    ignore[0, 0, edges[4] + 1:edges[5]:4] = 1
    npig = [[L], [1], [4 * tp2], [0], [lens[4]]]
    p, r, s = _pooled(lists, npig, score, match, ignore)
    _same((p, r, s), po.pooled_vectorised(lists, npig, score, match, ignore, REC))
    # pool 0: the maximum from the right travels two tiles back to position 0
    best = np.float64(L) / (np.float64(2 * L) + np.float64(L) + np.spacing(1))
    assert p[0, 0, 0, 0] == best and s[0, 0, 0, 0] == score[0] and r[0, 0, 0] == 1.0
    assert p[0, 1, 0, 0] == best and s[0, 1, 0, 0] == score[2 * L + (L + 99) // 100 - 1]
    assert (p[0, :, 0, 0] == best).all() and s[0, 100, 0, 0] == score[3 * L - 1]
    # pool 1: threshold 0 at position 0, every other threshold at position L, on the tile edge
    one = np.float64(1) / (np.float64(L) + np.float64(1) + np.spacing(1))
    assert (p[0, :, 1, 0] == one).all() and s[0, 0, 1, 0] == score[edges[1]] and (s[0, 1:, 1, 0] == score[edges[1] + L]).all()
    # pool 2: recall 1/4: the thresholds past it are never reached
    assert r[0, 2, 0] == 0.25 and (p[0, 26:, 2, 0] == 0).all() and (s[0, 26:, 2, 0] == 0).all() and (p[0, :26, 2, 0] > 0).all()
    # pools 3 and 4
    assert (p[0, :, 3, 0] == -1).all() and (s[0, :, 3, 0] == -1).all() and r[0, 3, 0] == -1
    assert (p[0, :, 4, 0] >= 0).all() and r[0, 4, 0] > 0


def test_no_positions_at_all():
    p, r, s = _pooled([[], []], [[3, 0], [0, 2]], np.zeros(5), np.ones((2, 3, 5), np.int32), np.zeros((2, 3, 5), np.uint8))
    assert p.shape == (3, 101, 2, 2) and r.shape == (3, 2, 2)
    for x in (p, s):
        assert (x[:, :, 0, 0] == 0).all() and (x[:, :, 0, 1] == -1).all() and (x[:, :, 1, 0] == -1).all() and (x[:, :, 1, 1] == 0).all()
    assert r[:, 0].tolist() == [[0, -1]] * 3 and r[:, 1].tolist() == [[-1, 0]] * 3


# ---- end to end
@pytest.fixture(scope="module")
def lvis_set():
    dataset, results = tgl.make_set()
    return dataset, results


def _assert_lvis_equal(e, want, max_dets):
    ev, precision, recall, res, text = want
    flat = tgl._flatten(ev)
    assert np.array_equal(tgl._host(e.group_keys), flat["keys"])
    for name in ("dt_offsets", "gt_offsets", "iou_offsets"):
        assert np.array_equal(tgl._host(getattr(e, name)), flat[name]), name
    assert np.array_equal(tgl._host(e.iou), flat["iou"])
    for name in ("dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        got = tgl._host(getattr(e, name))
        assert got.dtype == flat[name].dtype and np.array_equal(got, flat[name]), name
    assert e.precision.dtype == np.float64 and np.array_equal(e.precision, precision) and np.array_equal(e.recall, recall)
    got = e.get_results()
    assert list(got) == list(res) == list(e.stat_names) and f"AR@{max_dets}" in got
    for k in res:
        assert got[k] == res[k], k
    out = io.StringIO()
    e.print_results(file=out)
    assert out.getvalue() == text and f"maxDets={max_dets:>3d}" in text


def test_lvis_pools_against_the_rules(lvis_set):
    from object_detectors_amd.lviseval import LVISEval
    dataset, results = lvis_set
    ev = lo.evaluate(dataset, results)
    pools = [list(range(len(tgl.CATS)))] + ev["freq_groups"]
    want = po.pooled_of_groups(ev, pools)
    assert (want[0][:, :, :, 0] > 0).any(axis=(0, 1)).all()                       # every pool draws a curve
    e = LVISEval(dataset, results).run()
    before = (e.precision.tobytes(), e.recall.tobytes(), list(e.get_results().items()))
    assert e.accumulate_pooled() is e
    _same((e.precision_pool, e.recall_pool, e.scores_pool), want)
    assert e.precision_pool.shape == (10, 101, 4, 4) and e.recall_pool.shape == (10, 4, 4)
    assert (e.precision.tobytes(), e.recall.tobytes(), list(e.get_results().items())) == before
    got = e.summarize_pooled()
    expect = po.summarize(want[0], want[1], ("", "r", "c", "f"))
    assert list(got) == ["APpool", "APpool50", "APpool75", "APpools", "APpoolm", "APpooll", "APpoolr", "APpoolc", "APpoolf", "ARpool"]
    assert list(got.items()) == expect
    out = io.StringIO()
    e.print_pooled(file=out)
    assert out.getvalue() == "".join(f" {k:<10} = {v:0.3f}\n" for k, v in expect)
    # pools of the caller's own: each category alone is that category's cell of accumulate()
    e.accumulate_pooled([[k] for k in range(len(tgl.CATS))])
    assert np.array_equal(e.precision_pool, e.precision) and np.array_equal(e.recall_pool, e.recall)


def test_lvis_fixed_cut_against_the_rules(lvis_set):
    from object_detectors_amd.lviseval import LVISEval
    dataset, results = lvis_set
    _kept, removed = po.category_cut(dataset, results, 40)
    assert sum(1 for n in removed.values() if n > 0) >= 2 and sum(1 for n in removed.values() if n == 0) >= 2, removed
    per_image = np.bincount([tgl.IMG_IDS.index(r["image_id"]) for r in results if r["image_id"] in tgl.IMG_IDS])
    assert per_image.max() - lo.MAX_DETS == 20                                   # what the per-image cut would have removed
    capped = LVISEval(dataset, results, max_dets=None, max_dets_per_cat=40).run()
    _assert_lvis_equal(capped, po.run_cut(dataset, results, None, 40), -1)
    both = LVISEval(dataset, results, max_dets=30, max_dets_per_cat=60).run()     # both cuts bind: the category cut first
    want = po.run_cut(dataset, results, 30, 60)
    assert want[0]["counters"]["cut_dropped"] > 0
    _assert_lvis_equal(both, want, 30)
    fixed = LVISEval.fixed(dataset, results).run()
    want = po.run_cut(dataset, results, None, 10000)
    assert want[0]["counters"]["cut_dropped"] == 0 and fixed.num_dt > LVISEval(dataset, results).evaluate().num_dt
    _assert_lvis_equal(fixed, want, -1)
    assert lo.MAX_DETS == 300
    # the default arguments, in the same process: as before
    tgl._assert_equal(LVISEval(dataset, results).run(), tgl._want(dataset, results))


def test_segm_category_cut_equals_the_cut_result_file():
    """LVISSegmEval shares the front end: the category cut on the device equals the evaluation of the result file cut on the host."""
    from object_detectors_amd.lviseval import LVISSegmEval
    from tests import lvissegm_oracle as so
    dataset, results = so.make_set()
    rows = [so.to_result(r) for r in results]
    _kept, removed = po.category_cut(dataset, rows, 1)
    per_cat = max(2, sorted(n + 1 for n in removed.values())[len(removed) // 2])          # the median category size: cuts some, spares some
    kept, removed = po.category_cut(dataset, rows, per_cat)
    assert any(n > 0 for n in removed.values()) and any(n == 0 for n in removed.values())
    cut = LVISSegmEval(dataset, rows, max_dets=None, max_dets_per_cat=per_cat).run()
    host = LVISSegmEval(dataset, kept, max_dets=-1).run()
    assert cut.num_dt == host.num_dt < LVISSegmEval(dataset, rows, max_dets=None).evaluate().num_dt
    for name in ("group_keys", "dt_offsets", "iou", "dt_score", "dt_area", "dt_boxes", "dt_match", "dt_ignore", "gt_match", "gt_ignore"):
        assert torch.equal(getattr(cut, name), getattr(host, name)), name
    assert np.array_equal(cut.precision, host.precision) and np.array_equal(cut.recall, host.recall)
    assert list(cut.get_results().items()) == list(host.get_results().items()) and "AR@-1" in cut.get_results()
    cut.accumulate_pooled()
    host.accumulate_pooled()
    assert np.array_equal(cut.precision_pool, host.precision_pool) and cut.summarize_pooled() == host.summarize_pooled()


def test_protocols_tool_prints_the_three_tables(lvis_set, tmp_path, capsys):
    import importlib.util
    import json
    import os
    from object_detectors_amd.lviseval import LVISEval
    dataset, results = lvis_set
    gt_path, dt_path = tmp_path / "gt.json", tmp_path / "dt.json"
    gt_path.write_text(json.dumps(dataset))
    dt_path.write_text(json.dumps(results))
    spec = importlib.util.spec_from_file_location("lvis_protocols", os.path.join(os.path.dirname(os.path.dirname(__file__)), "tools", "lvis_protocols.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    tool.main(["--gt", str(gt_path), "--results", str(dt_path), "--per-cat", "40"])
    got = capsys.readouterr().out
    want = io.StringIO()
    LVISEval(dataset, results).run().print_results(file=want)
    fixed = LVISEval(dataset, results, max_dets=None, max_dets_per_cat=40).run()
    fixed.print_results(file=want)
    fixed.accumulate_pooled().print_pooled(file=want)
    titles = ["standard: 300 detections per image", "AP-fixed: no per-image cut, 40 detections per category", "AP-pool, on the AP-fixed detections"]
    assert [l for l in got.splitlines() if l not in titles] == want.getvalue().splitlines()
    assert [l for l in got.splitlines() if l in titles] == titles


def test_coco_pool_against_the_rules():
    from object_detectors_amd.cocoeval import COCOEval
    from tests.test_gpu_cocoeval import make_bbox_set
    dataset, results = make_bbox_set(True, 5)
    ev = co.evaluate(dataset, results)                                            # its groups keep the 100 best: ranks >= 100 are left out
    assert any(len(g["dt"]) == 100 for g in ev["groups"].values())
    want = po.pooled_of_groups(ev, [[0, 1, 2]], co.REC_THRS)
    e = COCOEval(dataset, "bbox")
    e.add_results(results)
    e.evaluate()
    assert int(e.dt_rank.max()) == 99 and e.num_dt == sum(len(g["dt"]) for g in ev["groups"].values()) < len(results) - 30   # so does the front end
    e.accumulate_pooled()
    _same((e.precision_pool, e.recall_pool, e.scores_pool), want)
    assert list(e.summarize_pooled()) == ["APpool", "APpool50", "APpool75", "APpools", "APpoolm", "APpooll", "ARpool"]
    assert list(e.summarize_pooled().items()) == po.summarize(want[0], want[1], iou_thrs=co.IOU_THRS)
    # a slot whose rank is not below the largest cut is not in the list
    rank = e.dt_rank.clone()
    rank[::7] = 100
    e.dt_rank = rank
    e.accumulate_pooled([[0, 1, 2], [1]])
    _same((e.precision_pool, e.recall_pool, e.scores_pool), po.pooled_of_groups(ev, [[0, 1, 2], [1]], co.REC_THRS, rank=rank.cpu().numpy(), cut=100))
