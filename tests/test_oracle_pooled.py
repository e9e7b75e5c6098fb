"""tests/pooled_oracle.py pinned: pools small enough to work out by hand, with the answers written out here, and the vectorised form against the
loops on seeded random lists.  CPU only."""
import numpy as np

from tests import pooled_oracle as po

REC = np.linspace(0, 1, 101)


def _one_cell(matched, ignored, npig, scores=None, form=po.pooled_loops):
    """One pool, one area range, one threshold; the list is the slots in the order given -> precision [R], recall, scores [R]."""
    n = len(matched)
    sc = np.linspace(1, .5, n) if scores is None else np.asarray(scores, np.float64)
    p, r, s = form([np.arange(n)], [[npig]], sc, np.asarray(matched, np.int32).reshape(1, 1, n), np.asarray(ignored, np.uint8).reshape(1, 1, n), REC)
    return p[0, :, 0, 0], r[0, 0, 0], s[0, :, 0, 0]


def test_one_true_positive_reaches_every_threshold():
    p, r, s = _one_cell([1], [0], 1, scores=[.75])
    assert r == 1.0
    assert (p == 1.0 / (1.0 + 2.0 ** -52)).all() and (s == .75).all()


def test_envelope_lifts_the_first_position():
    # F F T T with two ground truths: tp = 0 0 1 2, fp = 2 -> pr = 0, 0, 1/3, 2/4; from the right: .5 .5 .5 .5; rc = 0 0 .5 1
    p, r, s = _one_cell([0, 0, 1, 1], [0, 0, 0, 0], 2, scores=[.9, .8, .7, .6])
    half = 2.0 / (2.0 + 2.0 + 2.0 ** -52)                          # = 0.5: 4 + 2^-52 rounds to 4
    assert half == 0.5 and r == 1.0
    assert p[0] == half and s[0] == .9                             # threshold 0: the first position, lifted from 0 to the last true positive's
    assert (p[1:51] == half).all() and (s[1:51] == .7).all()       # 0.01 .. 0.50: the first true positive, 1/3 lifted as well
    assert (p[51:] == half).all() and (s[51:] == .6).all()


def test_precision_falls_where_nothing_lifts_it():
    # T F with one ground truth of two: pr = 1, 1/2; rc = .5 .5: thresholds past .5 are never reached
    p, r, s = _one_cell([1, 0], [0, 0], 2, scores=[.9, .8])
    assert r == 0.5
    assert (p[:51] == 1.0 / (1.0 + 2.0 ** -52)).all() and (s[:51] == .9).all()
    assert (p[51:] == 0).all() and (s[51:] == 0).all()


def test_all_ignored_gives_precision_zero():
    p, r, s = _one_cell([1, 0, 1], [1, 1, 1], 3, scores=[.9, .8, .7])
    assert r == 0.0
    assert p[0] == 0.0 and s[0] == .9                              # rc = 0 >= 0 at the first position: 0 / (0 + 0 + 2^-52)
    assert (p[1:] == 0).all() and (s[1:] == 0).all()


def test_no_ground_truth_gives_minus_one():
    p, r, s = _one_cell([0, 0], [0, 0], 0)
    assert r == -1 and (p == -1).all() and (s == -1).all()


def test_empty_list_with_ground_truth_gives_zero():
    p, r, s = _one_cell([], [], 4)
    assert r == 0 and (p == 0).all() and (s == 0).all()


def test_pool_list_is_stable_and_cut():
    scores = np.asarray([.5, .9, .5, .9, .1, .5])
    cat = np.asarray([0, 1, 2, 0, 1, 0])
    rank = np.asarray([0, 0, 0, 0, 0, 7])
    assert po.pool_list(scores, cat, rank, 5, [0, 1, 2]).tolist() == [1, 3, 0, 2, 4]
    assert po.pool_list(scores, cat, rank, 8, [0]).tolist() == [3, 0, 5]
    assert po.pool_list(scores, cat, rank, 8, []).tolist() == []


def test_vectorised_form_equals_the_loops():
    rng = np.random.RandomState(11)
    for _ in range(200):
        n = int(rng.randint(0, 301))
        nd = n + int(rng.randint(0, 5))
        A, T = int(rng.randint(1, 3)), int(rng.randint(1, 4))
        score = rng.randint(1, 41, nd) / 40.0                      # ties
        match = (rng.rand(A, T, nd) < rng.rand()).astype(np.int32) * rng.randint(1, 9, (A, T, nd)).astype(np.int32)
        ignore = (rng.rand(A, T, nd) < 0.2).astype(np.uint8)
        order = rng.permutation(nd)[:n]
        order = order[np.argsort(-score[order], kind="mergesort")]
        cut = int(rng.randint(0, n + 1))
        lists, npig = [order, order[:cut], order[:0]], rng.randint(0, n + 2, (3, A)).tolist()
        want = po.pooled_loops(lists, npig, score, match, ignore, REC)
        got = po.pooled_vectorised(lists, npig, score, match, ignore, REC)
        for w, g in zip(want, got):
            assert w.dtype == g.dtype == np.float64 and np.array_equal(w, g)


def test_category_cut_keeps_the_best_in_order_of_arrival():
    dataset = {"images": [{"id": 1}, {"id": 2}]}
    rows = [{"image_id": 1, "category_id": 5, "score": .2}, {"image_id": 2, "category_id": 5, "score": .9}, {"image_id": 3, "category_id": 5, "score": 1.},
            {"image_id": 1, "category_id": 5, "score": .9}, {"image_id": 2, "category_id": 8, "score": .1}, {"image_id": 2, "category_id": 5, "score": .5}]
    kept, removed = po.category_cut(dataset, rows, 2)
    assert kept == [rows[1], rows[3], rows[4]] and removed == {5: 2, 8: 0}
