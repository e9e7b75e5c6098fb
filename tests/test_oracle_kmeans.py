"""tests/kmeans_oracle.py pinned: hand-checked cases of every rule the header states, and scikit-learn's Lloyd where it is installed.
No GPU."""
import math

import numpy as np
import pytest

from tests import kmeans_oracle as O


def test_a_tie_goes_to_the_lower_index():
    """The point 1 is at distance 1 from both centres 0 and 2; duplicated centres tie everywhere."""
    p = O.one_pass([[1.0], [0.0], [2.0]], [[0.0], [2.0]], "euclid")
    assert p["labels"].tolist() == [0, 0, 1] and p["dmin"].tolist() == [1.0, 0.0, 0.0] and p["gap"] == 0.0
    p = O.one_pass([[3.0, 4.0]], [[1.0, 1.0], [1.0, 1.0]], "euclid")
    assert p["labels"].tolist() == [0] and p["dmin"].tolist() == [13.0]


def test_the_iou_distance_by_hand():
    """(2, 2) against (1, 4): intersection 1 x 2 = 2, union 4 + 4 - 2 = 6; against itself 0."""
    d = O.distances([[2.0, 2.0]], [[1.0, 4.0], [2.0, 2.0]], "iou")
    assert d.tolist() == [[1.0 - 2.0 / 6.0, 0.0]]


def test_an_empty_cluster_keeps_its_centre():
    """Centre 2 at 100 attracts nothing, stays at 100 through every pass and has count 0 at the end."""
    X = [[0.0], [1.0], [10.0], [11.0]]
    r = O.lloyd(X, [[0.0], [10.0], [100.0]], "euclid")
    assert r["centers"].tolist() == [[0.5], [10.5], [100.0]] and r["counts"].tolist() == [2, 2, 0]
    assert r["labels"].tolist() == [0, 0, 1, 1] and r["n_iter"] == 2 and r["changed"] == 0 and r["inertia"] == 1.0


def test_the_first_pass_counts_as_changed_and_max_iter_stops():
    """Centres that already are the means still take two passes: the first always counts as changed.  max_iter = 1 returns the initial
    centres with the first assignment."""
    X = [[0.0], [1.0], [10.0], [11.0]]
    assert O.lloyd(X, [[0.5], [10.5]], "euclid")["n_iter"] == 2
    r = O.lloyd(X, [[0.0], [1.0]], "euclid", max_iter=1)
    assert r["n_iter"] == 1 and r["centers"].tolist() == [[0.0], [1.0]] and r["labels"].tolist() == [0, 1, 1, 1] and r["changed"] == 4
    assert r["inertia"] == 81.0 + 100.0


def dataset():
    images = [{"id": 7, "width": 100, "height": 200}, {"id": 3, "width": 10, "height": 10}]
    boxes = [(7, 10, 20),       # 0.1 x 0.1: aspect 1, area 0.1 * 0.1 = 0.010000000000000002 > 0.01: band 1
             (3, 1, 1),         # the same quotients from another image: band 1
             (7, 5, 10),        # 0.05 x 0.05 = 0.0025000000000000005: band 0
             (7, 50, 100),      # 0.5 x 0.5 = 0.25: band 2
             (7, 12.5, 16),     # 0.125 x 0.08 = 0.01 exactly: on the edge, no band
             (7, 25, 80),       # 0.25 x 0.4 = 0.1 exactly: on the edge, no band
             (7, 10, 0),        # zero height: aspect inf, dropped
             (7, 0, 0),         # 0 / 0: NaN, dropped
             (7, 10, 100),      # 0.1 x 0.5: aspect 0.2 exactly: strict, dropped
             (7, 50, 20),       # 0.5 x 0.1: aspect 5 exactly: strict, dropped
             (99, 10, 20)]      # an unlisted image: no row at all
    anns = [{"image_id": i, "bbox": [0, 0, w, h], "category_id": 1} for i, w, h in boxes]
    return {"images": images, "annotations": anns}


def test_features_bands_and_their_edges():
    f, band = O.box_features(dataset())
    assert f.shape == (10, 4)
    assert band.tolist() == [1, 1, 0, 2, -1, -1, -1, -1, -1, -1]
    assert f[0].tolist() == [0.1, 0.1, 1.0, 0.1 * 0.1] and f[1].tolist() == f[0].tolist()
    assert f[4, 3] == 0.01 and f[5, 3] == 0.1 and f[4, 2] == 0.125 / 0.08
    assert f[6, 2] == math.inf and f[6, 3] == 0.0
    assert np.isnan(f[7, 2]) and f[7, 3] == 0.0
    assert f[8, 2] == 0.2 and f[9, 2] == 5.0


def test_seeded_init_is_problem_major_from_one_generator():
    torch = pytest.importorskip("torch")
    Xs = [np.arange(10.0).reshape(5, 2), np.arange(100.0, 114.0).reshape(7, 2)]
    got = O.seeded_init(Xs, 2, 3, seed=5)
    g = torch.Generator().manual_seed(5)
    for p, Xp in enumerate(Xs):
        for r in range(3):
            rows = torch.randperm(len(Xp), generator=g)[:2].numpy()
            assert np.array_equal(got[p][r], Xp[rows])


def boxes(seed, n):
    """Seeded log-uniform (w, h) with their aspect and area: the four features of the script."""
    rng = np.random.default_rng(seed)
    w, h = np.exp(rng.uniform(np.log(0.01), np.log(0.9), n)), np.exp(rng.uniform(np.log(0.01), np.log(0.9), n))
    return np.stack([w, h, w / h, w * h], axis=1)


@pytest.mark.parametrize("seed,n,k", [(1, 800, 3), (2, 800, 9), (3, 4000, 3), (4, 16000, 9)])
def test_against_scikit_learn(seed, n, k):
    """KMeans(init=C0, n_init=1, tol=0, algorithm='lloyd') stops as the rules do (on an unchanged assignment).  Labels must be equal; it
    centres the data first and sums in its own order, so its centres may differ by the bound of any summation order, 4 * N * 2^-53 * max|X|
    (the factor 4: the centring subtraction and its undoing, the sum, the division)."""
    cluster = pytest.importorskip("sklearn.cluster")
    X = boxes(seed, n)
    C0 = X[np.random.default_rng(seed + 100).permutation(n)[:k]]
    mine = O.lloyd(X, C0, "euclid", 300)
    assert mine["counts"].min() > 0 and mine["n_iter"] < 300
    km = cluster.KMeans(n_clusters=k, init=C0, n_init=1, tol=0, max_iter=300, algorithm="lloyd").fit(X)
    assert np.array_equal(km.labels_, mine["labels"])
    err = np.abs(km.cluster_centers_ - mine["centers"]).max()
    print(f"seed {seed} n {n} k {k}: passes {mine['n_iter']}, largest centre difference {err:.3g}, gap {mine['gap']:.3g}")
    assert err <= 4 * n * 2.0 ** -53 * np.abs(X).max()
