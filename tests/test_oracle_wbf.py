"""The literal host form of weighted boxes fusion (tests/wbf_oracle.py) against the written expectations of the hand cases, and the facts
the device kernel rests on: running sums give the bits of the member-list form, and a founding box must be kept as it is.  CPU only."""
import numpy as np
import pytest

from tests import wbf_cases as wc
from tests import wbf_oracle as wo

HAND = wc.hand_cases()


def _bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.int64)


def _fuse(c, **kw):
    return wo.fuse(c["models"], c["images"], **dict(c["kw"], **kw))


@pytest.mark.parametrize("c", HAND, ids=[c["name"] for c in HAND])
def test_hand_case(c):
    wc.check_expectation(c, _fuse(c))


def test_drift_needs_the_moved_box():
    """The third box of the drift case overlaps the first alone below the threshold."""
    boxes = np.asarray([[0, 0, 10, 10], [3.5, 0, 13.5, 10]], np.float64)
    assert abs(wo.overlap(boxes[0], boxes[1]) - 65 / 135) < 1e-15 and wo.overlap(boxes[0], boxes[1]) < .55


def test_boundary_case_cluster_counts():
    c, sizes = wc.boundary_case(96)
    got = _fuse(c)
    for image, n in sizes.items():
        rows = got["image_id"] == image
        assert int(rows.sum()) == n and sorted(got["members"][rows].tolist()) == wc.boundary_members(sizes, image)
    assert got["dropped"] == dict.fromkeys(wo.DROP_REASONS, 0)


def cluster_group_running(boxes, scores, iou_thr):
    """cluster_group with running sums in place of the member lists: what the kernel does."""
    S, C, fused, lists, of = [], [], [], [], []
    for j in range(len(scores)):
        best, at = np.float64(0), -1
        for c, F in enumerate(fused):
            v = wo.overlap(F, boxes[j])
            if v > best:
                best, at = v, c
        if at >= 0 and best > iou_thr:
            S[at], C[at] = S[at] + scores[j] * boxes[j], C[at] + scores[j]
            fused[at] = S[at] / C[at]
            lists[at].append(j)
        else:
            at = len(lists)
            S.append(scores[j] * boxes[j]), C.append(scores[j]), fused.append(boxes[j].copy()), lists.append([j])
        of.append(at)
    return lists, fused, of


RANDOM = wc.random_cases()


@pytest.fixture(scope="module")
def random_results():
    return [_fuse(c) for c in RANDOM]


@pytest.mark.parametrize("k", range(len(RANDOM)), ids=[c["name"] for c in RANDOM])
def test_random_sets_are_not_degenerate(random_results, k):
    got, c = random_results[k], RANDOM[k]
    n = got["members"]
    print("clusters", len(n), "multi-member", int((n > 1).sum()), "more than two", int((n > 2).sum()), "largest", int(n.max()))
    assert (n > 1).mean() >= .30 and (n > 2).mean() >= .05 and n.max() >= 6
    scores = [r["score"] for res in c["models"] for r in res]
    assert len(set(scores)) < len(scores) // 10                   # exact ties are everywhere
    assert len(set(got["image_id"].tolist())) >= 35 and len(set(got["category_id"].tolist())) == 6


@pytest.mark.parametrize("k", range(len(RANDOM)), ids=[c["name"] for c in RANDOM])
def test_running_sums_reproduce_member_lists(random_results, k):
    want, got = random_results[k], _fuse(RANDOM[k], cluster=cluster_group_running)
    assert np.array_equal(_bits(got["score"]), _bits(want["score"])) and np.array_equal(_bits(got["box"]), _bits(want["box"]))
    for key in ("image_id", "category_id", "members", "cluster_of"):
        assert np.array_equal(got[key], want[key])


def test_a_founding_box_is_not_its_quotient():
    """(s' * x) / s' is not x often enough that a founder's box has to be kept as it is."""
    rng = np.random.RandomState(0)
    s, x = rng.randint(1, 20, 40000) / 20, rng.uniform(0, 600, 40000)
    off = int(((s * x) / s != x).sum())
    print("(s * x) / s != x for", off, "of", len(x))
    assert off > len(x) // 50


def test_empty_second_model_halves_the_scores():
    """A set in which nothing fuses (disjoint boxes), with an empty second model at weights (1, 1), avg: every box comes back as it is with
    (s / 1) * min(1, 2) / 2 = half its score."""
    c, _sizes = wc.boundary_case(96)
    rows = [r for r in c["models"][0] if r["image_id"] <= 7]
    got = wo.fuse([rows, []], c["images"], weights=(1, 1))
    assert len(got["score"]) == len(rows) == 325 and (got["members"] == 1).all()
    back = got["cluster_of"][:len(rows)]
    assert sorted(back.tolist()) == list(range(len(rows)))
    assert np.array_equal(_bits(got["score"][back]), _bits(np.asarray([r["score"] for r in rows]) / 2))
    assert np.array_equal(_bits(got["box"][back]), _bits(np.asarray([r["bbox"] for r in rows])))
    assert got["image_id"][back].tolist() == [r["image_id"] for r in rows]
