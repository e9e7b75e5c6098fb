"""Host-side checks of the long-tail baselines: the float64 oracle against autograd and against what the reference already
pins ('ce', 'bce' of oracle/tv_oracle.py on fixture g13), the repeat factors on a dataset small enough to work out by hand, the sampler
and the tail mask's threshold."""
import math

import numpy as np
import pytest

from oracle import detrand
from oracle import tv_oracle as tv
from tests import longtail_oracle as lo
from tests.longtail_cases import HAND_DATASET, HAND_IMG_FREQ, HAND_R

torch = pytest.importorskip("torch")


def _case(seed, n, k):
    x = detrand.uniform(seed, (n, k), -4, 4).astype(np.float64)
    lab = detrand.randint(seed + 1, (n,), 0, k)
    lab[::3] = 0
    counts = detrand.randint(seed + 2, (k,), 0, 5000)
    counts[1] = 0                                        # a class never seen: N = max(0, 1)
    tail = (detrand.uniform(seed + 3, (k,), 0, 1) < 0.4).astype(np.uint8)
    tail[0] = 0
    return x, lab, counts, tail


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("n,k", [(1, 2), (6, 7), (9, 65)])
def test_oracle_gradients_match_autograd(n, k):
    x, lab, counts, tail = _case(100 + n, n, k)
    xt = torch.from_numpy(x).requires_grad_(True)
    lo.seesaw_forward(xt, lab, counts).backward()
    loss, g = lo.seesaw(x, lab, counts)
    assert _rel(g, xt.grad.numpy()) < 1e-12
    xt = torch.from_numpy(x).requires_grad_(True)
    lo.eql_forward(xt, lab, tail).backward()
    loss, g = lo.eql(x, lab, tail)
    assert _rel(g, xt.grad.numpy()) < 1e-12


def test_seesaw_factors_by_hand():
    """Two classes beside the label, worked out: y = 0 with N = (100, 10, 1000), x = (0, log 3, 0): s = (1/5, 3/5, 1/5).
    M = ((10/100)^p, 1) for columns 1, 2; r = (3, 1): C = (3^q, 1)."""
    p, q = 0.8, 2.0
    x = np.array([[0.0, math.log(3.0), 0.0]])
    shift = lo.seesaw_shift(x, np.array([0]), np.array([100, 10, 1000]), p, q, 1e-2).numpy()
    np.testing.assert_allclose(shift, [[0.0, p * math.log(0.1) + q * math.log(3.0), 0.0]], rtol=1e-13, atol=1e-15)
    # eps: s_y = 1/5 replaced by 1/2 leaves only r_1 = 6/5 above 1
    shift = lo.seesaw_shift(x, np.array([0]), np.array([1, 1, 1]), p, q, 0.5).numpy()
    np.testing.assert_allclose(shift, [[0.0, q * math.log(1.2), 0.0]], rtol=1e-13, atol=1e-15)


def test_anchors_on_the_reference_fixture(golden):
    """Seesaw with p = q = 0 is the reference's 'ce', EQL with an empty tail its 'bce', on the frcnn_* arrays of fixture g13.  The gradients
    agree to 1e-12.  tv_oracle returns its loss rounded to float32, so the loss is compared after the same rounding: equal."""
    g = golden("g13_frcnn")
    x, lab = g["frcnn_logits"].astype(np.float64), g["frcnn_labels"]
    k = x.shape[1]
    counts = detrand.randint(7, (k,), 1, 100000)
    oc, _ob, og, _ogb = tv.fastrcnn_loss(g["frcnn_logits"], g["frcnn_breg"], lab, g["frcnn_tgt"], "ce", want_grad=True)
    loss, grad = lo.seesaw(x, lab, counts, p=0.0, q=0.0)
    assert np.float32(loss) == oc and _rel(grad, og) < 1e-12
    oc, _ob, og, _ogb = tv.fastrcnn_loss(g["frcnn_logits"], g["frcnn_breg"], lab, g["frcnn_tgt"], "bce", want_grad=True)
    loss, grad = lo.eql(x, lab, np.zeros(k, np.uint8))
    assert np.float32(loss) == oc and _rel(grad, og) < 1e-12
    # and the factors do something on the same arrays
    assert abs(lo.seesaw(x, lab, counts)[0] - float(oc)) > 1e-3


# ---- repeat factors: 7 images, 5 categories, t = 0.5 (tests/longtail_cases.py)
def test_repeat_factors_by_hand():
    from object_detectors_amd.dataset_stats import dataset_arrays
    a = dataset_arrays(HAND_DATASET, "lvis")
    assert a["n_images"] == 7 and a["n_categories"] == 5 and a["image_index"].size == 10
    assert lo.image_frequencies(a["image_index"], a["category_index"], 5).tolist() == HAND_IMG_FREQ
    r = lo.repeat_factors(a["image_index"], a["category_index"], 7, 5, t=0.5)
    np.testing.assert_allclose(r, HAND_R, rtol=1e-15)
    assert (r > 1).sum() == 4
    # the default threshold repeats nothing here: every category is in more than 1e-3 of the images
    assert lo.repeat_factors(a["image_index"], a["category_index"], 7, 5).tolist() == [1.0] * 7


def _sampler(r, **kw):
    from object_detectors_amd.dataset_stats import RepeatFactorSampler
    return RepeatFactorSampler(torch.tensor(r, dtype=torch.float64), **kw)


def test_sampler_repeats_and_epochs():
    r = [1.0, 2.0, 1.5, 3.25, 1.0, 2.75, 1.9] * 30
    s = _sampler(r, seed=3)
    s.set_epoch(4)
    a, b = list(s), list(s)
    assert a == b and len(s) == len(a)
    assert list(_sampler(r, seed=3 + 4)) == a                   # the generator is seeded seed + epoch
    s.set_epoch(5)
    c = list(s)
    assert c != a
    for lst in (a, c):
        times = np.bincount(lst, minlength=len(r))
        for ri, ti in zip(r, times):
            assert ti in (math.floor(ri), math.floor(ri) + 1)
            if ri == math.floor(ri):
                assert ti == ri
    assert sorted(a) != a                                       # shuffled
    ordered = list(_sampler(r, seed=3 + 4, shuffle=False))
    assert ordered == sorted(a)                                 # the same draws, unshuffled
    with pytest.raises(ValueError):
        _sampler([0.5, 1.0])
    with pytest.raises(ValueError):
        _sampler(r, rank=2, world=2)


def test_sampler_ranks_partition_the_epoch():
    r = [1.0, 2.0, 1.5, 3.25, 1.0, 2.75, 1.9, 1.0, 1.0] * 11     # whichever length the draw gives, the cut makes it even
    whole = list(_sampler(r, seed=11))
    r0, r1 = list(_sampler(r, seed=11, rank=0, world=2)), list(_sampler(r, seed=11, rank=1, world=2))
    even = whole[:len(whole) - len(whole) % 2]
    assert len(r0) == len(r1) == len(even) // 2
    assert r0 == even[0::2] and r1 == even[1::2]                # disjoint positions that together cover the cut list
    odd = [1.0] * 7                                             # 7 entries: one is cut
    assert len(list(_sampler(odd, rank=0, world=2))) == len(list(_sampler(odd, rank=1, world=2))) == 3


def test_tail_mask_threshold():
    from object_detectors_amd.dataset_stats import tail_from_frequencies
    # of 1000 images: index 0 is forced to 0 although it never occurs; 3/1000 and 2/1000 are not below 2e-3 (the side is '<');
    # a category that never occurs and 1/1000 are
    tail = tail_from_frequencies(torch.tensor([0, 3, 2, 0, 1], dtype=torch.int32), 1000, lam=2e-3)
    assert tail.dtype == torch.uint8 and tail.tolist() == [0, 0, 0, 1, 1]
    assert tail_from_frequencies(torch.tensor([5, 0, 2, 1760, 1761], dtype=torch.int32), 10 ** 6).tolist() == [0, 1, 1, 0, 0]


def test_new_ops_refuse_cpu_tensors():
    from object_detectors_amd import ops
    assert sorted(ops.FRCNN_LOSS_TYPES) == ["bce", "ce", "focal_loss", "gombit", "gombit_fl"]
    assert sorted(ops.FRCNN_LONGTAIL_TYPES) == ["eql", "seesaw"]
    z = torch.zeros
    with pytest.raises(ValueError):
        ops.fastrcnn_loss_longtail(z(2, 3), z(2, 12), z(2, dtype=torch.int64), z(2, 4), "seesaw", counts=z(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.label_histogram(z(2, dtype=torch.int64), z(3, dtype=torch.int64))
    with pytest.raises(ValueError):
        ops.repeat_factors(z(2, dtype=torch.int32), z(2, dtype=torch.int32), z(3, dtype=torch.int32), 4)
