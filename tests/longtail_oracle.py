"""Float64 statement of the long-tail baselines (include/mi355det.h, "Long-tail baselines"): Seesaw loss, Equalization
loss v1 and the repeat factors, written as the rules read.  torch-CPU for the two losses, so that the forward can also run under autograd
(tests/test_longtail_host.py checks the analytic gradients against it); numpy for the repeat factors.  A checker only.

The losses take logits that already carry the class scale (x = class_scale * logits), like oracle/tv_oracle.py:fastrcnn_loss; the caller
multiplies the returned gradient by the scale to get the gradient w.r.t. the unscaled logits."""
import numpy as np
import torch


def _t(a, dtype=torch.float64):
    return a.to(dtype) if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def seesaw_shift(x, labels, counts, p=0.8, q=2.0, eps=1e-2):
    """log(M * C) [n, k], a constant of the loss: built from x.detach()."""
    x, labels = _t(x).detach(), _t(labels, torch.int64)
    n, k = x.shape
    rows = torch.arange(n)
    N = torch.clamp(_t(counts, torch.int64), min=1).to(torch.float64)
    Nj, Ny = N[None, :], N[labels][:, None]
    M = torch.where(Nj < Ny, (Nj / Ny) ** p, torch.ones_like(x))
    sig = torch.softmax(x, 1)
    r = sig / torch.clamp(sig[rows, labels], min=eps)[:, None]
    C = torch.where(r > 1, r ** q, torch.ones_like(x))
    M[rows, labels] = 1.0
    C[rows, labels] = 1.0
    return torch.log(M * C)


def seesaw_forward(x, labels, counts, p=0.8, q=2.0, eps=1e-2):
    """mean over rows of logsumexp(x') - x'_y; differentiable in x (torch float64), M and C detached."""
    x, labels = _t(x), _t(labels, torch.int64)
    xp = x + seesaw_shift(x, labels, counts, p, q, eps)
    return (torch.logsumexp(xp, 1) - xp[torch.arange(x.shape[0]), labels]).mean()


def seesaw(x, labels, counts, p=0.8, q=2.0, eps=1e-2):
    """-> (loss, d loss / d x [n, k]) as float64 numpy: (softmax(x') - onehot) / n."""
    x, labels = _t(x), _t(labels, torch.int64)
    n = x.shape[0]
    xp = x + seesaw_shift(x, labels, counts, p, q, eps)
    g = torch.softmax(xp, 1)
    g[torch.arange(n), labels] -= 1.0
    return float(seesaw_forward(x, labels, counts, p, q, eps)), (g / n).numpy()


def eql_weights(labels, tail, k):
    """(t, w) [n, k]: t_j = [j = y and j != 0], w_j = 1 - [y > 0] tail_j (1 - t_j)."""
    labels = _t(labels, torch.int64)
    n = labels.shape[0]
    t = torch.zeros(n, k, dtype=torch.float64)
    t[torch.arange(n), labels] = 1.0
    t[:, 0] = 0.0
    E = (labels > 0).to(torch.float64)[:, None]
    w = 1.0 - E * _t(tail)[None, :] * (1.0 - t)
    return t, w


def eql_forward(x, labels, tail):
    """sum_rows sum_j w_j BCEWithLogits(x_j, t_j) / n; differentiable in x."""
    x = _t(x)
    t, w = eql_weights(labels, tail, x.shape[1])
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    return (w * bce).sum() / x.shape[0]


def eql(x, labels, tail):
    """-> (loss, d loss / d x [n, k]) as float64 numpy: w (sigmoid(x) - t) / n."""
    x = _t(x)
    t, w = eql_weights(labels, tail, x.shape[1])
    return float(eql_forward(x, labels, tail)), (w * (torch.sigmoid(x) - t) / x.shape[0]).numpy()


def image_frequencies(image_index, category_index, n_categories):
    """img_freq [n_categories]: the number of distinct images per category."""
    pairs = np.unique(np.stack([np.asarray(image_index, np.int64), np.asarray(category_index, np.int64)], 1), axis=0)
    return np.bincount(pairs[:, 1], minlength=n_categories)


def repeat_factors(image_index, category_index, n_images, n_categories, t=1e-3):
    """r [n_images] float64: f_c = img_freq_c / n_images, r_c = max(1, sqrt(t / f_c)), r_i = max over image i's annotations, 1 without any."""
    f = image_frequencies(image_index, category_index, n_categories).astype(np.float64) / np.float64(n_images)
    with np.errstate(divide="ignore"):
        r_c = np.maximum(1.0, np.sqrt(np.float64(t) / f))          # f = 0: inf, never read (no annotation carries that category)
    r = np.ones(n_images, np.float64)
    np.maximum.at(r, np.asarray(image_index, np.int64), r_c[np.asarray(category_index, np.int64)])
    return r
