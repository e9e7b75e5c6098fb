"""bench.py --dump-outputs on the host: what the step's caller holds, as float32 .npy files; arrays above the sample size reduced to the
same seeded positions in every run, so two builds can be compared file for file within the dump budget."""
import os

import numpy as np
import torch

import bench


class _Plan:
    def __init__(self, heads, c):
        self.heads, self.c = heads, c

    def head_outputs(self):          # as engine.Plan: NCHW-shaped views of NHWC buffers padded in C
        return [h[..., :self.c].permute(0, 3, 1, 2) for h in self.heads]


class _Engine:
    def __init__(self, seed):
        g = torch.Generator().manual_seed(seed)
        self.flat_w = torch.randn(5000, generator=g)
        self.flat_g = torch.randn(5000, generator=g)
        self.buffers = {"a.bn.running_mean": torch.randn(3, generator=g), "a.bn.running_var": torch.rand(3, generator=g),
                        "b.bn.running_mean": torch.randn(5, generator=g), "b.bn.running_var": torch.rand(5, generator=g)}
        self._last_plan = _Plan([torch.randn((2, g_, g_, 8), generator=g) for g_ in (2, 4, 8)], 6)


def _dump(tmp_path, tag, seed=0):
    eng = _Engine(seed)
    d = str(tmp_path / tag)
    bench.dump_outputs(d, bench.step_outputs(eng, torch.arange(12, dtype=torch.float32)), sample=300)
    return eng, {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_files_dtype_and_small_arrays_whole(tmp_path):
    eng, out = _dump(tmp_path, "a")
    assert sorted(out) == ["bn_running_mean", "bn_running_var", "grads", "head0", "head1", "head2", "loss", "weights"]
    assert all(a.dtype == np.float32 and a.ndim == 1 for a in out.values())
    np.testing.assert_array_equal(out["loss"], np.arange(12, dtype=np.float32))
    np.testing.assert_array_equal(out["bn_running_mean"], torch.cat([eng.buffers["a.bn.running_mean"], eng.buffers["b.bn.running_mean"]]).numpy())
    # a head of 2 x 6 x 2 x 2 = 48 elements is written whole, in the NCHW order of the view the caller receives
    np.testing.assert_array_equal(out["head0"], eng._last_plan.head_outputs()[0].reshape(-1).numpy())


def test_dump_large_arrays_same_sample_every_run(tmp_path):
    eng, a = _dump(tmp_path, "a")
    _, b = _dump(tmp_path, "b")
    for name in ("weights", "grads", "head2"):
        assert a[name].shape == (300,)
        np.testing.assert_array_equal(a[name], b[name])
    # the sample is taken at fixed positions, independent of the values: another engine's weights are sampled where these were
    eng_c, c = _dump(tmp_path, "c", seed=1)
    pos = np.sort(np.random.default_rng(5000).choice(5000, 300, replace=False))
    np.testing.assert_array_equal(a["weights"], eng.flat_w.numpy()[pos])
    np.testing.assert_array_equal(c["weights"], eng_c.flat_w.numpy()[pos])


def test_dump_budget():
    # five arrays reach the sample size (three heads, weights, gradients); the loss and the BatchNorm statistics are far smaller
    assert 4 * (5 * bench.DUMP_SAMPLE + 12 + 2 * 100_000) <= 64 * 2 ** 20
