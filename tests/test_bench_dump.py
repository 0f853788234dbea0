"""bench.py --dump-outputs: the files hold float32, stay inside the byte budget, keep every array that fits whole and
sample a larger one at the same seeded positions in every run."""
import os

import numpy as np
import torch

import bench


def test_dump_keeps_small_arrays_whole_and_samples_large_ones(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4000)
    big = torch.arange(5000, dtype=torch.float64)
    arrays = {"loss": torch.tensor(1.5), "m": torch.arange(12.0).reshape(3, 4), "big": big, "big2": -big}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, arrays)
    bench.dump_outputs(b, arrays)
    got = {f[:-4]: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    assert sorted(got) == sorted(arrays)
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 4000
    assert got["loss"].shape == () and float(got["loss"]) == 1.5
    assert np.array_equal(got["m"], arrays["m"].numpy())
    # 1000 float32 in all, 13 taken by the small arrays: the two large ones share the rest
    assert got["big"].shape == (493,) and got["big2"].shape == (494,)
    assert np.all(np.diff(got["big"]) > 0) and set(got["big"]) <= set(big.numpy().astype(np.float32))
    for name, v in got.items():
        assert np.array_equal(v, np.load(os.path.join(b, name + ".npy")))
