"""bench.py --dump-outputs: the arrays of the last timed step as float32 .npy, small ones whole, the largest as a fixed seeded
sample of their rows, 64 MB in all at most (the writer itself, on CPU tensors)."""
import os

import numpy as np
import torch

import bench


def _dump(path, arrays):
    bench.dump_outputs(str(path), arrays)
    return {f[:-4]: np.load(os.path.join(path, f)) for f in sorted(os.listdir(path))}


def test_dump_outputs_budget_sample_and_repeatability(tmp_path):
    rows = 3_000_000
    big = torch.arange(rows, dtype=torch.float32).view(rows, 1).repeat(1, 8)   # row i holds i: a sampled row says where it came from
    arrays = {"big": big, "image": torch.rand(256 * 256, 3, generator=torch.Generator().manual_seed(1)),
              "radii": torch.arange(1000, dtype=torch.int32), "tau": torch.ones(6), "language": torch.empty(0, 15)}
    a = _dump(tmp_path / "a", arrays)
    assert set(a) == {"big", "image", "radii", "tau"}   # (an empty array - F = 0 - is not written)
    assert all(v.dtype == np.float32 for v in a.values())
    total = sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in a)
    assert total <= 64 * 10**6 and total > 0.9 * bench.DUMP_BUDGET_BYTES
    for k in ("image", "radii", "tau"):   # under their share: whole
        assert np.array_equal(a[k], arrays[k].float().numpy())
    idx = a["big"][:, 0]
    assert 0 < len(idx) < rows and np.all(np.diff(idx) > 0) and np.all(a["big"] == idx[:, None])
    b = _dump(tmp_path / "b", arrays)
    assert all(np.array_equal(a[k], b[k]) for k in a)   # the sample is fixed: equal shapes, equal rows
