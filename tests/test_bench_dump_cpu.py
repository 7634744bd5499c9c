"""bench.py --dump-outputs (bench.dump_outputs) without a GPU: the results are written whole in their own dtype, and an output over
the 64 MB budget is cut to a fixed, seeded sample of its rows -- the same rows on every run."""
import numpy as np
import torch

import bench


def test_small_output_is_written_whole_in_its_dtype(tmp_path):
    out = torch.arange(12 * 5, dtype=torch.float64).reshape(12, 5)
    rec = bench.dump_outputs(str(tmp_path / "d"), "tau", out)
    a = np.load(tmp_path / "d" / "tau.npy")
    assert a.dtype == np.float64 and np.array_equal(a, out.numpy())
    assert rec == {"file": "tau.npy", "rows": 12, "of_rows": 12, "dtype": "float64"}


def test_large_output_is_a_fixed_sample_of_rows_under_the_budget(tmp_path):
    B, nv = 300_000, 64  # 76.8 MB of float32
    out = torch.arange(B, dtype=torch.float32)[:, None].repeat(1, nv)
    out[:, 1] = -out[:, 0]
    recs = [bench.dump_outputs(str(tmp_path / d), "ydd", out) for d in ("a", "b")]
    a, b = np.load(tmp_path / "a" / "ydd.npy"), np.load(tmp_path / "b" / "ydd.npy")
    assert a.dtype == np.float32 and a.nbytes <= bench.DUMP_MAX_BYTES and a.shape[1] == nv
    assert a.shape[0] == recs[0]["rows"] and recs[0]["of_rows"] == B and a.shape[0] > B // 2
    assert np.array_equal(a, b)  # the same rows on every run
    rows = a[:, 0].astype(np.int64)
    assert np.all(np.diff(rows) > 0)  # distinct rows, in batch order
    assert np.array_equal(a, out.numpy()[rows])  # whole rows of the output
