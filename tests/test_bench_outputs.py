"""`bench.py --dump-outputs DIR` without a GPU: dump_outputs writes the accumulators as float32, whole when they fit and otherwise as a fixed,
seeded sample of their rows, so that a dump stays under 64 MB and two runs with the same arguments can be compared file for file."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_dump_outputs_writes_small_images_whole_and_a_fixed_row_sample_of_large_ones(tmp_path):
    bench = _bench()
    small = np.random.default_rng(1).random((40, 48, 4), dtype=np.float32)
    bench.dump_outputs(str(tmp_path / "small"), small)
    assert os.listdir(tmp_path / "small") == ["accum.npy"]
    got = np.load(tmp_path / "small" / "accum.npy")
    assert got.dtype == np.float32 and np.array_equal(got, small)

    big = np.arange(2048 * 2048 * 4, dtype=np.float32).reshape(2048, 2048, 4)      # 64 MiB: a 2048^2 workload's accumulators
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), big)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["accum.npy", "accum_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    rows = np.load(tmp_path / "a" / "accum_rows.npy")
    acc = np.load(tmp_path / "a" / "accum.npy")
    assert rows.dtype == np.float64 and acc.dtype == np.float32
    idx = rows.astype(np.int64)
    assert np.array_equal(idx, rows) and np.all(np.diff(idx) > 0) and 0 <= idx[0] and idx[-1] < 2048
    assert np.array_equal(acc, big[idx])
    for f in files:                                     # the sample is fixed: a second run writes the same files
        assert (tmp_path / "a" / f).read_bytes() == (tmp_path / "b" / f).read_bytes()
