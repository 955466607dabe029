"""bench.py --dump-outputs helpers (host only): the row sample is fixed from run to run and
fits the dump budget, and the arrays land as float32 / float64 .npy files that hold the
integer results exactly."""
import os

import numpy as np

import bench


def test_sample_rows_keeps_every_row_that_fits():
    assert np.array_equal(bench.sample_rows(100, 1 << 10), np.arange(100))


def test_sample_rows_is_a_fixed_sorted_sample_within_budget():
    row_bytes = 10000 * 12 + 8  # a G100 row: u64 distances as float64 + one next-hop byte as float32
    a = bench.sample_rows(10000, row_bytes)
    b = bench.sample_rows(10000, row_bytes)
    assert np.array_equal(a, b)
    assert a.dtype == np.int64 and len(a) == bench.DUMP_BUDGET_BYTES // row_bytes
    assert len(a) * row_bytes <= bench.DUMP_BUDGET_BYTES
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 10000


def test_dump_outputs_writes_exact_float_arrays(tmp_path):
    dist = np.array([[0, 1, (1 << 53) - 1], [7, 0, 3]], dtype=np.uint64)
    nh = np.array([[[0], [255]], [[1], [2]]], dtype=np.uint8)
    counts = np.array([[0, 70000], [1 << 30, 5]], dtype=np.int32)
    out = str(tmp_path / "dump")
    bench.dump_outputs(out, {"dist": dist, "next_hops": nh, "changed": counts})
    assert sorted(os.listdir(out)) == ["changed.npy", "dist.npy", "next_hops.npy"]
    got = {n: np.load(os.path.join(out, n + ".npy")) for n in ("dist", "next_hops", "changed")}
    assert got["dist"].dtype == np.float64 and np.array_equal(got["dist"].astype(np.uint64), dist)
    assert got["next_hops"].dtype == np.float32 and np.array_equal(got["next_hops"].astype(np.uint8), nh)
    assert got["changed"].dtype == np.float64 and np.array_equal(got["changed"].astype(np.int32), counts)


def test_dump_outputs_names_each_rank_under_several_gpus(tmp_path):
    bench.dump_outputs(str(tmp_path), {"dist": np.zeros((1, 2), dtype=np.uint64)}, rank=3, world=8)
    assert os.listdir(str(tmp_path)) == ["dist.rank3.npy"]
