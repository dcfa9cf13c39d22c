"""bench.py --dump-outputs without a GPU: the rows written are all of them or a fixed seeded sample within the budget, and the
arrays land as float32 / float64 .npy files."""
import os

import numpy as np

import bench


def test_small_outputs_are_written_whole():
    assert np.array_equal(bench.dump_rows(512, 100 * 12 + 8), np.arange(512))


def test_large_outputs_are_a_fixed_sample_within_the_budget():
    row_bytes = 1000 * 12 + 8                    # the default workload: 10000 queries x k = 1000
    a = bench.dump_rows(10_000, row_bytes)
    b = bench.dump_rows(10_000, row_bytes)
    assert np.array_equal(a, b)
    assert 0 < len(a) < 10_000 and len(a) * row_bytes <= bench.DUMP_BUDGET <= 64 * 10 ** 6
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 10_000


def test_dump_scan_writes_float_arrays(tmp_path):
    dists = np.sort(np.random.default_rng(0).random((6, 4), dtype=np.float32), axis=1)
    ids = np.arange(24, dtype=np.int32).reshape(6, 4)
    ids[0, 0] = -1                               # the int32 bit pattern of uint32 0xffffffff
    bench.dump_scan(str(tmp_path), dists, ids)
    assert sorted(os.listdir(str(tmp_path))) == ["dists.npy", "ids.npy", "query_rows.npy"]
    d, i, r = (np.load(str(tmp_path / (n + ".npy"))) for n in ("dists", "ids", "query_rows"))
    assert d.dtype == np.float32 and np.array_equal(d, dists)
    assert i.dtype == np.float64 and i[0, 0] == 2.0 ** 32 - 1 and np.array_equal(i.ravel()[1:], np.arange(1, 24))
    assert r.dtype == np.float64 and np.array_equal(r, np.arange(6))
