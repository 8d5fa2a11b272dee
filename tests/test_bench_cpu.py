"""CPU checks of bench.py's --dump-outputs: the sample positions and the files it writes."""
import numpy as np
import torch

import bench
from mojo_simdjson_amd import _lib


def test_dump_positions_are_fixed_sorted_and_one_per_stratum():
    assert np.array_equal(bench.dump_positions(1000, size=4096), np.arange(1000))
    n, size = 10_000_019, 4096
    p = bench.dump_positions(n, size=size)
    assert p.size == size and np.array_equal(p, bench.dump_positions(n, size=size))
    k = np.arange(size)
    assert np.all((p >= k * n // size) & (p < (k + 1) * n // size))  # distinct and sorted: one per stratum
    assert not np.array_equal(p, k * n // size)  # seeded, not the strata's first entries


def test_dump_outputs_writes_result_and_sampled_indices(tmp_path):
    n = 9000
    want = (np.arange(n + 50, dtype=np.int64) * 640_000) & 0xFFFFFFFF  # past 2^31: negative in the int32 tensor
    d_idx = torch.from_numpy(want.astype(np.uint32).view(np.int32))
    carry = _lib.MsjCarry()
    carry.count, carry.bytes, carry.utf8_error, carry.code = n - 3, 123456789, 1, 7
    bench.dump_outputs(str(tmp_path), "_rank1", d_idx, n, -5, n - 3, carry)
    res = np.load(tmp_path / "result_rank1.npy")
    assert res.dtype == np.float64
    assert list(res) == [-5, n - 3, n - 3, 123456789, 0, 0, 0, 0, 1, 0, 7, 0]
    got = np.load(tmp_path / "structural_indexes_rank1.npy")
    assert got.dtype == np.float64 and np.array_equal(got, want[bench.dump_positions(n)].astype(np.float64))

    bench.dump_outputs(str(tmp_path / "no_emit"), "", None, 0, 0, 0, carry)
    assert sorted(p.name for p in (tmp_path / "no_emit").iterdir()) == ["result.npy"]
