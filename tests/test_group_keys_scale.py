"""msj_bucket_rows_device and msj_group_keys_device past their grids (csrc/group_keys_kernel.hip: kGridBlocks = 1 024 blocks of
256 rows for both kernels): R = 262 401 is one block and one row past 1 024 * 256 rows, so block 0 comes round a second time
with a full block and once more -- as the grid's second block -- with a single row, whose key bytes are the tail.  The widest
key (W = 88: 23 MB of key bytes, the LDS tile at its 22 KiB) and the narrowest (W = 5: R * W mod 16 = 5).  Whole tensors
against the host twin (tests/group_keys_math_host.cpp), the fill behind every room; the columns are made with numpy."""
import numpy as np
import pytest

from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import test_group_keys as tgk
from tests import test_group_keys_math as tgm

pytestmark = pytest.mark.gpu

GRID_BLOCKS, BLOCK_ROWS = 1024, 256
R = GRID_BLOCKS * BLOCK_ROWS + BLOCK_ROWS + 1

dev = tgk.dev
gtw = tgk.gtw


def number_column(seed, n):
    """Records of every kind by numpy: int64 and doubles near each other (so equal reals meet), some without bits, some with a
    code, some strings"""
    rng = np.random.default_rng(seed)
    col = np.zeros(n, dtype=FIELD_DTYPE)
    small = rng.integers(-50, 50, n)
    is_double = rng.random(n) < 0.4
    col["bits"] = np.where(is_double, (small / 2.0).view(np.uint64), small.view(np.uint64))
    col["type"] = np.where(is_double, ord("d"), ord("l"))
    col["token"] = np.arange(n, dtype=np.uint32)
    odd = rng.random(n)
    col["flags"][odd < 0.02] = 64
    col["code"][(odd >= 0.02) & (odd < 0.04)] = 20
    col["type"][(odd >= 0.04) & (odd < 0.06)] = ord('"')
    wide = (odd >= 0.06) & (odd < 0.10)
    col["bits"][wide] = rng.integers(0, 2**63, int(wide.sum()), dtype=np.uint64) * 2 + 1
    return col


def code_column(seed, n):
    return np.random.default_rng(seed).integers(-2, 1000, n).astype(np.int32)


def test_the_size_is_past_the_grid():
    assert R == 262401 and (R * 5) % 16 == 5 and (R * 88) % 16 == 8


@pytest.mark.parametrize("W", (88, 5))
def test_keys_past_the_grid(dev, gtw, W):
    if W == 88:
        parts = [tgm.Part(number_column(j, R + 1), tgm.NULL_IS_GROUP if j % 2 else 0) for j in range(8)]
    else:
        parts = [tgm.Part(code_column(9, R + 1))]
    want = tgk.run_keys(dev, gtw, parts, R, capacity=R, bytes_capacity=R * W)
    assert (want.res.code, want.res.n_rows, want.res.key_width, want.res.bytes_len) == (0, R, W, R * W)
    assert 0 < want.res.n_null_rows and 0 < want.res.n_keys < R


def test_bucket_past_the_grid(dev, gtw):
    rows = number_column(3, R + 1)
    want = tgk.run_bucket(dev, gtw, rows, R, 60000, -7, capacity=R)
    assert want.res.code == 0 and min(want.res.n_bucketed, want.res.n_range, want.res.n_skipped, want.res.n_other) > 0
    tgk.run_bucket(dev, gtw, rows, R, 60000, -7, in_place=True)
