"""msj_join_rows_device past its grids (csrc/join_rows_kernel.hip), in the manner of tests/test_sort_rows_scale.py: the smallest
L, R, G and M at which every kernel's grid makes a second trip and every one-workgroup scan takes a second chunk, whole
tensors against the host twin and the numpy definition (tests/test_join_rows.py's ``run_join``).

The borders, with the constant each comes from:
  R = 1 048 576 + 1 025   jn_count / jn_scatter: kTileBlocks = 1 024 blocks x kTile = 1 024 rows, one whole tile and one row
                          past the grid; jn_scan: more than kScan = 1 024 tiles per bucket, so scan_in_place takes a second chunk
  L = 1 048 576 + 1 025   jn_left / jn_offsets: the same kTileBlocks x kTile; jn_total: the scan of the tiles' sums a second chunk
  G = 1 048 576 + 3       jn_clear: kClearBlocks = 4 096 blocks x 256 entries over count[0 .. G]; jn_start_sums / jn_start_apply:
                          kTileBlocks x kTile entries; jn_start_scan: a second chunk of kScan tile sums.  Three digits
  M > 4 194 304           jn_emit: kEmitBlocks = 4 096 blocks x kTile = 1 024 pairs (INNER and LEFT: a key held by 2 000 rows of
                          each side gives 4.0 M pairs on top of the million of the others; M stays under 20 M)
"""
import numpy as np
import pytest

from tests import test_join_rows as tjr
from tests import test_join_rows_math as tjm
from tests.test_join_rows import dev, jtw  # noqa: F401

pytestmark = pytest.mark.gpu

ROWS = 1024 * 1024 + 1025
G = 1024 * 1024 + 3
EMIT = 4096 * 1024


@pytest.fixture(scope="module")
def keys():
    rng = np.random.default_rng(3)
    def side():
        k = rng.integers(0, G, ROWS, dtype=np.int64)
        k[rng.random(ROWS) < 0.05] = -1
        k[rng.choice(ROWS, 2000, replace=False)] = G - 1        # the hot key: the last entry of count[]
        k[-1] = 0
        return k.astype(np.int32)
    return side(), side()


@pytest.mark.parametrize("kind", tjm.KINDS)
def test_past_every_grid(dev, jtw, keys, kind):  # noqa: F811
    want, _ = tjr.run_join(dev, jtw, keys[0], keys[1], G, kind, where=kind)
    M = want.res.n_pairs
    assert M < 20_000_000 and (M > EMIT if kind in (tjm.INNER, tjm.LEFT) else M > 0)
