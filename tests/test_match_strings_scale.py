"""msj_match_strings_device past its grids (csrc/match_strings_kernel.hip), in the manner of
tests/test_dictionary_order_scale.py: the smallest column at which every grid-strided kernel makes a second trip and the
staging of a tile's offsets takes every path, whole tensors against the host twin, and the twin's single-piece column once
against ``bytes.find``.

The borders, with the constant each comes from (``tmm.constants``):
  R = 1 024 x 256 + 256 + 1    one block and one row past kRowBlocks = 1 024 blocks x 256 rows: ms_check, ms_step (per pattern)
                               and ms_finish wrap
  bytes = 2 049 x 8 192 + 1    one tile and one byte past kByteBlocks = 2 048 blocks x kTile = 8 192 bytes: ms_bytes takes two
                               tiles per block, the second with the row index carried over from the first
  9 000 empty rows at byte 0   more rows overlap tile 0 than it has bytes, and more than kStage = 1 024: the searches of that
                               tile run on memory
  rows of 20 bytes             about 400 rows per tile: the staging takes a second step of kStageChunk = 256 offsets
  one row of 10 MiB            hundreds of tiles inside one row; its only match of the second pattern ends at its last byte
"""
import numpy as np
import pytest

from tests import test_match_strings as tms
from tests import test_match_strings_math as tmm
from tests.test_match_strings import dev, tw  # noqa: F401

pytestmark = pytest.mark.gpu


class FlatColumn(tmm.Column):
    """Every row with a value, the values back to back: tmm.Column's members from numpy arrays"""

    def __init__(self, lengths, data):
        self.R = len(lengths)
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
        self.valid = np.ones(self.R, dtype=np.uint8)
        self.data, self.bytes_len = data, len(data)
        assert int(self.offsets[-1]) == self.bytes_len
        self.place(0)


def test_past_every_grid(dev, tw):  # noqa: F811
    c = tmm.constants(tw)
    R = c["row_blocks"] * c["threads"] + c["threads"] + 1
    total = (c["byte_blocks"] + 1) * c["tile"] + 1
    empty, big = c["tile"] + 808, 10 << 20
    assert empty > c["stage"] and 8 * c["tile"] // 20 > c["chunk"]
    lengths = np.full(R, 20, dtype=np.int64)
    lengths[:empty] = 0
    lengths[empty + 5000] = big
    lengths[-1] = total - (int(lengths.sum()) - 20)
    assert lengths[-1] > 0 and int(lengths.sum()) == total
    rng = np.random.default_rng(4)
    data = rng.choice(np.frombuffer(b"abcdefgh ", dtype=np.uint8), total)
    offsets = np.concatenate([[0], np.cumsum(lengths)])
    for k in rng.choice(R, 3000, replace=False):  # needles inside rows, across row borders, and at the long row's very end
        at = int(offsets[k]) + int(rng.integers(0, 24))
        if at + 6 <= total:
            data[at:at + 6] = np.frombuffer(b"NEEDLE", dtype=np.uint8)
    end = int(offsets[empty + 5001])
    data[end - 3:end] = np.frombuffer(b"END", dtype=np.uint8)
    col = FlatColumn(lengths, data.tobytes())
    specs = [b"NEEDLE", ([b"a", b"END"], tmm.AT_END)]
    want_res, _, want_rec = tms.run_match(dev, tw, col, specs, definition=False)
    raw, off = col.data, col.offsets.tolist()
    found = [raw.find(b"NEEDLE", off[k], off[k + 1]) for k in range(R)]
    assert want_rec["code"][0].tolist() == [20 if f < 0 or f + 6 > off[k + 1] else 0 for k, f in enumerate(found)]
    assert all(f < 0 or want_rec["bits"][0][k] == f - off[k] for k, f in enumerate(found) if want_rec["code"][0][k] == 0)
    assert 1000 < int((want_rec["code"][0] == 0).sum()) < 3000 and want_rec["code"][1][empty + 5000] == 0 and want_res.n_values == R
