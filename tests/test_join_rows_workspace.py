"""The workspace size msj_join_rows_device reports (host arithmetic, no GPU), in the manner of
tests/test_dictionary_extend_workspace.py, against tests/join_rows_workspace_sizes.json.

The size is the call's layout, measured (csrc/launch.h: msj_carver over csrc/join_rows_kernel.hip's layout), so it is held
twice: against the table recorded when the layout was written, and against the layout carved again here in Python.  Each of
the three arguments crosses the grid of counts of tests/test_workspace_sizes.py -- the rounding borders of a tile, of 16
bytes and of the row limit -- while the other two stand at its anchors.  To re-record the table after a change made on
purpose:

    python -m tests.test_join_rows_workspace > tests/join_rows_workspace_sizes.json
"""
import ctypes
import json
import os
import sys

import pytest

from tests.test_workspace_sizes import ANCHORS, ROWS

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "join_rows_workspace_sizes.json")
NAME = "msj_join_rows_workspace_bytes"

TILE = 1024          # kTile: rows, keys or pairs of a block's tile
BUCKETS = 256        # join_rows_math.h: kBuckets
MAX_ROWS = 1 << 31   # csrc/bytes_block.h: most_rows; join_rows_math.h: most_keys
STATE = 32 + 4 * BUCKETS * 4   # sizeof(State): four counters, the bucket totals of four passes
TAIL = 64            # the call's tail slack


def triples():
    out = []
    for which in range(3):
        for anchor in ANCHORS:
            for x in ROWS:
                t = [anchor, anchor, anchor]
                t[which] = x
                out.append(tuple(t))
    return out


def tiles(n):
    return (n + TILE - 1) // TILE


def carved(left_rows, right_rows, keys_capacity):
    """The layout in Python: every array starts at a multiple of 16 bytes (msj_carver.take)"""
    l, r, g = min(left_rows, MAX_ROWS), min(right_rows, MAX_ROWS), min(keys_capacity, MAX_ROWS) + 1
    at = 0
    for count, size in ((1, STATE), (g, 4), (tiles(g), 4), (r, 4), (r, 4), (r, 4), (r, 4), (BUCKETS * tiles(r), 4), (l, 4), (l + 1, 8),
                        (tiles(l) + 1, 8)):
        at = (at + count * size + 15) & ~15
    return at + TAIL


def measure():
    from mojo_simdjson_amd import _lib

    f = getattr(_lib.load(), NAME)
    f.restype, f.argtypes = ctypes.c_uint64, [ctypes.c_uint64] * 3
    return {NAME: [[a, b, c, f(a, b, c)] for a, b, c in triples()]}


@pytest.fixture(scope="module")
def now():
    return measure()[NAME]


def test_sizes_as_recorded(now):
    with open(TABLE) as f:
        recorded = json.load(f)[NAME]
    assert [r[:3] for r in recorded] == [list(t) for t in triples()]
    differ = [(got[:3], got[3], want[3]) for got, want in zip(now, recorded) if got != want]
    assert not differ, f"{len(differ)} sizes changed, (arguments, now, recorded): {differ[:5]}"


def test_sizes_are_the_layout(now):
    differ = [(a, b, c, got, carved(a, b, c)) for a, b, c, got in now if got != carved(a, b, c)]
    assert not differ, differ[:5]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("{\n" + f' "{NAME}": {json.dumps(measure()[NAME], separators=(",", ":"))}' + "\n}")
