"""The workspace size msj_dictionary_order_device reports (host arithmetic, no GPU), in the manner of
tests/test_join_rows_workspace.py, against tests/dictionary_order_workspace_sizes.json.

The size is the call's layout, measured (csrc/launch.h: msj_carver over csrc/dictionary_order_kernel.hip's layout), so it is
held twice: against the table recorded when the layout was written, and against the layout carved again here in Python.  The
capacity crosses the grid of counts of tests/test_workspace_sizes.py -- the rounding borders of a tile, of 16 bytes and of the
entry limit.  To re-record the table after a change made on purpose:

    python -m tests.test_dictionary_order_workspace > tests/dictionary_order_workspace_sizes.json
"""
import ctypes
import json
import os
import sys

import pytest

from tests.test_workspace_sizes import ROWS

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dictionary_order_workspace_sizes.json")
NAME = "msj_dictionary_order_workspace_bytes"

TILE = 1024             # kTile: positions or tied entries of a block's tile
BUCKETS = 256           # dictionary_order_math.h: kBuckets
MAX_ENTRIES = 1 << 31   # dictionary_order_math.h: most_entries
STATE = 3 * 8 + 2 * 8 + 2 * 4 + BUCKETS * 4   # sizeof(State): three counters, the round's tied count and the rounds run, the mask, the bucket totals
TAIL = 64               # the call's tail slack


def tiles(n):
    return (n + TILE - 1) // TILE


def carved(capacity):
    """The layout in Python: every array starts at a multiple of 16 bytes (msj_carver.take)"""
    n = min(capacity, MAX_ENTRIES)
    t = tiles(n)
    at = 0
    for count, size in ((1, STATE), (t + 1, 4), (t, 8), (t, 8), (t, 8), (t, 8), (n, 8), (n, 8), (n, 4), (n, 8), (n, 8), (n, 4), (n, 4), (n, 4),
                        (BUCKETS * t, 4), (t + 1, 4)):
        at = (at + count * size + 15) & ~15
    return at + TAIL


def measure():
    from mojo_simdjson_amd import _lib

    f = getattr(_lib.load(), NAME)
    return {NAME: [[c, f(c)] for c in ROWS]}


@pytest.fixture(scope="module")
def now():
    return measure()[NAME]


def test_sizes_as_recorded(now):
    with open(TABLE) as f:
        recorded = json.load(f)[NAME]
    assert [r[0] for r in recorded] == list(ROWS)
    differ = [(got[0], got[1], want[1]) for got, want in zip(now, recorded) if got != want]
    assert not differ, f"{len(differ)} sizes changed, (capacity, now, recorded): {differ[:5]}"


def test_sizes_are_the_layout(now):
    differ = [(c, got, carved(c)) for c, got in now if got != carved(c)]
    assert not differ, differ[:5]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("{\n" + f' "{NAME}": {json.dumps(measure()[NAME], separators=(",", ":"))}' + "\n}")
