"""The workspace size msj_dictionary_extend_device reports (host arithmetic, no GPU), in the manner of
tests/test_workspace_sizes.py and over its grid of counts, against tests/dictionary_extend_workspace_sizes.json.

The size is the call's layout, measured (csrc/launch.h: msj_carver over csrc/dictionary_extend_kernel.hip's layout), so it
is held twice: against the table recorded when the layout was written, and against the layout carved again here in Python --
the arrays of msj_dictionary_device's layout per ITEM, rows + dict_capacity of them.  To re-record the table after a
change made on purpose:

    python -m tests.test_dictionary_extend_workspace > tests/dictionary_extend_workspace_sizes.json
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

from tests.test_workspace_sizes import ROWS

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "dictionary_extend_workspace_sizes.json")
NAME = "msj_dictionary_extend_workspace_bytes"

B = 256              # kRows: items per block
LONG_CAP = 1024      # kLongCap: entries of the list of long items
MIN_SLOTS = 1024     # csrc/dictionary_math.h: kMinSlots
MAX_ITEMS = 1 << 31  # csrc/bytes_block.h: most_rows
STATE, TAIL = 64, 64  # sizeof(State); the call's tail slack


def carved(rows, dict_capacity):
    """The layout in Python: every array starts at a multiple of 16 bytes (msj_carver.take)"""
    items = min(rows + dict_capacity, MAX_ITEMS)
    slots = MIN_SLOTS
    while slots < 2 * items:
        slots *= 2
    at = 0
    for count, size in ((1, STATE), (items, 8), (items, 4), (slots, 4), (items // B + 1, 8), (items // B + 1, 8), (LONG_CAP, 4)):
        at = (at + count * size + 15) & ~15
    return at + TAIL


def measure():
    from mojo_simdjson_amd import _lib

    f = getattr(_lib.load(), NAME)
    f.restype, f.argtypes = ctypes.c_uint64, [ctypes.c_uint64, ctypes.c_uint64]
    return {NAME: [[r, c, f(r, c)] for r, c in itertools.product(ROWS, ROWS)]}


@pytest.fixture(scope="module")
def now():
    return measure()[NAME]


def test_sizes_as_recorded(now):
    with open(TABLE) as f:
        recorded = json.load(f)[NAME]
    assert [r[:2] for r in recorded] == [list(p) for p in itertools.product(ROWS, ROWS)]
    differ = [(got[:2], got[2], want[2]) for got, want in zip(now, recorded) if got != want]
    assert not differ, f"{len(differ)} sizes changed, (arguments, now, recorded): {differ[:5]}"


def test_sizes_are_the_layout(now):
    differ = [(r, c, got, carved(r, c)) for r, c, got in now if got != carved(r, c)]
    assert not differ, differ[:5]
    from mojo_simdjson_amd import _lib

    lib = _lib.load()
    lib.msj_dictionary_workspace_bytes.restype, lib.msj_dictionary_workspace_bytes.argtypes = ctypes.c_uint64, [ctypes.c_uint64]
    # without room for prior entries the layout is msj_dictionary_device's (the states have one size)
    assert all(got == lib.msj_dictionary_workspace_bytes(r) for r, c, got in now if c == 0)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("{\n" + f' "{NAME}": {json.dumps(measure()[NAME], separators=(",", ":"))}' + "\n}")
