"""The workspace size msj_match_strings_device reports (host arithmetic, no GPU), in the manner of
tests/test_dictionary_order_workspace.py, against tests/match_strings_workspace_sizes.json.

The size is the call's layout, measured (csrc/launch.h: msj_carver over csrc/match_strings_kernel.hip's layout), so it is held
twice: against the table recorded when the layout was written, and against the layout carved again here in Python.  The rows
cross the grid of counts of tests/test_workspace_sizes.py, the patterns 1, 2 and 16.  To re-record the table after a change
made on purpose:

    python -m tests.test_match_strings_workspace > tests/match_strings_workspace_sizes.json
"""
import json
import os
import sys

import pytest

from tests.test_workspace_sizes import ROWS

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "match_strings_workspace_sizes.json")
NAME = "msj_match_strings_workspace_bytes"

PATTERNS = (1, 2, 16)
MAX_ROWS = 1 << 31   # match_strings_math.h: most_rows
STATE = 16           # sizeof(State): the verdict of the offsets check and three spare words
TAIL = 64            # the call's tail slack


def carved(rows, n_patterns):
    """The layout in Python: every array starts at a multiple of 16 bytes (msj_carver.take); per (pattern, row) the word
    the places compete on and the cursor"""
    n = min(rows, MAX_ROWS)
    at = 0
    for count, size in ((1, STATE), (n * n_patterns, 8), (n * n_patterns, 8)):
        at = (at + count * size + 15) & ~15
    return at + TAIL


def measure():
    from mojo_simdjson_amd import _lib

    f = getattr(_lib.load(), NAME)
    return {NAME: [[r, p, f(r, p)] for r in ROWS for p in PATTERNS]}


@pytest.fixture(scope="module")
def now():
    return measure()[NAME]


def test_sizes_as_recorded(now):
    with open(TABLE) as f:
        recorded = json.load(f)[NAME]
    assert [r[:2] for r in recorded] == [[r, p] for r in ROWS for p in PATTERNS]
    differ = [(got[0], got[1], got[2], want[2]) for got, want in zip(now, recorded) if got != want]
    assert not differ, f"{len(differ)} sizes changed, (rows, patterns, now, recorded): {differ[:5]}"


def test_sizes_are_the_layout(now):
    differ = [(r, p, got, carved(r, p)) for r, p, got in now if got != carved(r, p)]
    assert not differ, differ[:5]
    assert all(got <= 16 * min(r, MAX_ROWS) * p + STATE + TAIL + 32 for r, p, got in now)   # at most 16 bytes per (pattern, row)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print("{\n" + f' "{NAME}": {json.dumps(measure()[NAME], separators=(",", ":"))}' + "\n}")
