"""The workspace sizes msj_bucket_rows_device and msj_group_keys_device report (host arithmetic, no GPU), in the manner of
tests/test_match_strings_workspace.py, against tests/group_keys_workspace_sizes.json.

A size is the call's layout, measured (csrc/launch.h: msj_carver over csrc/group_keys_kernel.hip's layout), so it is held
twice: against the table recorded when the layout was written, and against the layout carved again here in Python.  Both
calls keep the counters alone, so no size depends on the capacity; the rows cross the grid of counts of
tests/test_workspace_sizes.py all the same.  To re-record the table after a change made on purpose:

    python -m tests.test_group_keys_workspace > tests/group_keys_workspace_sizes.json
"""
import json
import os
import sys

import pytest

from tests.test_workspace_sizes import ROWS

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "group_keys_workspace_sizes.json")
NAMES = ("msj_bucket_rows_workspace_bytes", "msj_group_keys_workspace_bytes")

STATE = 64   # sizeof(State): the counters
TAIL = 64    # the call's tail slack


def carved(rows):
    """The layout in Python: the one array starts at 0 and what follows at a multiple of 16 bytes (msj_carver.take)"""
    return ((STATE + 15) & ~15) + TAIL


def measure():
    from mojo_simdjson_amd import _lib

    lib = _lib.load()
    return {name: [[r, getattr(lib, name)(r)] for r in ROWS] for name in NAMES}


@pytest.fixture(scope="module")
def now():
    return measure()


@pytest.mark.parametrize("name", NAMES)
def test_sizes_as_recorded(now, name):
    with open(TABLE) as f:
        recorded = json.load(f)[name]
    assert [r[0] for r in recorded] == list(ROWS)
    differ = [(got[0], got[1], want[1]) for got, want in zip(now[name], recorded) if got != want]
    assert not differ, f"{len(differ)} sizes changed, (rows, now, recorded): {differ[:5]}"


@pytest.mark.parametrize("name", NAMES)
def test_sizes_are_the_layout(now, name):
    differ = [(r, got, carved(r)) for r, got in now[name] if got != carved(r)]
    assert not differ, differ[:5]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    m = measure()
    print("{\n" + ",\n".join(f' "{name}": {json.dumps(m[name], separators=(",", ":"))}' for name in NAMES) + "\n}")
