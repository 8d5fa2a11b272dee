"""The workspace size every call behind stage 1 reports (host arithmetic, no GPU), against tests/workspace_sizes.json.

A call's size is its layout, measured (csrc/launch.h: msj_carver), and callers budget device memory with these numbers
(INTEGRATION.md), so a size changes only when a layout is changed on purpose.  The table holds what the library
returned when it was recorded, over a grid that crosses every rounding border of the layouts.  To re-record it after
such a change:

    python -m tests.test_workspace_sizes > tests/workspace_sizes.json
"""
import ctypes
import itertools
import json
import os
import sys

import pytest

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "workspace_sizes.json")

U64, U32, INT = ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int

# counts on both sides of the borders the layouts round at: a block of 256 rows, a tile of 1 024, a block of 2 048 tokens,
# an odd count over 2^20, the most a window holds
COUNTS = (0, 1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049, (1 << 20) + 37, (1 << 31) - 1)
ROWS = COUNTS + ((1 << 31) + 5,)  # a capacity above the row limit of csrc/bytes_block.h (most_rows)
ANCHORS = (257, (1 << 20) + 37)   # where the other counts stand while one crosses the grid, in the calls with three
MATCH = (0, 1, 2)
PATHS = (1, 16)
RAW_FLAGS = (0, 1)  # MSJ_RAW_COMPACT

# name -> (argument types, the values of each argument)
CALLS = {
    "msj_tokens_workspace_bytes": ((U64, INT), (COUNTS, MATCH)),
    "msj_stage2_prep_workspace_bytes": ((U64, U64, INT), (COUNTS, COUNTS, MATCH)),
    "msj_documents_workspace_bytes": ((U64,), (COUNTS,)),
    "msj_number_values_workspace_bytes": ((U64, U64), (COUNTS, COUNTS)),
    "msj_validate_workspace_bytes": ((U64, U64), (COUNTS, COUNTS)),
    "msj_tape_workspace_bytes": ((U64, U64), (COUNTS, COUNTS)),
    "msj_validate_documents_workspace_bytes": ((U64, U64, U64), (COUNTS, COUNTS, ROWS)),
    "msj_tape_documents_workspace_bytes": ((U64, U64, U64), (COUNTS, COUNTS, ROWS)),
    "msj_select_documents_workspace_bytes": ((U64, U64, U64, U32), (COUNTS, COUNTS, ROWS, PATHS)),
    "msj_string_column_workspace_bytes": ((U64,), (ROWS,)),
    "msj_array_column_workspace_bytes": ((U64, U64), (COUNTS, ROWS)),
    "msj_select_elements_workspace_bytes": ((U64, U64, U32), (COUNTS, ROWS, PATHS)),
    "msj_array_elements_workspace_bytes": ((U64, U64), (COUNTS, ROWS)),
    "msj_object_entries_workspace_bytes": ((U64, U64), (COUNTS, ROWS)),
    "msj_raw_column_workspace_bytes": ((U64, U64, U32), (COUNTS, ROWS, RAW_FLAGS)),
    "msj_dictionary_workspace_bytes": ((U64,), (ROWS,)),
    "msj_filter_rows_workspace_bytes": ((U64,), (ROWS,)),  # (0: msj_take_rows_device's)
    "msj_cast_strings_workspace_bytes": ((U64,), (ROWS,)),
    "msj_aggregate_workspace_bytes": ((U64, U64, U32), (ROWS, ROWS, PATHS)),
    "msj_sort_rows_workspace_bytes": ((U64,), (ROWS,)),
}


def points(values):
    """Every combination; where three arguments are counts, each crosses its grid with the others at ANCHORS."""
    swept = [i for i, v in enumerate(values) if v in (COUNTS, ROWS)]
    if len(swept) < 3:
        return list(itertools.product(*values))
    out = []
    for i in swept:
        grids = [v if j == i or j not in swept else ANCHORS for j, v in enumerate(values)]
        out += [p for p in itertools.product(*grids) if p not in out]
    return out


def measure():
    from mojo_simdjson_amd import _lib

    lib = _lib.load()
    table = {}
    for name, (types, values) in CALLS.items():
        f = getattr(lib, name)
        f.restype, f.argtypes = U64, list(types)
        table[name] = [list(p) + [f(*p)] for p in points(values)]
    return table


@pytest.fixture(scope="module")
def now():
    return measure()


@pytest.fixture(scope="module")
def recorded():
    with open(TABLE) as f:
        return json.load(f)


def test_table_covers_every_call(recorded):
    assert len(CALLS) == 20 and sorted(recorded) == sorted(CALLS)
    for name, (_, values) in CALLS.items():
        assert [r[:-1] for r in recorded[name]] == [list(p) for p in points(values)], name


@pytest.mark.parametrize("name", sorted(CALLS))
def test_sizes_as_recorded(name, now, recorded):
    differ = [(got[:-1], got[-1], want[-1]) for got, want in zip(now[name], recorded[name]) if got != want]
    assert not differ, f"{name}: {len(differ)} sizes changed, (arguments, now, recorded): {differ[:5]}"


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    rows = ",\n".join(f' "{k}": {json.dumps(v, separators=(",", ":"))}' for k, v in measure().items())
    print("{\n" + rows + "\n}")
