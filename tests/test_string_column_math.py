"""CPU check of msj_string_column_device's arithmetic (mojo_simdjson_amd/csrc/string_column_math.h).

The definition in include/msj_stage1.h is restated in Python from its text alone (`definition` below): per document the
value tests/select_reference.py finds for the path -- a str gives its UTF-8, anything else is no string.  The host twin
(tests/string_column_math_host.cpp: the row test, the lengths, the code rule and the byte -> row mapping of the header,
serially) runs over the records of the select twin (tests/test_select_math.py); its offsets, validity bytes, bytes and
result must equal the definition's, fill and canary behind every array included.  The kernels that run the same header on
the device are covered by tests/test_string_column.py (-m gpu).
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import select_reference as ref
from tests import test_number_math as tnm
from tests import test_select_math as tsm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
FILL = 0x77
CANARY = 64         # bytes behind every array
ESCAPED = 2         # MSJ_SPAN_ESCAPED
LANE_BODY = 1024    # csrc/wave_unescape.h: kLaneBody

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/string_column_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libstring_column_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "string_column_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("scm_string_column", [ctypes.c_char_p, u64, vp, vp, vp, vp, u64, vp, u64, vp], None),
                            ("scm_row_of_byte", [vp, u32, u64], u32),
                            ("scm_row", [vp, u64, ctypes.POINTER(u64), ctypes.POINTER(u64)], ctypes.c_int),
                            ("scm_ulen", [ctypes.c_char_p, u64, vp], u64),
                            ("scm_is_long", [vp, u64, u32], ctypes.c_int)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def oracle():
    return helpers.load_oracle()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


@pytest.fixture(scope="module")
def vtwin():
    return tdm.load_twin()


@pytest.fixture(scope="module")
def stwin():
    return tsm.load_twin()


@pytest.fixture(scope="module")
def ctwin():
    return load_twin()


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Column:
    """What one call left: the result and the three arrays, each with its fill and 64 bytes of canary behind its capacity.
    data is None in the layout-only form."""

    def __init__(self, res, offsets, valid, data, capacity, bytes_capacity):
        self.res, self.offsets, self.valid, self.data = res, offsets, valid, data
        self.capacity, self.bytes_capacity = capacity, bytes_capacity

    def summary(self):
        r = self.res
        return (r.code, r.flags, r.n_rows, r.n_strings, r.n_escaped, r.total_bytes, r.n_other)

    def rows(self):
        """The rows as Python values: the bytes of a string, None for a row that is none"""
        D = int(self.res.n_rows)
        off = self.offsets[:D + 1].tolist()
        return [bytes(self.data[off[k]:off[k + 1]]) if self.valid[k] else None for k in range(D)]

    def untouched(self, rows, nbytes):
        """Offsets past `rows` (-1: none written at all), validity bytes at or past it, bytes at or past `nbytes`, and the
        canaries, are as they were filled"""
        ok = bool((self.offsets.view(np.uint8)[8 * (rows + 1):] == FILL).all()) and bool((self.valid[max(rows, 0):] == FILL).all())
        return ok and (self.data is None or bool((self.data[nbytes:] == FILL).all()))


def filled(capacity, bytes_capacity, layout_only=False):
    """-> (offsets uint64[capacity + 1 + 8], valid uint8[capacity + 64], bytes uint8[bytes_capacity + 64] or None)"""
    offsets = np.full(8 * (capacity + 1) + CANARY, FILL, dtype=np.uint8).view(np.uint64)
    valid = np.full(capacity + CANARY, FILL, dtype=np.uint8)
    data = None if layout_only else np.full(bytes_capacity + CANARY, FILL, dtype=np.uint8)
    return offsets, valid, data


def select_result(D, code=0, n_paths=1):
    return _lib.MsjSelectDocumentsResult(code, 0, D, n_paths, 0, 0, 0)


def twin_column(ctwin, data, records, D, length=None, sel_code=0, capacity=None, bytes_capacity=None, layout_only=False):
    """scm_string_column over `records` (FIELD_DTYPE, one path's column).  bytes_capacity None: what a layout-only first
    call reports.  -> Column"""
    length = len(data) if length is None else length
    capacity = D if capacity is None else capacity
    records = np.ascontiguousarray(records)
    sel = select_result(D, sel_code)
    if bytes_capacity is None and not layout_only:
        bytes_capacity = int(twin_column(ctwin, data, records, D, length, sel_code, capacity, layout_only=True).res.total_bytes)
    offsets, valid, out = filled(capacity, bytes_capacity or 0, layout_only)
    res = _lib.MsjStringColumnResult()
    ctwin.scm_string_column(data, length, records.ctypes.data, ctypes.byref(sel), offsets.ctypes.data, valid.ctypes.data, capacity,
                            out.ctypes.data if out is not None else None, 0 if layout_only else bytes_capacity, ctypes.byref(res))
    return Column(res, offsets, valid, out, capacity, 0 if layout_only else bytes_capacity)


def record(b, r, typ='"', flags=0, code=0, token=0):
    rec = np.zeros(1, dtype=FIELD_DTYPE)
    rec["bits"], rec["token"], rec["type"], rec["flags"], rec["code"] = b | (r << 32), token, ord(typ) if typ else 0, flags, code
    return rec


# ---- the definition ---------------------------------------------------------------------------------------------------------

def definition(values):
    """values: (code, Python value) per document, as tests/select_reference.py gives them for the path (a document with a
    verdict code: (its code, None)).  -> (offsets, valid, bytes, n_strings, n_other)"""
    offsets, valid, out, n_other = [0], [], bytearray(), 0
    for code, v in values:
        is_string = code == 0 and isinstance(v, str)
        if is_string:
            out += v.encode("utf-8", "surrogatepass")
        n_other += code == 0 and not is_string
        valid.append(int(is_string))
        offsets.append(len(out))
    return offsets, valid, bytes(out), sum(valid), n_other


def check_against_definition(col, values, records):
    """A Column with room for every row and every byte against the definition"""
    offsets, valid, out, n_strings, n_other = definition(values)
    D = len(values)
    n_escaped = sum(1 for k in range(D) if valid[k] and int(records[k]["flags"]) & ESCAPED)
    assert col.summary() == (0, 0, D, n_strings, n_escaped, len(out), n_other), col.summary()
    assert col.offsets[:D + 1].tolist() == offsets and col.valid[:D].tolist() == valid
    assert col.untouched(D, len(out))
    if col.data is not None:
        assert bytes(col.data[:len(out)]) == out
    return n_strings, n_escaped, n_other


def ndjson(values, key="s"):
    """One document {"<key>": value} per entry; an entry that is bytes is the document's text as it is"""
    import json

    return [v if isinstance(v, bytes) else json.dumps({key: v}, ensure_ascii=False, separators=(",", ":")).encode("utf-8") for v in values]


def column_of(oracle, nm, stwin, lines, pointer="/s", verdicts=None, sep=b"\n"):
    """The select twin's records of `pointer` over the stream of `lines` -> (data, WindowArrays, records[D], (code, value) per row)"""
    data = tdk.join(lines, sep)
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    assert w.D == len(lines)
    got = tsm.twin_select(stwin, w, [pointer], verdicts=verdicts)
    codes = [c for c, _ in verdicts] if verdicts is not None else None
    out = tsm.check_against_reference(w, got, [pointer], lines, codes=codes)
    return data, w, got.column(0)[:w.D].copy(), [out[(0, k)] for k in range(w.D)]


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_corpus_equals_definition(oracle, nm, stwin, ctwin):
    """Every path of every fourth stream of the select corpus, and of the pins: offsets, validity, bytes and the result are
    the definition's, with the bytes and in the layout-only form."""
    streams = [tsm.pin_stream()] + tsm.corpus()[::4]
    totals = [0, 0, 0]
    for j, (data, docs, pointers) in enumerate(streams):
        w = tdm.WindowArrays(oracle, nm, data, is_final=True)
        got = tsm.twin_select(stwin, w, pointers)
        out = tsm.check_against_reference(w, got, pointers, docs)
        for p in range(len(pointers)):
            records = got.column(p)[:w.D]
            values = [out[(p, k)] for k in range(w.D)]
            for layout_only in (False, True):
                col = twin_column(ctwin, data, records, w.D, layout_only=layout_only)
                counts = check_against_definition(col, values, records)
            totals = [a + b for a, b in zip(totals, counts)]
    assert totals[0] > 50 and totals[1] > 20 and totals[2] > 500, totals   # strings, escaped ones, other values


def test_pins(oracle, nm, vtwin, stwin, ctwin):
    """The cases read from the definition: the empty string, escapes with a surrogate pair, values that are no strings, a
    missing key, a document with a verdict code."""
    lines = [b'{"s":""}', b'{"s":"\\u0041\\ud83d\\ude00\\n"}', b'{"s":null}', b'{"s":7}', b'{"s":{}}', b'{"t":1}',
             b'{"s":"x","a":[1,tru]}', b'{"s":"plain"}', b'{"s":[1]}', b'{"s":true}', b'{"s":"a\\\\b\\/c\\"d"}', b'{"s":1.5}']
    data = tdk.join(lines, b"\n")
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    verdicts, _ = tdm.twin_documents(vtwin, w, 100)
    assert [c for c, _ in verdicts] == [0] * 6 + [tvm.T_ATOM] + [0] * 5
    _, _, records, values = column_of(oracle, nm, stwin, lines, verdicts=verdicts)
    col = twin_column(ctwin, data, records, w.D)
    check_against_definition(col, values, records)
    rows = col.rows()
    assert rows[0] == b"" and col.valid[0] == 1
    assert rows[1] == "A\U0001F600\n".encode() and len(rows[1]) == 6
    assert rows[2:7] == [None] * 5 and rows[7] == b"plain" and rows[8:10] == [None] * 2 and rows[10] == b'a\\b/c"d' and rows[11] is None
    # null, 7, {}, [1], true and 1.5 are counted as other; the missing key and the invalid document are not
    assert col.summary() == (0, 0, 12, 4, 2, 6 + 5 + 7, 6)
    assert [int(r["code"]) for r in records[5:7]] == [ref.NO_SUCH_FIELD, tvm.T_ATOM]


def test_spans_against_the_window(ctwin):
    """Hand-made records: a span that ends at len is a string, one that ends at len + 1 is none and is never read; the
    largest span a record can name does not overflow."""
    data = b'0123456789'
    b, r = ctypes.c_uint64(), ctypes.c_uint64()
    at = lambda rec, length=len(data): (ctwin.scm_row(rec.ctypes.data, length, ctypes.byref(b), ctypes.byref(r)), b.value, r.value)
    assert at(record(4, 6)) == (1, 4, 6) and at(record(4, 7)) == (4, 0, 0) and at(record(10, 0)) == (1, 10, 0) and at(record(11, 0)) == (4, 0, 0)
    assert at(record(0xFFFFFFFF, 0xFFFFFFFF)) == (4, 0, 0) and at(record(0xFFFFFFFF, 0xFFFFFFFF), 1 << 33) == (1, 0xFFFFFFFF, 0xFFFFFFFF)
    assert at(record(2, 3, flags=ESCAPED)) == (3, 2, 3) and at(record(2, 9, flags=ESCAPED)) == (4, 0, 0)
    assert at(record(0, 0, typ="l")) == (4, 0, 0) and at(record(0, 0, typ="", code=20)) == (0, 0, 0) and at(record(2, 3, code=17)) == (0, 0, 0)
    assert ctwin.scm_is_long(record(0, LANE_BODY + 1, flags=ESCAPED).ctypes.data, 1 << 20, LANE_BODY) == 1
    assert ctwin.scm_is_long(record(0, LANE_BODY, flags=ESCAPED).ctypes.data, 1 << 20, LANE_BODY) == 0
    assert ctwin.scm_is_long(record(0, LANE_BODY + 1).ctypes.data, 1 << 20, LANE_BODY) == 0
    records = np.concatenate([record(0, 3), record(4, 7), record(4, 6), record(9, 2), record(9, 1), record(3, 0)])
    col = twin_column(ctwin, data, records, 6)
    assert col.rows() == [b"012", None, b"456789", None, b"9", b""] and col.summary() == (0, 0, 6, 4, 0, 10, 2)
    # the same records against a window one byte shorter: the two spans that end at 10 are no strings any more
    short = twin_column(ctwin, data, records, 6, length=9)
    assert short.rows() == [b"012", None, None, None, None, b""] and short.summary() == (0, 0, 6, 2, 0, 3, 4)


def test_capacities(oracle, nm, stwin, ctwin):
    """bytes_capacity one short and 0: MSJ_CAPACITY, offsets and validity complete, total_bytes exact, no byte past the
    capacity.  d_bytes NULL: the layout alone, code 0.  D > capacity: MSJ_CAPACITY and nothing else written.  A select
    result with a code: that code, a zero result, nothing written."""
    lines = ndjson(["abc", "", 5, "d\ne€", "tail"])
    data, w, records, values = column_of(oracle, nm, stwin, lines)
    full = twin_column(ctwin, data, records, w.D)
    check_against_definition(full, values, records)
    total = int(full.res.total_bytes)
    assert total == 3 + 0 + 6 + 4 and full.res.n_escaped == 1
    for cap in (total - 1, 3, 0):
        col = twin_column(ctwin, data, records, w.D, bytes_capacity=cap)
        assert col.summary() == (MSJ_CAPACITY,) + full.summary()[1:]
        assert np.array_equal(col.offsets, full.offsets) and np.array_equal(col.valid, full.valid)
        assert bytes(col.data[:cap]) == bytes(full.data[:cap]) and col.untouched(w.D, cap)
    layout = twin_column(ctwin, data, records, w.D, layout_only=True)
    assert layout.summary() == full.summary() and np.array_equal(layout.offsets, full.offsets) and np.array_equal(layout.valid, full.valid)
    roomy = twin_column(ctwin, data, records, w.D, capacity=w.D + 3, bytes_capacity=total + 9)
    assert roomy.summary() == full.summary() and roomy.untouched(w.D, total) and roomy.rows() == full.rows()
    over = twin_column(ctwin, data, records, w.D, capacity=w.D - 1, bytes_capacity=total)
    assert over.summary() == (MSJ_CAPACITY, 0, w.D, 0, 0, 0, 0) and over.untouched(-1, 0)
    for code in (MSJ_CAPACITY, 24):
        skipped = twin_column(ctwin, data, records, w.D, sel_code=code, bytes_capacity=total)
        assert skipped.summary() == (code, 0, 0, 0, 0, 0, 0) and skipped.untouched(-1, 0)
    empty = twin_column(ctwin, data, records, 0, capacity=2, bytes_capacity=4)
    assert empty.summary() == (0,) * 7 and empty.offsets[0] == 0 and empty.untouched(0, 0)


def test_long_and_escaped_lengths(oracle, nm, stwin, ctwin):
    """Escaped bodies of kLaneBody and kLaneBody + 1 raw bytes and one that is all \\u00e9 (a third of its raw length in
    the output), between plain ones."""
    values = ["a" * (LANE_BODY - 2) + "\n", "b" * (LANE_BODY - 1) + "\n", "é" * 300, "x" * 3000, ""]
    lines = ndjson(values[:2]) + [b'{"s":"' + b"\\u00e9" * 300 + b'"}'] + ndjson(values[3:])
    data, w, records, rows = column_of(oracle, nm, stwin, lines)
    assert [int(x) >> 32 for x in records["bits"]] == [LANE_BODY, LANE_BODY + 1, 1800, 3000, 0]
    assert [int(x) & ESCAPED for x in records["flags"]] == [2, 2, 2, 0, 0]
    col = twin_column(ctwin, data, records, w.D)
    check_against_definition(col, rows, records)
    assert [len(x) for x in col.rows()] == [LANE_BODY - 1, LANE_BODY, 600, 3000, 0]
    assert [ctwin.scm_ulen(data, len(data), records[k:k + 1].ctypes.data) for k in range(5)] == [LANE_BODY - 1, LANE_BODY, 600, 3000, 0]


def test_byte_to_row_mapping(ctwin):
    """row_of_byte: the last row whose offset is <= the position.  Runs of equal offsets (empty rows) at the front, in the
    middle and at the end never capture a byte; every position of every list against a linear search."""
    lists = [[0, 5], [0, 0, 0, 4, 9], [0, 3, 3, 3, 3, 8], [0, 2, 7, 7, 7], [0, 0, 1, 1, 2, 2, 2, 3], [5, 5, 9, 9, 1000, 1000],
             [0] + [k // 3 for k in range(1, 257)], [1 << 40, (1 << 40) + 1, (1 << 40) + 1, (1 << 40) + 70000]]
    rng = np.random.default_rng(7)
    lists.append(np.concatenate([[0], np.cumsum(rng.integers(0, 3, 256))]).tolist())
    for off in lists:
        a = np.array(off, dtype=np.uint64)
        n = len(off) - 1
        positions = range(off[0], off[-1]) if off[-1] - off[0] < 5000 else [off[0], off[1] - 1, off[1], off[-1] - 1]
        for pos in positions:
            want = max(k for k in range(n) if off[k] <= pos)
            got = ctwin.scm_row_of_byte(a.ctypes.data, n, pos)
            assert got == want and off[got] <= pos < off[got + 1], (off[:8], pos, got, want)
