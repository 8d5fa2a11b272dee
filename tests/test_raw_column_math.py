"""CPU check of msj_raw_column_device's arithmetic (mojo_simdjson_amd/csrc/raw_column_math.h).

The host twin (tests/raw_column_math_host.cpp: the token texts, the row test, the lengths and the two searches of the
header, serially) runs over records of the select twin (tests/test_select_math.py) and over hand-made ones.  The yardstick
is Python and knows nothing of the header: a valid row's verbatim text is what json's raw_decode consumes from the value's
first byte; the compact text equals the verbatim one on minified input, decodes to the same value (pairs kept) on
pretty-printed input, and under the stage-1 oracle has one structural per token of the value, each starting where the text
of the one in front ended (the texts measured by `token_len` below, from the bytes alone).  The kernels that run the same
header on the device are covered by tests/test_raw_column.py (-m gpu); records and arrays from anywhere by
tests/test_raw_column_sanitizers.py.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib, synth
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import select_reference as ref
from tests import test_number_math as tnm
from tests import test_select_math as tsm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
COMPACT = 1         # MSJ_RAW_COMPACT
FILL = 0x77
CANARY = 64         # bytes behind every array
LONG_DIGITS = 1025  # a number of more characters than 1 024 has MSJ_SPAN_LONG and no d_end

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/raw_column_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libraw_column_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "raw_column_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("rcm_raw_column", [ctypes.c_char_p, u64, vp, u64, vp, vp, vp, vp, vp, vp, vp, u64, vp, u64, u32, vp], None),
                            ("rcm_text_len", [ctypes.c_char_p, u64, vp, u64, vp, vp, vp, u64], u64),
                            ("rcm_row", [vp, u64, ctypes.POINTER(u32), ctypes.POINTER(u32)], ctypes.c_int),
                            ("rcm_token_of_byte", [vp, u64, u64, u64], u64)):
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
def rtwin():
    return load_twin()


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Column:
    """What one call left: the result and the three arrays, each with its fill and 64 bytes of canary behind its capacity.
    data is None in the layout-only form."""

    def __init__(self, res, offsets, valid, data, capacity, bytes_capacity, flags):
        self.res, self.offsets, self.valid, self.data = res, offsets, valid, data
        self.capacity, self.bytes_capacity, self.flags = capacity, bytes_capacity, flags

    def summary(self):
        r = self.res
        return (r.code, r.flags, r.n_rows, r.n_values, r.n_containers, r.total_bytes, r.n_other)

    def rows(self):
        """The rows as Python values: the bytes of a value, None for a row that is none"""
        R = int(self.res.n_rows)
        off = self.offsets[:R + 1].tolist()
        return [bytes(self.data[off[k]:off[k + 1]]) if self.valid[k] else None for k in range(R)]

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


def select_result(R, code=0):
    return _lib.MsjSelectDocumentsResult(code, 0, R, 1, 0, 0, 0)


class Arrays:
    """The arrays the call reads, each exactly n long (a WindowArrays' or the device's, downloaded)"""

    def __init__(self, data, idx, typ, end, flags, length=None):
        self.data, self.length = bytes(data), len(data) if length is None else length
        self.idx, self.end = np.ascontiguousarray(idx, dtype=np.uint32), np.ascontiguousarray(end, dtype=np.uint32)
        self.typ, self.flags = np.ascontiguousarray(typ, dtype=np.uint8), np.ascontiguousarray(flags, dtype=np.uint8)
        self.n = int(self.idx.size)


def arrays_of(w):
    return Arrays(w.data, w.idx, w.typ, w.end, w.flags)


def twin_raw(rtwin, a, records, R=None, compact=False, sel_code=0, capacity=None, bytes_capacity=None, layout_only=False):
    """rcm_raw_column over `records` (FIELD_DTYPE) and the Arrays a.  bytes_capacity None: what a layout-only first call
    reports.  -> Column"""
    records = np.ascontiguousarray(records)
    R = len(records) if R is None else R
    capacity = R if capacity is None else capacity
    flags = COMPACT if compact else 0
    if bytes_capacity is None and not layout_only:
        bytes_capacity = int(twin_raw(rtwin, a, records, R, compact, sel_code, capacity, layout_only=True).res.total_bytes)
    offsets, valid, out = filled(capacity, bytes_capacity or 0, layout_only)
    res = _lib.MsjRawColumnResult()
    sel = select_result(R, sel_code)
    rtwin.rcm_raw_column(a.data, a.length, a.idx.ctypes.data, a.n, a.typ.ctypes.data, a.end.ctypes.data, a.flags.ctypes.data,
                         records.ctypes.data, ctypes.byref(sel), offsets.ctypes.data, valid.ctypes.data, capacity,
                         out.ctypes.data if out is not None else None, 0 if layout_only else bytes_capacity, flags, ctypes.byref(res))
    return Column(res, offsets, valid, out, capacity, 0 if layout_only else bytes_capacity, flags)


def record(token, typ="l", bits=0, flags=0, code=0):
    rec = np.zeros(1, dtype=FIELD_DTYPE)
    rec["bits"], rec["token"], rec["type"], rec["flags"], rec["code"] = bits, token, ord(typ) if typ else 0, flags, code
    return rec


def value_records(w):
    """A hand-made record for every token of the window that starts a value (a key is a string value too): containers with
    their partner in bits"""
    out = []
    for i in range(w.n):
        c = chr(int(w.typ[i]))
        if c in "{[":
            out.append(record(i, c, bits=int(w.match[i])))
        elif c not in "}],:":
            out.append(record(i, '"' if c == '"' else "l"))
    return np.concatenate(out)


def select_records(stwin, w, pointer, verdicts=None):
    return tsm.twin_select(stwin, w, [pointer], verdicts=verdicts).column(0)[:w.D].copy()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------

_NUMBER = re.compile(rb"-?[0-9]+(\.[0-9]+)?([eE][+-]?[0-9]+)?")
_DECODER = json.JSONDecoder()


def token_len(text, s):
    """The length of the token text that starts at text[s], from the bytes alone"""
    c = text[s:s + 1]
    if c == b'"':
        j = s + 1
        while text[j] != 0x22:
            j += 2 if text[j] == 0x5C else 1
        return j + 1 - s
    if c in b"-0123456789":
        return _NUMBER.match(text, s).end() - s
    return {b"t": 4, b"n": 4, b"f": 5}.get(c, 1)


def expect_verbatim(data, idx, rec):
    """The bytes json consumes from the value's first byte on (one char per byte: offsets stay byte offsets)"""
    s = int(idx[int(rec["token"])])
    _, e = _DECODER.raw_decode(data.decode("latin-1"), s)
    return data[s:e]


def check_verbatim(col, a, records):
    """Every row of a verbatim Column with room for everything against the yardstick; records with a code are no rows"""
    rows = col.rows()
    assert len(rows) == len(records)
    n_values = n_containers = 0
    for k, rec in enumerate(records):
        if rec["code"] != 0:
            assert rows[k] is None, k
            continue
        assert rows[k] == expect_verbatim(a.data, a.idx, rec), (k, rows[k][:60])
        n_values += 1
        n_containers += chr(int(rec["type"])) in "{["
    total = sum(len(r) for r in rows if r is not None)
    assert col.summary() == (0, 0, len(records), n_values, n_containers, total, 0), col.summary()
    assert col.offsets[len(records)] == total and col.untouched(len(records), total)
    return rows


def check_compact(oracle, rows_c, rows_v, records):
    """Compact rows against verbatim ones: the same value with every pair kept, and under the stage-1 oracle one structural
    per token of the value, each where the text of the one in front ended, the last text ending the row"""
    pairs = lambda b: json.loads(b.decode("utf-8", "surrogatepass"), object_pairs_hook=list)
    for k, rec in enumerate(records):
        c, v = rows_c[k], rows_v[k]
        assert (c is None) == (v is None), k
        if c is None:
            continue
        assert pairs(c) == pairs(v), (k, c[:80])
        idx, _ = helpers.oracle_window(oracle.msj_oracle_stage1, c)
        is_box = chr(int(rec["type"])) in "{["
        want_tokens = int(rec["bits"]) - int(rec["token"]) + 1 if is_box else 1
        assert idx.size == want_tokens, (k, idx.size, want_tokens, c[:80])
        at = 0
        for s in idx.tolist():
            assert s == at, (k, s, at, c[:80])
            at = s + token_len(c, s)
        assert at == len(c), (k, at, len(c))


# ---- tests ------------------------------------------------------------------------------------------------------------------

PIN_LINES = [b'{"s":"str"}', b'{"s":12}', b'{"s":-2.5e3}', b'{"s":true}', b'{"s":false}', b'{"s":null}', b'{"s":""}',
             b'{"s":"a\\n\\u00e9\\"q\\\\"}', b'{"s":"x , ] } : [ {  \\t y"}', b'{"s":{}}', b'{"s":[]}',
             b'{"s":{"a":[{"b":[{"c":[1,"2",null]}]}],"d":{}}}', b'{"t":1}', b'[1,2]', b'{"s":"x","a":[1,tru]}', b'{"s":[1,[2,[3,[4,[5]]]]]}',
             b'{"a":0,"s":0.5}']


def test_pins(oracle, nm, vtwin, stwin, rtwin):
    """Every scalar kind, "", escapes, a string that holds structural characters and blanks, {} and [], nesting to depth
    5, a missing key, an INCORRECT_TYPE row, a document with a verdict code; the root through ""; then the same rows in
    descending order with two of them named twice.  Verbatim and compact agree on minified input."""
    data = tdk.join(PIN_LINES, b"\n")
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    a = arrays_of(w)
    verdicts, _ = tdm.twin_documents(vtwin, w, 100)
    assert [c for c, _ in verdicts] == [0] * 14 + [tvm.T_ATOM] + [0] * 2
    for pointer in ("/s", ""):
        records = select_records(stwin, w, pointer, verdicts)
        if pointer == "/s":
            assert [int(r["code"]) for r in records[12:15]] == [ref.NO_SUCH_FIELD, ref.INCORRECT_TYPE, tvm.T_ATOM]
        for recs in (records, np.concatenate([records[::-1], records[11:12], records[11:12], records[0:1]])):
            col = twin_raw(rtwin, a, recs)
            rows = check_verbatim(col, a, recs)
            compact = twin_raw(rtwin, a, recs, compact=True)
            assert compact.rows() == rows and compact.summary() == (0, COMPACT) + col.summary()[2:]
            check_compact(oracle, compact.rows(), rows, recs)
            layout = twin_raw(rtwin, a, recs, layout_only=True)
            assert layout.summary() == col.summary() and np.array_equal(layout.offsets, col.offsets) and np.array_equal(layout.valid, col.valid)
        if pointer == "/s":
            want = [x[5:-1] for x in PIN_LINES]
            assert rows[:len(PIN_LINES)][::-1][:12] == want[:12] and rows[-3] == rows[-2] == want[11] and rows[-1] == b'"str"'
            assert rows[len(PIN_LINES) - 1 - 8] == b'"x , ] } : [ {  \\t y"' and rows[len(PIN_LINES) - 1 - 15] == b"[1,[2,[3,[4,[5]]]]]"
        else:
            assert rows[:len(PIN_LINES)][::-1] == [None if k == 14 else x for k, x in enumerate(PIN_LINES)]


def test_window_ends(oracle, nm, stwin, rtwin):
    """A value that is the last token of the window and is followed by len directly: a number, a string, an atom and a LONG
    number as the last document's root; and a window whose last token is a closing bracket, followed by a blank."""
    for tail in (b"12", b'"zz"', b"null", b"7" * LONG_DIGITS, b'{"s":[1]} '):
        data = b'{"s":1}\n' + tail
        w = tdm.WindowArrays(oracle, nm, data, is_final=True)
        a = arrays_of(w)
        for pointer in ("", "/s"):
            records = select_records(stwin, w, pointer)
            rows = check_verbatim(twin_raw(rtwin, a, records), a, records)
            assert twin_raw(rtwin, a, records, compact=True).rows() == rows
        assert rows[0] == b"1"
    records = select_records(stwin, w, "")
    assert twin_raw(rtwin, a, records).rows() == [b'{"s":1}', b'{"s":[1]}']


def test_long_numbers(oracle, nm, stwin, rtwin):
    """A number of 1 025 characters (MSJ_SPAN_LONG: no d_end) followed by 0, 1 and 70 blanks, as a field, as an array's
    last element and as the root; every kind of blank.  The compact text drops the blanks, the verbatim text of the
    enclosing container keeps them."""
    big = b"1" + b"0" * (LONG_DIGITS - 1)
    for blanks in (b"", b" ", b" \t\r\n" * 17 + b"  "):
        lines = [b'{"s":' + big + blanks + b'}', b'{"s":[1,' + big + blanks + b']}', big + blanks, b'{"s":-' + big[:-1] + blanks + b',"t":2}']
        data = tdk.join(lines, b"\n")
        w = tdm.WindowArrays(oracle, nm, data, is_final=True)
        assert w.D == 4 and int(((w.flags & 128) != 0).sum()) == 4
        a = arrays_of(w)
        for pointer in ("/s", ""):
            records = select_records(stwin, w, pointer)
            rows = check_verbatim(twin_raw(rtwin, a, records), a, records)
            crows = twin_raw(rtwin, a, records, compact=True).rows()
            check_compact(oracle, crows, rows, records)
            assert all(c is None or c == bytes(v).replace(blanks, b"") or not blanks for c, v in zip(crows, rows))
        assert rows[2] == big and crows[0] == b'{"s":' + big + b"}"


@pytest.mark.parametrize("name", ["minified", "pretty2", "pretty4", "pretty_tab_crlf"])
def test_every_value_of_a_synthetic_document(oracle, nm, rtwin, name):
    """Every value of ~12 KiB of the synthetic workloads as a row -- the root, every container, every key and scalar:
    verbatim against json, compact equal to verbatim on the minified one and, on the pretty-printed ones (indent 2, 4, tab
    with CRLF), the same values with one structural per token and no blank between them."""
    data = synth.workload(name, 12 << 10).tobytes()
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    a = arrays_of(w)
    records = value_records(w)
    assert len(records) > 300 and records[0]["token"] == 0 and records[0]["bits"] == w.n - 1
    col = twin_raw(rtwin, a, records)
    rows = check_verbatim(col, a, records)
    compact = twin_raw(rtwin, a, records, compact=True)
    assert compact.summary()[2:5] == col.summary()[2:5]
    if name == "minified":
        assert compact.rows() == rows
    else:
        assert compact.res.total_bytes < col.res.total_bytes
        check_compact(oracle, compact.rows(), rows, records)
        assert not re.search(rb"[\r\n\t]", compact.rows()[0])


def test_capacities(oracle, nm, stwin, rtwin):
    """bytes_capacity one short and 0: MSJ_CAPACITY, offsets and validity complete, total_bytes exact, no byte past the
    capacity.  R > capacity: MSJ_CAPACITY and nothing else written.  A select result with a code: that code, a zero result
    with the flags kept.  No row: offsets[0] and a zero result."""
    data = tdk.join(PIN_LINES, b"\n")
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    a = arrays_of(w)
    records = select_records(stwin, w, "/s")
    for compact in (False, True):
        f = COMPACT if compact else 0
        full = twin_raw(rtwin, a, records, compact=compact)
        total = int(full.res.total_bytes)
        for cap in (total - 1, 3, 0):
            col = twin_raw(rtwin, a, records, compact=compact, bytes_capacity=cap)
            assert col.summary() == (MSJ_CAPACITY,) + full.summary()[1:]
            assert np.array_equal(col.offsets, full.offsets) and np.array_equal(col.valid, full.valid)
            assert bytes(col.data[:cap]) == bytes(full.data[:cap]) and col.untouched(w.D, cap)
        roomy = twin_raw(rtwin, a, records, compact=compact, capacity=w.D + 3, bytes_capacity=total + 9)
        assert roomy.summary() == full.summary() and roomy.untouched(w.D, total) and roomy.rows() == full.rows()
        over = twin_raw(rtwin, a, records, compact=compact, capacity=w.D - 1, bytes_capacity=total)
        assert over.summary() == (MSJ_CAPACITY, f, w.D, 0, 0, 0, 0) and over.untouched(-1, 0)
        for code in (MSJ_CAPACITY, 24):
            skipped = twin_raw(rtwin, a, records, compact=compact, sel_code=code, bytes_capacity=total)
            assert skipped.summary() == (code, f, 0, 0, 0, 0, 0) and skipped.untouched(-1, 0)
        empty = twin_raw(rtwin, a, records, R=0, compact=compact, capacity=2, bytes_capacity=4)
        assert empty.summary() == (0, f, 0, 0, 0, 0, 0) and empty.offsets[0] == 0 and empty.untouched(0, 0)


def test_row_test_and_searches(oracle, nm, rtwin):
    """Hand-made records against the row test: a token at n, a container whose partner is the token itself, in front of it
    or at n is counted as other and owns nothing; a record with a code is in no count.  token_of_byte: the last token whose
    sum is <= the byte, tokens without text never capture one."""
    data = b'{"a":[1,2],"b":{}}'
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    a = arrays_of(w)
    n = w.n
    token, last = ctypes.c_uint32(), ctypes.c_uint32()
    at = lambda rec: (rtwin.rcm_row(rec.ctypes.data, n, ctypes.byref(token), ctypes.byref(last)), token.value, last.value)
    assert at(record(0, "{", bits=n - 1)) == (3, 0, n - 1) and at(record(0, "{", bits=n)) == (4, 0, 0) and at(record(3, "[", bits=3)) == (4, 0, 0)
    assert at(record(3, "[", bits=2)) == (4, 0, 0) and at(record(n - 1, "l")) == (1, n - 1, n - 1) and at(record(n, "l")) == (4, 0, 0)
    assert at(record(0xFFFFFFFF, "", code=20)) == (0, 0, 0) and at(record(2, "{", bits=1 << 40)) == (4, 0, 0) and at(record(1, '"', bits=1 << 40)) == (1, 1, 1)
    records = np.concatenate([record(0, "{", bits=n - 1), record(n, "l"), record(3, "[", bits=7), record(3, "[", bits=3), record(0, "", code=17),
                              record(1, '"'), record(n - 1, "l")])
    col = twin_raw(rtwin, a, records)
    assert col.rows() == [data, None, b"[1,2]", None, None, b'"a"', b"}"] and col.summary() == (0, 0, 7, 4, 2, len(data) + 5 + 3 + 1, 2)
    for sums in ([0, 1, 4, 4, 4, 9, 10], [0, 0, 0, 3], [5, 5, 6, 6, 8], [0, 1 << 40, (1 << 40) + 2, (1 << 41)]):
        p = np.array(sums, dtype=np.uint64)
        lo, hi = 0, len(sums) - 2
        for q in set(range(sums[lo], min(sums[hi + 1], sums[lo] + 40))) | {sums[hi + 1] - 1}:
            want = max(i for i in range(lo, hi + 1) if sums[i] <= q)
            got = rtwin.rcm_token_of_byte(p.ctypes.data, lo, hi, q)
            assert got == want and sums[got] <= q < sums[got + 1], (sums, q, got, want)
