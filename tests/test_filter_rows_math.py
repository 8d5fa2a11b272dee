"""CPU check of the arithmetic of msj_predicates_create, msj_filter_rows_device and msj_take_rows_device
(mojo_simdjson_amd/csrc/filter_rows_math.h).

The host twin (tests/filter_rows_math_host.cpp: the header's compile step, exact number compare, string compares, row verdict
and offset gather, serially) runs over hand-made records.  The yardstick is Python and knows nothing of the header: Python's
own ``int`` / ``float`` comparison, which is exact; for strings ``==`` and ``bytes.startswith`` over the bytes the
string-column twin (tests/string_column_math_host.cpp) writes for the record, which is the definition of a row's value;
``all`` / ``any`` over the predicates; ``sum(keep[:min(offset, R)])`` for a re-based list offset; a Python loop for the
take.  Every array at its exact size with the fill and 64 canary bytes behind each capacity.  The kernels that run the same
header on the device are covered by tests/test_filter_rows.py (-m gpu); arrays from anywhere by
tests/test_filter_rows_sanitizers.py.
"""
import ctypes
import math
import os
import struct
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import test_string_column_math as tcm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
FILL = 0x77
CANARY = 64
ESCAPED, NO_BITS = 2, 64
HOLDS, MET_CODE, MET_NO_BITS = 1, 2, 4   # csrc/filter_rows_math.h: what one predicate says of one record
FOUND, TYPE, NUM_EQ, NUM_LT, NUM_LE, NUM_GT, NUM_GE, STR_EQ, STR_PREFIX = range(9)
NUM_OPS = (NUM_EQ, NUM_LT, NUM_LE, NUM_GT, NUM_GE)
NOT, DOUBLE, ANY = 1, 2, 1
MISSING = (0, 0xFFFFFFFF, 0, 0, 20)      # the record of an index out of range: bits, token, type, flags, code

_twin = None


def load_twin():
    """The host twin of the calls (g++ build of tests/filter_rows_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libfilter_rows_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "filter_rows_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, cint = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    for name, args, res in (("frm_predicates_bytes", [], u64),
                            ("frm_compile", [vp, u32, u32, vp], cint),
                            ("frm_cmp_int_double", [ctypes.c_int64, ctypes.c_double], cint),
                            ("frm_starts_with", [ctypes.c_char_p, u64, u64, u64, cint, ctypes.c_char_p, u32], cint),
                            ("frm_eval", [vp, u32, vp, ctypes.c_char_p, u64], u32),
                            ("frm_filter_rows", [vp, ctypes.c_char_p, u64, vp, u64, u32, vp, vp, vp, u64, vp, u64, vp, vp, vp, vp], cint),
                            ("frm_take_rows", [vp, vp, vp, u64, u32, vp, vp, u64, u64, vp, vp], None)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def ftwin():
    return load_twin()


@pytest.fixture(scope="module")
def ctwin():
    return tcm.load_twin()


# ---- predicates -------------------------------------------------------------------------------------------------------------

def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


class Spec:
    """One predicate as the tests write it: column, op, operand (int, float, bytes, a TYPE mask, or None), negated"""

    def __init__(self, column, op, operand=None, neg=False):
        self.column, self.op, self.operand, self.neg = column, op, operand, neg

    def c_struct(self, keep_alive):
        flags, bits, n, ptr = (NOT if self.neg else 0), 0, 0, None
        if self.op in NUM_OPS and isinstance(self.operand, float):
            flags |= DOUBLE
            bits = double_bits(self.operand)
        elif self.op in NUM_OPS or self.op == TYPE:
            bits = int(self.operand) & 0xFFFFFFFFFFFFFFFF
        elif self.op in (STR_EQ, STR_PREFIX):
            buf = ctypes.create_string_buffer(bytes(self.operand), max(len(self.operand), 1))
            keep_alive.append(buf)
            n, ptr = len(self.operand), ctypes.addressof(buf)
        return _lib.MsjPredicate(self.column, self.op, flags, n, bits, ptr)


def spec_table(specs):
    """-> (ctypes array of msj_predicate, what keeps its operand bytes alive)"""
    alive = []
    table = (_lib.MsjPredicate * max(len(specs), 1))(*[s.c_struct(alive) for s in specs])
    return table, alive


def compile_specs(ftwin, specs, any_=False):
    """The compiled predicates as the host twin keeps them -> a ctypes buffer (asserts the compile step takes them)"""
    table, alive = spec_table(specs)
    blob = ctypes.create_string_buffer(ftwin.frm_predicates_bytes())
    assert ftwin.frm_compile(table, len(specs), ANY if any_ else 0, blob) == 0
    return blob


# ---- records ----------------------------------------------------------------------------------------------------------------

def rec(bits=0, typ=None, flags=0, code=0, token=0):
    r = np.zeros(1, dtype=FIELD_DTYPE)
    r["bits"], r["token"], r["type"], r["flags"], r["code"] = bits & 0xFFFFFFFFFFFFFFFF, token, ord(typ) if typ else 0, flags, code
    return r


def int_rec(i):
    return rec(i, "l")


def double_rec(x):
    return rec(double_bits(x), "d")


def error_rec(code):
    return rec(0, None, 0, code, 0xFFFFFFFF)


def string_rec(b, r, escaped=False):
    return rec(b | (r << 32), '"', ESCAPED if escaped else 0)


def string_value(ctwin, data, length, record):
    """The bytes msj_string_column_device would write for the record -- by the string-column twin -- or None for a row that
    is no string"""
    col = tcm.twin_column(ctwin, data, record.reshape(1), 1, length=length)
    return col.rows()[0]


# ---- the yardstick ----------------------------------------------------------------------------------------------------------

def number_of(record):
    """The record's number as a Python int or float, or None"""
    if int(record["code"]) != 0 or chr(int(record["type"])) not in "ld" or int(record["flags"]) & NO_BITS:
        return None
    bits = int(record["bits"])
    if chr(int(record["type"])) == "l":
        return bits - (1 << 64) if bits >> 63 else bits
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def py_pred(spec, record, value):
    """(holds, met) of one predicate on one record, in Python; value: the row's string bytes or None"""
    code, typ, flags = int(record["code"]), int(record["type"]), int(record["flags"])
    met = MET_CODE if code else 0
    if spec.op == FOUND:
        holds = code == 0
    elif spec.op == TYPE:
        holds = code == 0 and bool(_lib.TYPE_BITS.get(chr(typ), 0) & spec.operand)
    elif spec.op in NUM_OPS:
        x = number_of(record)
        if code == 0 and chr(typ) in "ld" and flags & NO_BITS:
            met |= MET_NO_BITS
        y = spec.operand
        holds = x is not None and {NUM_EQ: x == y, NUM_LT: x < y, NUM_LE: x <= y, NUM_GT: x > y, NUM_GE: x >= y}[spec.op]
    elif spec.op == STR_EQ:
        holds = value is not None and value == spec.operand
    else:
        holds = value is not None and value.startswith(spec.operand)
    return bool(holds) != spec.neg, met


def py_filter(specs, any_, columns, values, R, list_offsets=None, P=None):
    """columns[c][k] records, values[c][k] string bytes or None -> (keep, kept, n_no_bits, n_missing, list_out)"""
    keep, n_no_bits, n_missing = [], 0, 0
    for k in range(R):
        said = [py_pred(s, columns[s.column][k], values[s.column][k]) for s in specs]
        holds = [h for h, _ in said]
        met = 0
        for _, m in said:
            met |= m
        keep.append(int(any(holds) if any_ else all(holds)))
        n_no_bits += bool(met & MET_NO_BITS)
        n_missing += bool(met & MET_CODE)
    kept = [k for k in range(R) if keep[k]]
    out = None
    if list_offsets is not None:
        out = [sum(keep[:min(int(list_offsets[r]), R)]) for r in range(P + 1)]
    return keep, kept, n_no_bits, n_missing, out


# ---- the twin's calls -------------------------------------------------------------------------------------------------------

class Filtered:
    """What one filter call left, every array with its fill and canary"""

    def __init__(self, rc, res, keep, kept, list_out, kept_select):
        self.rc, self.res, self.keep, self.kept, self.list_out, self.kept_select = rc, res, keep, kept, list_out, kept_select

    def summary(self):
        r = self.res
        return (r.code, r.flags, r.n_rows, r.n_kept, r.n_no_bits, r.n_missing, r.reserved)

    def select_summary(self):
        s = self.kept_select
        return (s.code, s.flags, s.n_documents, s.n_paths, s.n_found, s.n_no_bits, s.reserved)


def filled_filter(capacity, mask_only, list_rows):
    keep = np.full(capacity + CANARY, FILL, dtype=np.uint8)
    kept = None if mask_only else np.full(4 * capacity + CANARY, FILL, dtype=np.uint8).view(np.uint32)
    list_out = None if list_rows is None else np.full(8 * (list_rows + 1) + CANARY, FILL, dtype=np.uint8).view(np.uint64)
    return keep, kept, list_out


def twin_filter(ftwin, blob, data, length, fields, stride, n_columns, sel, capacity, mask_only=False, list_offsets=None, list_rows=None,
                list_n_rows=None):
    """frm_filter_rows.  fields: FIELD_DTYPE[n_columns * stride] at its exact size; sel: MsjSelectDocumentsResult"""
    fields = np.ascontiguousarray(fields)
    keep, kept, list_out = filled_filter(capacity, mask_only, list_rows if list_offsets is not None else None)
    res, ksel = _lib.MsjFilterRowsResult(), _lib.MsjSelectDocumentsResult()
    n_rows = ctypes.c_uint64(list_n_rows) if list_n_rows is not None else None
    rc = ftwin.frm_filter_rows(blob, data, length, fields.ctypes.data, stride, n_columns, ctypes.byref(sel), keep.ctypes.data,
                               kept.ctypes.data if kept is not None else None, capacity,
                               list_offsets.ctypes.data if list_offsets is not None else None, list_rows or 0,
                               ctypes.byref(n_rows) if n_rows is not None else None,
                               list_out.ctypes.data if list_out is not None else None, ctypes.byref(res), ctypes.byref(ksel))
    return Filtered(rc, res, keep, kept, list_out, ksel)


def twin_take(ftwin, take, take_sel, fields, stride, n_columns, rows_sel, out_stride, out_capacity):
    """frm_take_rows -> (MsjTakeRowsResult, out FIELD_DTYPE[(n_columns - 1) * out_stride + out_capacity + 4 of canary], out select)"""
    fields, take = np.ascontiguousarray(fields), np.ascontiguousarray(take, dtype=np.uint32)
    n_out = (n_columns - 1) * out_stride + out_capacity
    out = np.full(16 * n_out + CANARY, FILL, dtype=np.uint8).view(FIELD_DTYPE)
    res, osel = _lib.MsjTakeRowsResult(), _lib.MsjSelectDocumentsResult()
    ftwin.frm_take_rows(take.ctypes.data, ctypes.byref(take_sel), fields.ctypes.data, stride, n_columns, ctypes.byref(rows_sel), out.ctypes.data,
                        out_stride, out_capacity, ctypes.byref(res), ctypes.byref(osel))
    return res, out, osel


def take_summary(r):
    return (r.code, r.flags, r.n_rows, r.n_out_of_range, r.n_found, r.n_no_bits, r.reserved)


def fill_record():
    return np.full(16, FILL, dtype=np.uint8).view(FIELD_DTYPE)[0]


def py_take(take, K, columns, R, n_columns, out_stride, out_capacity):
    """-> (out as a list of record tuples or None where nothing is written, n_out_of_range, n_found, n_no_bits)"""
    out = [None] * ((n_columns - 1) * out_stride + out_capacity)
    oor = found = no_bits = 0
    for j in range(K):
        src = int(take[j])
        oor += src >= R
        for c in range(n_columns):
            t = tuple(int(x) for x in columns[c][src].tolist()) if src < R else MISSING
            found += t[4] == 0
            no_bits += bool(t[3] & NO_BITS)
            out[c * out_stride + j] = t
    return out, oor, found, no_bits


def check_take(res, out, osel, take, K, columns, R, n_columns, out_stride, out_capacity, sel_code=0, stride=None):
    """One take call against the Python loop, the whole of the output array"""
    fill = tuple(int(x) for x in fill_record().tolist())
    got = [tuple(int(x) for x in r.tolist()) for r in out]
    over = K > out_capacity or K >= 1 << 31 or R > (stride if stride is not None else R) or R >= 1 << 31
    if sel_code or over:
        assert take_summary(res) == (sel_code or MSJ_CAPACITY, 0, 0 if sel_code else K, 0, 0, 0, 0)
        assert all(g == fill for g in got)
        assert (osel.code, osel.n_documents, osel.n_paths, osel.n_found, osel.n_no_bits) == (res.code, 0, n_columns, 0, 0)
        return
    want, oor, found, no_bits = py_take(take, K, columns, R, n_columns, out_stride, out_capacity)
    assert take_summary(res) == (0, 0, K, oor, found, no_bits, 0)
    assert (osel.code, osel.flags, osel.n_documents, osel.n_paths, osel.n_found, osel.n_no_bits, osel.reserved) == (0, 0, K, n_columns, found, no_bits, 0)
    for at, w in enumerate(want):
        assert got[at] == (w if w is not None else fill), at
    assert all(g == fill for g in got[len(want):])


def check_filter(got, specs, any_, columns, values, R, capacity, mask_only=False, list_offsets=None, list_rows=None, P=None, sel_code=0):
    """One filter call against the yardstick, the whole of every output array"""
    flags = ANY if any_ else 0
    assert got.rc == 0
    untouched = lambda a, n: a is None or bool((a.view(np.uint8)[n:] == FILL).all())
    if sel_code or R > capacity or R >= 1 << 31:
        assert got.summary() == (sel_code or MSJ_CAPACITY, 0 if sel_code else flags, 0 if sel_code else R, 0, 0, 0, 0)
        assert got.select_summary() == (got.res.code, 0, 0, 1, 0, 0, 0)
        assert untouched(got.keep, 0) and untouched(got.kept, 0) and untouched(got.list_out, 0)
        return
    list_over = list_offsets is not None and (P > list_rows or P >= 1 << 31)
    keep, kept, n_no_bits, n_missing, list_want = py_filter(specs, any_, columns, values, R, None if list_over else list_offsets, P)
    code = MSJ_CAPACITY if list_over else 0
    assert got.summary() == (code, flags, R, len(kept), n_no_bits, n_missing, 0)
    assert got.select_summary() == (code, 0, len(kept), 1, len(kept), 0, 0)
    assert got.keep[:R].tolist() == keep and untouched(got.keep, R)
    if not mask_only:
        assert got.kept[:len(kept)].tolist() == kept and untouched(got.kept, 4 * len(kept))
    if list_offsets is not None:
        if list_over:
            assert untouched(got.list_out, 0)
        else:
            assert got.list_out[:P + 1].tolist() == list_want and untouched(got.list_out, 8 * (P + 1))


# ---- tests: numbers ---------------------------------------------------------------------------------------------------------

INTS = [0, 1, -1, 2**53 - 1, -(2**53 - 1), 2**53, -2**53, 2**53 + 1, -(2**53 + 1), 2**63 - 1, -2**63]
DOUBLES = [0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.0**53, -2.0**53, 2.0**53 + 2, -(2.0**53 + 2), 9.223372036854775807e18,
           -9.223372036854775807e18, 5e-324, 1.7976931348623157e308, -1.7976931348623157e308]


def test_exact_compare(ftwin):
    """All five ops over the cross product of the pinned integers and doubles, on either side, against Python's own exact
    comparison: int with double, double with int, int with int, double with double"""
    values = INTS + DOUBLES
    n = 0
    for operand in values:
        specs = [Spec(0, op, operand) for op in NUM_OPS] + [Spec(0, op, operand, neg=True) for op in NUM_OPS]
        blob = compile_specs(ftwin, specs)
        for x in values:
            record = int_rec(x) if isinstance(x, int) else double_rec(x)
            for i, s in enumerate(specs):
                said = ftwin.frm_eval(blob, i, record.ctypes.data, b"", 0)
                assert (bool(said & HOLDS), said & ~HOLDS) == py_pred(s, record[0], None), (x, s.op, operand, s.neg)
                n += 1
    assert n == len(values) ** 2 * 10
    # the pins of the header file
    assert ftwin.frm_cmp_int_double(9007199254740993, 9007199254740992.0) == 1
    assert ftwin.frm_cmp_int_double(0, -0.0) == 0
    assert ftwin.frm_cmp_int_double(-2**63, -9.223372036854775807e18) == 0 and ftwin.frm_cmp_int_double(2**63 - 1, 9.223372036854775807e18) == -1
    assert ftwin.frm_cmp_int_double(5, math.nan) == 2
    nan = rec(0x7FF8000000000000, "d")
    blob = compile_specs(ftwin, [Spec(0, op, 1) for op in NUM_OPS] + [Spec(0, op, 1.0) for op in NUM_OPS])
    assert all(ftwin.frm_eval(blob, i, nan.ctypes.data, b"", 0) == 0 for i in range(10))


# ---- tests: strings ---------------------------------------------------------------------------------------------------------

def string_window():
    """A window of string bodies and the records that name them -> (data, [(name, record)])"""
    bodies = [("plain A", b"A", False), ("escaped A", b"\\u0041", True), ("empty", b"", False), ("ab", b"ab", False),
              ("surrogate pair", b"\\ud83d\\ude00x", True), ("euro", b"\\u20acz", True), ("euro plain", "€z".encode(), False),
              ("two escapes", b"\\u0041\\u0041", True), ("nul", b"a\\u0000b", True), ("simple escapes", b"q\\n\\t\\\"\\\\", True),
              ("lone low surrogate", b"\\ude00", True), ("damaged hex", b"ab\\u00zzcd", True), ("cut escape", b"abc\\u00", True),
              ("trailing backslash", b"ab\\", True), ("255 q", b"q" * 255, False), ("256 q", b"q" * 256, False),
              ("255 escaped", b"\\u0071" * 255, True), ("long escaped", b"\\u0071" * 300, True), ("flag without escape", b"abc", True)]
    data, records = bytearray(), []
    for name, body, escaped in bodies:
        data += b'"'
        records.append((name, string_rec(len(data), len(body), escaped)))
        data += body + b'" '
    tail = b"tail"                       # a span that ends at len, and one a byte past it
    data += b'"'
    records.append(("ends at len", string_rec(len(data), len(tail))))
    records.append(("one past len", string_rec(len(data), len(tail) + 1)))
    records.append(("escaped one past len", string_rec(len(data), len(tail) + 1, True)))
    data += tail
    records.append(("huge span", string_rec(0xFFFFFFFF, 0xFFFFFFFF)))
    return bytes(data), records


OPERANDS = [b"", b"A", b"a", b"ab", b"abc", b"q" * 255, b"q" * 254 + b"r", b"\xf0\x9f\x98\x80", b"\xf0\x9f\x98\x80x", b"\xf0\x9f", b"\xe2",
            b"\xe2\x82", b"\xe2\x82\xac", b"\xe2\x83", b"\xe2\x82\xacz", b"AA", b"a\0b", b"a\0", b"\0", b"q\n\t\"\\", b"q\n", b"tail", b"tai",
            b"tail ", b"ab\\", b"abc\\u00", b"\xed\xb8\x80"]


def test_strings_against_the_string_column(ftwin, ctwin):
    """STR_EQ and STR_PREFIX, plain and negated, of every operand on every record, against == and startswith over the bytes
    the string-column twin writes for the record"""
    data, records = string_window()
    values = {name: string_value(ctwin, data, len(data), r) for name, r in records}
    assert values["plain A"] == values["escaped A"] == b"A" and values["surrogate pair"] == b"\xf0\x9f\x98\x80x"
    assert values["euro"] == values["euro plain"] == b"\xe2\x82\xacz" and values["nul"] == b"a\0b"
    assert values["ends at len"] == b"tail" and values["one past len"] is None and values["huge span"] is None
    assert values["255 escaped"] == b"q" * 255 and values["two escapes"] == b"AA"
    for at in range(0, len(OPERANDS), 4):
        specs = [Spec(0, op, o, neg) for o in OPERANDS[at:at + 4] for op in (STR_EQ, STR_PREFIX) for neg in (False, True)]
        blob = compile_specs(ftwin, specs)
        for name, r in records:
            for i, s in enumerate(specs):
                said = ftwin.frm_eval(blob, i, r.ctypes.data, data, len(data))
                assert (bool(said & HOLDS), said & ~HOLDS) == py_pred(s, r[0], values[name]), (name, s.op, s.operand, s.neg)
    # a raw length outside [n, 6n] is decided before a byte is read: the window pointer may be anything
    assert ftwin.frm_starts_with(None, 100, 10, 12, 1, b"abc", 3) == 0


# ---- tests: every op on every kind of record ----------------------------------------------------------------------------------

def all_kinds(data_len):
    kinds = [rec(7, "{", token=3), rec(9, "[", token=4), string_rec(1, 1), string_rec(5, 7, True), int_rec(-5), int_rec(300),
             double_rec(250.5), double_rec(-0.0), rec(0, "t"), rec(0, "f"), rec(0, "n"), error_rec(20), error_rec(17), error_rec(3),
             rec(0, "l", NO_BITS), rec(0, "d", NO_BITS), rec(123, "x"), rec(5, "l", 0, 20), string_rec(data_len, 1)]
    return kinds


def every_spec():
    specs = [Spec(0, FOUND)] + [Spec(0, TYPE, m) for m in (1, 2, 4, 8, 16, 32, 64, 128, 0xFF, 8 | 16, 4 | 128)]
    specs += [Spec(0, op, y) for op in NUM_OPS for y in (300, 250.5, 0, -5.0)]
    specs += [Spec(0, op, o) for op in (STR_EQ, STR_PREFIX) for o in (b"", b"A", b"AB")]
    return specs + [Spec(s.column, s.op, s.operand, True) for s in specs]


def test_every_op_on_every_record_kind(ftwin, ctwin):
    data = b'"A"  \\u0041B'
    kinds = all_kinds(len(data))
    specs = every_spec()
    for at in range(0, len(specs), 16):
        part = specs[at:at + 16]
        blob = compile_specs(ftwin, part)
        for r in kinds:
            value = string_value(ctwin, data, len(data), r)
            for i, s in enumerate(part):
                said = ftwin.frm_eval(blob, i, r.ctypes.data, data, len(data))
                assert (bool(said & HOLDS), said & ~HOLDS) == py_pred(s, r[0], value), (r, s.op, s.operand, s.neg)


# ---- tests: ALL against ANY -------------------------------------------------------------------------------------------------

def draw_columns(rng, data_len, n_columns, stride):
    kinds = all_kinds(data_len)
    fields = np.concatenate([kinds[int(rng.integers(len(kinds)))] for _ in range(n_columns * stride)])
    return fields


def values_of(ctwin, data, fields, n_columns, stride, R):
    col = tcm.twin_column(ctwin, data, fields, n_columns * stride) if fields.size else None
    rows = col.rows() if col is not None else []
    return [rows[c * stride:c * stride + stride] for c in range(n_columns)]


@pytest.mark.parametrize("n_preds", [1, 2, 16])
def test_all_against_any(ftwin, ctwin, n_preds):
    rng = np.random.default_rng(n_preds)
    data = b'"A"  \\u0041B'
    pool = every_spec()
    for any_ in (False, True):
        for trial in range(6):
            n_columns, R = 16, 70
            fields = draw_columns(rng, len(data), n_columns, R)
            specs = []
            for _ in range(n_preds):
                s = pool[int(rng.integers(len(pool)))]
                specs.append(Spec(int(rng.integers(n_columns)), s.op, s.operand, s.neg))
            specs[0].column = 15 if trial == 0 else specs[0].column
            columns = [fields[c * R:(c + 1) * R] for c in range(n_columns)]
            values = values_of(ctwin, data, fields, n_columns, R, R)
            got = twin_filter(ftwin, compile_specs(ftwin, specs, any_), data, len(data), fields, R, n_columns, tcm.select_result(R), R)
            check_filter(got, specs, any_, columns, values, R, R)


# ---- tests: create ----------------------------------------------------------------------------------------------------------

def test_create_errors(ftwin):
    blob = ctypes.create_string_buffer(ftwin.frm_predicates_bytes())

    def rc(specs, flags=0, n=None):
        table, alive = spec_table(specs)
        return ftwin.frm_compile(table, len(specs) if n is None else n, flags, blob)

    ok = Spec(0, FOUND)
    assert rc([ok]) == 0 and rc([ok] * 16) == 0 and rc([ok], ANY) == 0
    assert ftwin.frm_compile(None, 1, 0, blob) == -1
    assert rc([ok], n=0) == -1 and rc([ok] * 17) == -1
    assert rc([Spec(15, FOUND)]) == 0 and rc([Spec(16, FOUND)]) == -1
    assert rc([Spec(0, 9)]) == -1 and rc([Spec(0, 0xFFFFFFFF)]) == -1
    assert rc([ok], 2) == -1 and rc([ok], 0x80000000) == -1
    assert rc([Spec(0, STR_EQ, b"x" * 255)]) == 0 and rc([Spec(0, STR_EQ, b"x" * 256)]) == -1 and rc([Spec(0, STR_PREFIX, b"x" * 256)]) == -1
    assert rc([Spec(0, STR_EQ, b"")]) == 0
    for op in NUM_OPS:
        assert rc([Spec(0, op, 1.5)]) == 0 and rc([Spec(0, op, -2**63)]) == 0
        assert rc([Spec(0, op, math.inf)]) == -1 and rc([Spec(0, op, -math.inf)]) == -1 and rc([Spec(0, op, math.nan)]) == -1
    assert rc([Spec(0, TYPE, 0)]) == -1 and rc([Spec(0, TYPE, 0x100)]) == -1 and rc([Spec(0, TYPE, 0xFF)]) == 0
    # an unknown flag; MSJ_PRED_DOUBLE on an op that is not numeric is one; a string operand without its pointer
    for bad in (_lib.MsjPredicate(0, FOUND, 4, 0, 0, None), _lib.MsjPredicate(0, FOUND, DOUBLE, 0, 0, None),
                _lib.MsjPredicate(0, STR_EQ, DOUBLE, 0, 0, None), _lib.MsjPredicate(0, STR_EQ, 0, 3, 0, None)):
        assert ftwin.frm_compile(ctypes.byref(bad), 1, 0, blob) == -1
    # a column at or past n_columns: refused by the call, on the host
    good = compile_specs(ftwin, [Spec(3, FOUND)])
    fields = np.concatenate([error_rec(20)] * 8)
    assert twin_filter(ftwin, good, b"", 0, fields, 2, 3, tcm.select_result(2), 2).rc == -1
    assert twin_filter(ftwin, good, b"", 0, fields, 2, 4, tcm.select_result(2), 2).rc == 0


# ---- tests: compaction, list offsets and take on damaged inputs -------------------------------------------------------------

def damaged_case(rng, ftwin, ctwin, case):
    data = b'"A"  \\u0041B'
    n_columns = int(rng.integers(1, 4))
    stride = int(rng.integers(0, 40))
    fields = draw_columns(rng, len(data), n_columns, stride) if stride else np.zeros(0, dtype=FIELD_DTYPE)
    columns = [fields[c * stride:(c + 1) * stride] for c in range(n_columns)]
    values = values_of(ctwin, data, fields, n_columns, stride, stride)
    pool = every_spec()
    specs = []
    for _ in range(int(rng.integers(1, 4))):
        s = pool[int(rng.integers(len(pool)))]
        specs.append(Spec(int(rng.integers(n_columns)), s.op, s.operand, s.neg))
    any_ = bool(rng.integers(2))
    blob = compile_specs(ftwin, specs, any_)
    # R below, at and above the capacity; the capacity one short
    form = case % 6
    capacity = stride if form != 1 else max(stride - 1, 0)
    R = stride if form != 2 else int(rng.integers(0, stride + 1))
    if form == 3:
        R = stride + 1 + int(rng.integers(3))
    if n_columns > 1 and capacity > stride:
        capacity = stride
    sel_code = 5 if case % 41 == 0 else 0
    sel = tcm.select_result(R, sel_code)
    mask_only = form == 4
    # list offsets: ascending, descending, past R, huge
    list_rows = int(rng.integers(0, 12))
    offs = np.sort(rng.integers(0, R + 1, list_rows + 1)).astype(np.uint64)
    for _ in range(int(rng.integers(0, 4))):
        k = int(rng.integers(list_rows + 1))
        offs[k] = [R + 1 + int(rng.integers(4)), 0xFFFFFFFFFFFFFFFF, int(rng.integers(0, R + 1)), 1 << 31][int(rng.integers(4))]
    P = list_rows
    n_list = None
    if case % 5 == 0:
        n_list = P = [0, max(list_rows - 1, 0), list_rows, list_rows + 1][int(rng.integers(4))]
    with_list = case % 3 != 0
    got = twin_filter(ftwin, blob, data, len(data), fields, stride, n_columns, sel, capacity, mask_only,
                      offs if with_list else None, list_rows if with_list else None, n_list if with_list else None)
    check_filter(got, specs, any_, columns, values, R, capacity, mask_only, offs if with_list else None, list_rows, P, sel_code)
    # the take: the kept rows, or a damaged vector -- indices at R - 1, R and 0xFFFFFFFF, repeats, any order
    Rt = min(R, stride) if case % 4 else R
    if got.kept is not None and got.res.code == 0 and case % 2:
        take = got.kept[:got.res.n_kept].copy()
    else:
        take = rng.integers(0, max(Rt, 1), int(rng.integers(0, 50))).astype(np.uint32)
    for _ in range(int(rng.integers(0, 4))):
        if take.size:
            take[int(rng.integers(take.size))] = [max(Rt - 1, 0), Rt, 0xFFFFFFFF, take[0]][int(rng.integers(4))]
    K = int(take.size)
    tform = (case // 6) % 4
    out_capacity = K if tform != 1 else max(K - 1, 0)
    Kd = K if tform != 2 else K + 1     # the device word says one more than the vector holds room for
    out_stride = out_capacity + int(rng.integers(0, 3))
    take_code = 9 if case % 53 == 0 else 0
    res, out, osel = twin_take(ftwin, take, tcm.select_result(Kd, take_code), fields, stride, n_columns, tcm.select_result(Rt, sel_code), out_stride,
                               out_capacity)
    check_take(res, out, osel, take, Kd, columns, Rt, n_columns, out_stride, out_capacity, take_code or sel_code, stride)


def test_damaged_inputs(ftwin, ctwin):
    """300 seeded cases, none dropped: every one is compared with the yardstick over the whole of its arrays"""
    rng = np.random.default_rng(20261020)
    for case in range(300):
        damaged_case(rng, ftwin, ctwin, case)


def test_pinned_compaction(ftwin, ctwin):
    """The small shapes by hand: no row, one row, every other row, the mask-only form, list offsets with empty lists, a list
    whose elements all go, offsets that descend or exceed R, take indices at R - 1, R and 0xFFFFFFFF"""
    data = b""
    R = 9
    fields = np.concatenate([int_rec(k) for k in range(R)])
    specs = [Spec(0, NUM_GE, 2), Spec(0, NUM_LT, 6.5)]   # rows 2..6
    blob = compile_specs(ftwin, specs)
    offs = np.array([0, 0, 2, 2, 5, 9, 3, 100, 2**63], dtype=np.uint64)
    got = twin_filter(ftwin, blob, data, 0, fields, R, 1, tcm.select_result(R), R, list_offsets=offs, list_rows=8)
    assert got.keep[:R].tolist() == [0, 0, 1, 1, 1, 1, 1, 0, 0] and got.kept[:5].tolist() == [2, 3, 4, 5, 6]
    assert got.list_out[:9].tolist() == [0, 0, 0, 0, 3, 5, 1, 5, 5]
    check_filter(got, specs, False, [fields], [[None] * R], R, R, False, offs, 8, 8)
    got = twin_filter(ftwin, blob, data, 0, fields, R, 1, tcm.select_result(0), R, list_offsets=offs, list_rows=8)
    assert got.summary() == (0, 0, 0, 0, 0, 0, 0) and got.list_out[:9].tolist() == [0] * 9
    got = twin_filter(ftwin, blob, data, 0, fields, R, 1, tcm.select_result(R), R - 1)
    check_filter(got, specs, False, [fields], [[None] * R], R, R - 1)
    got = twin_filter(ftwin, blob, data, 0, fields, R, 1, tcm.select_result(R), R, mask_only=True)
    check_filter(got, specs, False, [fields], [[None] * R], R, R, True)
    take = np.array([8, 9, 0xFFFFFFFF, 0, 0, 3], dtype=np.uint32)
    res, out, osel = twin_take(ftwin, take, tcm.select_result(6), fields, R, 1, tcm.select_result(R), 6, 6)
    assert take_summary(res) == (0, 0, 6, 2, 4, 0, 0)
    assert [tuple(int(x) for x in r.tolist()) for r in out[:3]] == [(8, 0, ord("l"), 0, 0), MISSING, MISSING]
    check_take(res, out, osel, take, 6, [fields], R, 1, 6, 6, 0, R)
    res, out, osel = twin_take(ftwin, take, tcm.select_result(6), fields, R, 1, tcm.select_result(R), 5, 5)
    check_take(res, out, osel, take, 6, [fields], R, 1, 5, 5, 0, R)
