"""CPU check of the arithmetic of msj_cast_strings_device (mojo_simdjson_amd/csrc/cast_strings_math.h).

The host twin (tests/cast_strings_math_host.cpp: the header's grammar, calendar, number wrapper and record-in / record-out,
serially) runs over hand-made windows and records.  The yardstick is Python and knows nothing of the header: a ``re`` of the
timestamp grammar, ``datetime.date(y, m, d).toordinal() - 719163`` for the days (year 0000 as the same day of year 0400 less
146097 days) and integer arithmetic; for numbers tests/test_number_math.py's ``expected``, which is Python's ``int`` and
``float``.  The yardstick itself is checked against ``datetime.fromisoformat``.  A row's value is what the string-column twin
(tests/string_column_math_host.cpp) writes for its record.  Every array at its exact size with the fill and 64 canary bytes
behind each capacity.  The kernels that run the same header on the device are covered by tests/test_cast_strings.py (-m gpu);
arrays from anywhere by tests/test_cast_strings_sanitizers.py.
"""
import ctypes
import datetime
import os
import random
import re
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import test_number_math as tnm
from tests import test_string_column_math as tcm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
FILL = 0x77
CANARY = 64
ESCAPED, NO_BITS = 2, 64
TIMESTAMP, NUMBER = 1, 2
UNITS = {"s": 0, "ms": 1, "us": 2, "ns": 3}
PER_SECOND = {"s": 1, "ms": 10**3, "us": 10**6, "ns": 10**9}
KEEP_NUMBERS = 1
PASSED, CAST, SYNTAX, RANGE, OTHER = range(5)     # csrc/cast_strings_math.h: what became of one record
NUMBER_ERROR, INCORRECT_TYPE = 9, 17
MAX_BYTES = {TIMESTAMP: 35, NUMBER: 128}
ERROR_9 = (0, 0xFFFFFFFF, 0, 0, NUMBER_ERROR)       # bits, token, type, flags, code
ERROR_17 = (0, 0xFFFFFFFF, 0, 0, INCORRECT_TYPE)

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/cast_strings_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libcast_strings_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "cast_strings_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, cint = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int
    for name, args, res in (("csm_days_from_civil", [u32, u32, u32], ctypes.c_int64),
                            ("csm_parse_timestamp", [ctypes.c_char_p, u64, u32, vp], u32),
                            ("csm_parse_number", [ctypes.c_char_p, u64, vp, vp], u32),
                            ("csm_cast_record", [vp, ctypes.c_char_p, u64, u32, u32, u32, vp], u32),
                            ("csm_cast_strings", [vp, u64, vp, vp, u32, u32, u32, vp, u64, vp, vp], cint)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def ctw():
    return load_twin()


@pytest.fixture(scope="module")
def ctwin():
    return tcm.load_twin()


# ---- the yardstick ----------------------------------------------------------------------------------------------------------

TS = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})"
                rb"(?:[Tt ]([0-9]{2}):([0-9]{2})(?::([0-9]{2})(?:[.,]([0-9]{1,9}))?)?(?:([Zz])|([+-])([0-9]{2})(?::?([0-9]{2}))?)?)?")


def py_days(y, m, d):
    """Days since 1970-01-01, proleptic Gregorian, year 0..9999; ValueError for a day the month has not"""
    if y == 0:
        return datetime.date(400, m, d).toordinal() - 719163 - 146097
    return datetime.date(y, m, d).toordinal() - 719163


def py_timestamp(value, unit):
    """(outcome, the int64) of a value's bytes"""
    m = TS.fullmatch(value)
    if m is None or len(value) > 35:
        return SYNTAX, 0
    y, mo, d = int(m.group(1)), int(m.group(2)), int(m.group(3))
    hh, mi, ss = (int(m.group(i) or 0) for i in (4, 5, 6))
    try:
        days = py_days(y, mo, d)
    except ValueError:
        return SYNTAX, 0
    if hh > 23 or mi > 59 or ss > 59:
        return SYNTAX, 0
    off = 0
    if m.group(9):
        oh, om = int(m.group(10)), int(m.group(11) or 0)
        if oh > 23 or om > 59:
            return SYNTAX, 0
        off = (oh * 3600 + om * 60) * (1 if m.group(9) == b"+" else -1)
    per = PER_SECOND[unit]
    frac = int((m.group(7) or b"0").ljust(9, b"0")) // (10**9 // per)
    v = (days * 86400 + hh * 3600 + mi * 60 + ss - off) * per + frac
    if not -(1 << 63) <= v < (1 << 63):
        return RANGE, 0
    return CAST, v & ((1 << 64) - 1)


def py_number(value):
    """(outcome, bits, tag) of a value's bytes: the number tests' reference on a text that is a number whole"""
    if len(value) > 128 or tnm.GRAMMAR.fullmatch(value) is None:
        return SYNTAX, 0, "l"
    kind, bits = tnm.expected(value)
    if kind == tnm.ERR_RANGE:
        return RANGE, 0, "l"
    assert kind in (tnm.INT64, tnm.DOUBLE)
    return CAST, bits, "l" if kind == tnm.INT64 else "d"


def py_value(value, kind, unit):
    if kind == TIMESTAMP:
        o, bits = py_timestamp(value, unit)
        return o, bits, "l"
    return py_number(value)


def as_tuple(rec):
    return int(rec["bits"]), int(rec["token"]), int(rec["type"]), int(rec["flags"]), int(rec["code"])


def py_record(rec, value, kind, unit, flags):
    """(the output record as a tuple, outcome); value: the row's string bytes by the string-column twin, None for a row
    that is no string"""
    t = as_tuple(rec)
    if t[4] != 0:
        return t, PASSED
    if value is None:
        if flags & KEEP_NUMBERS and chr(t[2]) in "ld":
            return t, CAST
        return ERROR_17, OTHER
    raw = t[0] >> 32
    if (t[3] & ESCAPED and raw > 6 * MAX_BYTES[kind]) or len(value) > MAX_BYTES[kind]:
        return ERROR_9, SYNTAX
    o, bits, tag = py_value(value, kind, unit)
    return ((bits, t[1], ord(tag), 0, 0), CAST) if o == CAST else (ERROR_9, o)


# ---- windows and records ----------------------------------------------------------------------------------------------------

def rec(bits=0, typ=None, flags=0, code=0, token=0):
    r = np.zeros(1, dtype=FIELD_DTYPE)
    r["bits"], r["token"], r["type"], r["flags"], r["code"] = bits & 0xFFFFFFFFFFFFFFFF, token, ord(typ) if typ else 0, flags, code
    return r


def escape_at(value, i):
    """The raw body that spells byte i of `value` as \\u00XX"""
    return value[:i] + b"\\u%04x" % value[i] + value[i + 1:]


def window_of(bodies, gap=b'","'):
    """Raw bodies -> (the window's bytes, the records of the bodies as strings: ESCAPED where a backslash is in one, tokens
    ascending)"""
    data, recs = bytearray(b'["'), []
    for k, body in enumerate(bodies):
        recs.append(rec(len(data) | (len(body) << 32), '"', ESCAPED if b"\\" in body else 0, token=2 * k + 1))
        data += body + gap
    return bytes(data), np.concatenate(recs) if recs else np.zeros(0, dtype=FIELD_DTYPE)


class Cast:
    """What one call left: the result, the select result, the records with their canary"""

    def __init__(self, rc, res, sel, out, capacity):
        self.rc, self.res, self.sel, self.out, self.capacity = rc, res, sel, out, capacity

    def records(self, n=None):
        n = int(self.res.n_rows) if n is None else n
        return self.out[:16 * n].view(FIELD_DTYPE)

    def summary(self):
        r, s = self.res, self.sel
        return ((r.code, r.flags, r.n_rows, r.n_cast, r.n_syntax, r.n_range, r.n_other),
                (s.code, s.flags, s.n_documents, s.n_paths, s.n_found, s.n_no_bits, s.reserved))

    def untouched(self, rows):
        return bool((self.out[16 * rows:] == FILL).all())


def twin_cast(ctw, data, records, kind, unit="ns", flags=0, R=None, length=None, capacity=None, sel_code=0, in_place=False, room=None):
    """room: the records the output array really has, where the capacity the call is told is not to be allocated"""
    R = len(records) if R is None else R
    capacity = len(records) if capacity is None else capacity
    length = len(data) if length is None else length
    records = np.ascontiguousarray(records)
    out = np.full(16 * (capacity if room is None else room) + CANARY, FILL, dtype=np.uint8)
    if in_place:
        out[:16 * len(records)] = records.view(np.uint8)
    src = out if in_place else records.view(np.uint8)
    sel = tcm.select_result(R, sel_code)
    res, osel = _lib.MsjCastStringsResult(), _lib.MsjSelectDocumentsResult()
    rc = ctw.csm_cast_strings(data, length, src.ctypes.data, ctypes.byref(sel), kind, UNITS[unit], flags, out.ctypes.data, capacity,
                              ctypes.byref(res), ctypes.byref(osel))
    return Cast(rc, res, osel, out, capacity)


def check_column(ctw, ctwin, data, records, kind, unit="ns", flags=0, length=None):
    """The twin over the records against the yardstick over the string-column twin's values: every record, every counter"""
    length = len(data) if length is None else length
    got = twin_cast(ctw, data, records, kind, unit, flags, length=length)
    assert got.rc == 0
    values = tcm.twin_column(ctwin, data, records, len(records), length=length).rows() if len(records) else []
    want = [py_record(r, v, kind, unit, flags) for r, v in zip(records, values)]
    outs = got.records()
    for k, (w, o) in enumerate(want):
        assert as_tuple(outs[k]) == w, (k, values[k], as_tuple(records[k]), as_tuple(outs[k]), w, o)
    n = [sum(1 for _, o in want if o == x) for x in (CAST, SYNTAX, RANGE, OTHER)]
    no_bits = sum(1 for w, _ in want if w[3] & NO_BITS)
    assert got.summary() == ((0, kind | UNITS[unit] << 8 | flags << 16, len(records), *n), (0, 0, len(records), 1, n[0], no_bits, 0))
    assert got.untouched(len(records))
    return [o for _, o in want]


# ---- corpora ----------------------------------------------------------------------------------------------------------------

def timestamp_corpus():
    """Accepted and refused timestamp values: every optional part, separator and offset form; every field at its bounds"""
    out = []
    date = b"2024-05-01"
    for sep in (b"T", b"t", b" "):
        for tail in (b"12:34", b"12:34:56", b"12:34:56.7", b"12:34:56,789", b"12:34:56.123456789"):
            for off in (b"", b"Z", b"z", b"+05", b"-05", b"+0530", b"+05:30", b"-23:59", b"+23:59", b"+00:00"):
                out.append(date + sep + tail + off)
    out += [date, b"0000-01-01T00:00:00Z", b"9999-12-31T23:59:59Z", b"0000-01-01T00:00:00+23:59", b"9999-12-31T23:59:59-23:59",
            b"0000-01-01T00:00:00-23:59", b"9999-12-31T23:59:59+23:59", b"0000-02-29", b"1970-01-01T00:00:00Z", b"1969-12-31T23:59:59.999999999Z"]
    for y in (1900, 2000, 2100, 2023, 2024, 0, 400, 9999):
        for m in range(0, 14):
            for d in (0, 1, 28, 29, 30, 31, 32):
                out.append(b"%04d-%02d-%02d" % (y, m, d))
    for bad in (b"24:00", b"23:60", b"23:59:60", b"00:00:00", b"23:59:59", b"23:59:5", b"2:00", b"12:3", b"12:34:", b"12:34:56.", b"12-34"):
        out.append(date + b"T" + bad)
    for off in (b"+24:00", b"+23:60", b"+2", b"+05:", b"+05:3", b"+053", b"Z ", b"ZZ", b"+05:30Z", b"x", b"+", b"-", b"+0A"):
        out.append(date + b"T12:34:56" + off)
    for digits in range(0, 11):
        out.append(date + b"T12:34:56." + b"9876543219"[:digits] + b"Z")
        out.append(b"1969-12-31T23:59:59." + b"0000000011"[:digits])
    out += [b"2262-04-11T23:47:16.854775807Z", b"2262-04-11T23:47:16.854775808Z", b"1677-09-21T00:12:43.145224192Z",
            b"1677-09-21T00:12:43.145224191Z", b"2262-04-11T23:47:17Z", b"1677-09-21T00:12:43Z", b"1677-09-21T00:12:44Z",
            b"2262-04-12", b"1677-09-21", b"1677-09-22", b"2262-04-11T23:47:16.854775807+00:00", b"2262-04-12T00:47:16.854775807+01:00"]
    long35 = b"2024-05-01T12:34:56.123456789+05:30"
    assert len(long35) == 35
    out += [long35, long35 + b"0", long35 + b" ", b" " + date, date + b" ", b"+" + date, b"+2024-05-01", b"20240501", b"2024-5-1", b"2024/05/01",
            b"2024-05-01T123456", b"2024-05-01T12:34:56.789 Z", b"", b"2024", b"2024-05-0", b"2024-05-01T", b"2024-05-01Z", b"2024-05-01+05:30",
            b"2024-05-01T12:34:56\x00", b"\xff\xfe24-05-01", b"2024-05-01 12:34:56.789+05:30"]
    return out


def number_corpus():
    """The number tests' corpus as string values, with what only a string can hold"""
    rng = random.Random(11)
    out = list(tnm.boundary_texts()) + list(tnm.SYNTAX) + tnm.fallback_texts(rng, 20)
    out += [b"12.50", b"9007199254740993", b"1e-3", b"-0", b"1e400", b"-1e400", b"0", b"-", b"", b" 1", b"1 ", b"\t1", b"1\n", b"+1", b"1,2", b"1:2",
            b"[1]", b"1}", b"1e5 ", b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"1.0", b"NaN",
            b"Infinity", b"0x10", b"1_000", b"1" * 128, b"1" * 129, b"0." + b"3" * 126, b"0." + b"3" * 127, b"1e" + b"0" * 126, b"1e" + b"0" * 127]
    return [t for t in out if b'"' not in t and b"\\" not in t]


def escaped_twins(values, rng):
    """For each value the raw bodies that spell its first, a middle and its last byte as \\u00XX, and one with a NUL inside"""
    out = []
    for v in values:
        if not v:
            continue
        for i in {0, len(v) // 2, len(v) - 1}:
            out.append(escape_at(v, i))
        out.append(v[:len(v) // 2] + b"\\u0000" + v[len(v) // 2:])
    return out


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_days_and_fixed_points(ctw):
    assert py_days(1970, 1, 1) == 0 and py_days(0, 1, 1) * 86400 == -62167219200
    assert py_timestamp(b"0000-01-01T00:00:00Z", "s") == (CAST, -62167219200 & ((1 << 64) - 1))
    assert py_timestamp(b"9999-12-31T23:59:59Z", "s") == (CAST, 253402300799)
    assert py_timestamp(b"2262-04-11T23:47:16.854775807Z", "ns") == (CAST, (1 << 63) - 1)
    assert py_timestamp(b"1677-09-21T00:12:43.145224192Z", "ns") == (CAST, 1 << 63)
    assert py_timestamp(b"2262-04-11T23:47:16.854775808Z", "ns")[0] == RANGE and py_timestamp(b"1677-09-21T00:12:43.145224191Z", "ns")[0] == RANGE
    for y in list(range(0, 10000, 7)) + [0, 1, 399, 400, 1900, 2000, 2100, 9999]:
        for m, d in ((1, 1), (2, 28), (3, 1), (12, 31)):
            assert ctw.csm_days_from_civil(y, m, d) == py_days(y, m, d), (y, m, d)
    assert ctw.csm_days_from_civil(0, 2, 29) == py_days(0, 2, 29) and ctw.csm_days_from_civil(2000, 2, 29) == py_days(2000, 2, 29)


def test_yardstick_against_fromisoformat():
    """The yardstick's own arithmetic, on the subset ``datetime.fromisoformat`` of Python 3.10 accepts"""
    rng = random.Random(5)
    utc = datetime.timezone.utc
    epoch = datetime.datetime(1970, 1, 1, tzinfo=utc)
    n = 0
    for _ in range(2000):
        y, mo, d = rng.randrange(1, 10000), rng.randrange(1, 13), rng.randrange(1, 29)
        hh, mi, ss, us = rng.randrange(24), rng.randrange(60), rng.randrange(60), rng.randrange(10**6)
        oh, om = rng.randrange(-23, 24), rng.randrange(60)
        text = "%04d-%02d-%02dT%02d:%02d:%02d.%06d%s%02d:%02d" % (y, mo, d, hh, mi, ss, us, "-" if oh < 0 else "+", abs(oh), om)
        try:
            delta = datetime.datetime.fromisoformat(text) - epoch
        except (ValueError, OverflowError):
            continue
        want = (delta.days * 86400 + delta.seconds) * 10**6 + delta.microseconds
        assert py_timestamp(text.encode(), "us") == (CAST, want & ((1 << 64) - 1)), text
        n += 1
    assert n > 1900


@pytest.mark.parametrize("unit", ["s", "ms", "us", "ns"])
def test_timestamp_corpus(ctw, ctwin, unit):
    values = timestamp_corpus()
    data, records = window_of(values)
    outcomes = check_column(ctw, ctwin, data, records, TIMESTAMP, unit)
    assert outcomes.count(CAST) > 200 and outcomes.count(SYNTAX) > 300 and (unit != "ns" or outcomes.count(RANGE) >= 6)
    for v in values:  # the grammar on its own, without a record
        bits = ctypes.c_uint64()
        o = ctw.csm_parse_timestamp(v, len(v), UNITS[unit], ctypes.byref(bits))
        assert (o, bits.value) == py_timestamp(v, unit), v


def test_pins(ctw):
    def ts(v, unit):
        bits = ctypes.c_uint64()
        return ctw.csm_parse_timestamp(v, len(v), UNITS[unit], ctypes.byref(bits)), ctypes.c_int64(bits.value).value
    assert ts(b"0000-01-01T00:00:00Z", "s") == (CAST, -62167219200)
    assert ts(b"9999-12-31T23:59:59Z", "s") == (CAST, 253402300799)
    assert ts(b"9999-12-31T23:59:59-23:59", "us") == (CAST, (253402300799 + 86340) * 10**6)
    assert ts(b"0000-01-01T00:00:00+23:59", "ms") == (CAST, (-62167219200 - 86340) * 1000)
    assert ts(b"2262-04-11T23:47:16.854775807Z", "ns") == (CAST, (1 << 63) - 1)
    assert ts(b"1677-09-21T00:12:43.145224192Z", "ns") == (CAST, -(1 << 63))
    assert ts(b"2262-04-11T23:47:16.854775808Z", "ns")[0] == RANGE and ts(b"1677-09-21T00:12:43.145224191Z", "ns")[0] == RANGE
    assert ts(b"2024-05-01T12:34:56.789Z", "ms") == (CAST, 1714566896789) and ts(b"2024-05-01T18:04:56,7891+05:30", "ms") == (CAST, 1714566896789)
    assert ts(b"1969-12-31T23:59:59.9999Z", "ms") == (CAST, -1)   # the fraction is cut, the value floors
    assert ts(b"2024-05-01", "s") == (CAST, 1714521600) and ts(b"2016-12-31T23:59:60Z", "s")[0] == SYNTAX

    def num(v):
        bits, typ = ctypes.c_uint64(), ctypes.c_uint32()
        return ctw.csm_parse_number(v, len(v), ctypes.byref(bits), ctypes.byref(typ)), bits.value, chr(typ.value)
    assert num(b"9007199254740993") == (CAST, 9007199254740993, "l") and num(b"-0") == (CAST, 0, "l")
    assert num(b"12.50") == (CAST, 0x4029000000000000, "d") and num(b"1e400")[0] == RANGE
    assert num(b"1 ")[0] == SYNTAX and num(b" 1")[0] == SYNTAX and num(b"+1")[0] == SYNTAX and num(b"")[0] == SYNTAX and num(b"1,")[0] == SYNTAX
    assert num(b"1" * 128)[0] == RANGE and num(b"1" * 129)[0] == SYNTAX and num(b"0." + b"3" * 126)[0] == CAST


def test_escaped_twins(ctw, ctwin):
    rng = random.Random(3)
    for kind, values in ((TIMESTAMP, timestamp_corpus()), (NUMBER, number_corpus())):
        accepted = [v for v in values if py_value(v, kind, "ns")[0] == CAST]
        assert len(accepted) > 100
        bodies = escaped_twins(accepted[::3], rng)
        data, records = window_of(bodies)
        outcomes = check_column(ctw, ctwin, data, records, kind, "ns" if kind == TIMESTAMP else "s")
        assert outcomes.count(CAST) >= 3 * outcomes.count(SYNTAX) - 3 > 0   # three twins accepted per NUL twin refused
    # "2024-05-01" is 2024-05-01; a body of 6 * 35 raw bytes is read, one of 6 * 35 + 1 is not
    long35 = b"2024-05-01T12:34:56.123456789+05:30"
    all_escaped = b"".join(b"\\u%04x" % c for c in long35)
    data, records = window_of([b"\\u0032024-05-01", all_escaped, all_escaped + b"0", b"\\u0031" * 128, b"\\u0031" * 129, b"1" * 127 + b"\\u0031",
                               b"1" * 128 + b"\\u0031"])
    assert check_column(ctw, ctwin, data, records, TIMESTAMP, "s")[:3] == [CAST, CAST, SYNTAX]
    assert check_column(ctw, ctwin, data, records, NUMBER, "s")[3:] == [RANGE, SYNTAX, RANGE, SYNTAX]


def test_number_corpus(ctw, ctwin):
    values = number_corpus()
    data, records = window_of(values)
    outcomes = check_column(ctw, ctwin, data, records, NUMBER, "s")
    assert min(outcomes.count(x) for x in (CAST, SYNTAX, RANGE)) > 5


def tag_records(data_len):
    """Every tag, a number without bits, every kind of code, spans at and past the window's end"""
    recs = [rec(5, "l", token=3), rec(tnm.struct.unpack("<Q", tnm.struct.pack("<d", 1.5))[0], "d", token=4), rec(0, "l", NO_BITS, token=5),
            rec(0, "d", NO_BITS, token=6), rec(7, "{", token=7), rec(9, "[", token=8), rec(0, "t", token=9), rec(0, "f", token=10),
            rec(0, "n", token=11), rec(0, None, 0, 20, 0xFFFFFFFF), rec(0, None, 0, 17, 0xFFFFFFFF), rec(0, None, 0, 9, 0xFFFFFFFF),
            rec(123, "l", 64, 3, 77), rec(2 | (10 << 32), '"', 0, 5, 1)]
    for b, r in ((data_len - 10, 10), (data_len - 10, 11), (data_len - 1, 1), (data_len, 0), (data_len, 1), (data_len + 1, 0),
                 (0xFFFFFFFF, 0), (0xFFFFFFFF, 0xFFFFFFFF), (0, 0xFFFFFFFF), (2, 0)):
        recs.append(rec(b | (r << 32), '"', token=20))
        recs.append(rec(b | (r << 32), '"', ESCAPED, token=21))
    return np.concatenate(recs)


@pytest.mark.parametrize("kind", [TIMESTAMP, NUMBER])
@pytest.mark.parametrize("flags", [0, KEEP_NUMBERS])
def test_tags_codes_and_spans(ctw, ctwin, kind, flags):
    data = b'["2024-05-01","12.5"]2024-05-01'
    records = tag_records(len(data))
    outcomes = check_column(ctw, ctwin, data, records, kind, "s", flags)
    assert outcomes[:4] == ([CAST] * 4 if flags else [OTHER] * 4) and outcomes[9:14] == [PASSED] * 5
    got = twin_cast(ctw, data, records, kind, "s", flags)
    assert int(got.sel.n_no_bits) == (3 if flags else 1)    # the two kept numbers without bits, and the passed record's flag
    # the same records against a window one byte shorter: the last body leaves it
    check_column(ctw, ctwin, data, records, kind, "s", flags, length=len(data) - 1)


def test_results_and_capacity(ctw, ctwin):
    data, records = window_of([b"2024-05-01", b"x", b"2024-05-02T00:00"])
    n = len(records)
    flags = TIMESTAMP | 1 << 8
    got = twin_cast(ctw, data, records, TIMESTAMP, "ms", capacity=n - 1)
    assert got.summary() == ((MSJ_CAPACITY, flags, n, 0, 0, 0, 0), (MSJ_CAPACITY, 0, 0, 1, 0, 0, 0)) and got.untouched(0)
    got = twin_cast(ctw, data, records, TIMESTAMP, "ms", R=1 << 31, capacity=1 << 32, room=0)
    assert got.summary()[0] == (MSJ_CAPACITY, flags, 1 << 31, 0, 0, 0, 0)
    got = twin_cast(ctw, data, records, TIMESTAMP, "ms", sel_code=5)
    assert got.summary() == ((5, flags, 0, 0, 0, 0, 0), (5, 0, 0, 1, 0, 0, 0)) and got.untouched(0)
    got = twin_cast(ctw, data, records, TIMESTAMP, "ms", R=0)
    assert got.summary() == ((0, flags, 0, 0, 0, 0, 0), (0, 0, 0, 1, 0, 0, 0)) and got.untouched(0)
    got = twin_cast(ctw, data, records, TIMESTAMP, "ms", R=2, capacity=n + 3)
    assert got.summary()[0] == (0, flags, 2, 1, 1, 0, 0) and got.untouched(2)
    a, b = twin_cast(ctw, data, records, TIMESTAMP, "ms"), twin_cast(ctw, data, records, TIMESTAMP, "ms", in_place=True)
    assert a.summary() == b.summary() and bytes(a.out) == bytes(b.out)
    for kind, unit, fl in ((0, 0, 0), (3, 0, 0), (TIMESTAMP, 4, 0), (NUMBER, 1, 0), (NUMBER, 0, 2), (TIMESTAMP, 0, 2)):
        sel = tcm.select_result(n)
        res, out = _lib.MsjCastStringsResult(), np.zeros(16 * n, dtype=np.uint8)
        assert ctw.csm_cast_strings(data, len(data), records.ctypes.data, ctypes.byref(sel), kind, unit, fl, out.ctypes.data, n, ctypes.byref(res),
                                    None) == -1


def format_instant(rng, secs, ns):
    """One instant (seconds since the epoch within years 0001..9999, nanoseconds) through a random formatter ->
    (text, the digits of the fraction it kept)"""
    oh, om = rng.choice([(0, 0), (5, 30), (-8, 0), (23, 59), (-23, -59), (1, 0)])
    local = secs + oh * 3600 + om * 60
    days, rem = divmod(local, 86400)
    date = datetime.date.fromordinal(days + 719163)
    digits = rng.randrange(0, 10)
    text = "%04d-%02d-%02d%s%02d:%02d:%02d" % (date.year, date.month, date.day, rng.choice("Tt "), rem // 3600, rem // 60 % 60, rem % 60)
    if digits:
        text += rng.choice(".,") + ("%09d" % ns)[:digits]
    if (oh, om) == (0, 0):
        text += rng.choice(["Z", "z", "", "+00:00", "-00", "+0000"])
    else:
        sign = "-" if oh < 0 else "+"
        text += sign + "%02d" % abs(oh) + rng.choice([":", ""]) + "%02d" % abs(om) if om or rng.random() < 0.5 else sign + "%02d" % abs(oh)
    return text.encode(), digits


def test_random_instants_round_trip(ctw, ctwin):
    rng = random.Random(2024)
    lo, hi = py_days(1, 1, 3) * 86400, py_days(9999, 12, 29) * 86400
    values, want = [], []
    for _ in range(3000):
        secs, ns = rng.randrange(lo, hi), rng.randrange(10**9)
        text, digits = format_instant(rng, secs, ns)
        values.append(text)
        want.append(secs * 10**9 + ns // 10**(9 - digits) * 10**(9 - digits))
    for unit in UNITS:
        data, records = window_of(values)
        check_column(ctw, ctwin, data, records, TIMESTAMP, unit)
        outs = twin_cast(ctw, data, records, TIMESTAMP, unit).records()
        for k, w in enumerate(want):
            v = w // (10**9 // PER_SECOND[unit])
            if -(1 << 63) <= v < (1 << 63):
                assert int(outs[k]["bits"]) == v & ((1 << 64) - 1) and int(outs[k]["code"]) == 0, (values[k], unit)
            else:
                assert int(outs[k]["code"]) == NUMBER_ERROR, (values[k], unit)


def damaged(rng, values, count):
    out = []
    for _ in range(count):
        v = bytearray(rng.choice(values))
        i = rng.randrange(len(v))
        how = rng.randrange(3)
        c = rng.choice(b"0123456789-+:.,TtZz eE\x00x/")
        if how == 0:
            v[i] = c
        elif how == 1:
            v.insert(i, c)
        else:
            del v[i]
        out.append(bytes(v))
    return out


def test_damaged_texts(ctw, ctwin):
    rng = random.Random(77)
    for kind, corpus in ((TIMESTAMP, timestamp_corpus()), (NUMBER, number_corpus())):
        good = [v for v in corpus if v and py_value(v, kind, "ns")[0] == CAST]
        values = damaged(rng, good, 400)
        data, records = window_of(values)
        for unit in (("ms", "ns") if kind == TIMESTAMP else ("s",)):
            outcomes = check_column(ctw, ctwin, data, records, kind, unit)
            assert outcomes.count(SYNTAX) > 100 and outcomes.count(CAST) > 20


def mixed_corpus(kind):
    """The accept / reject corpus of a kind as raw bodies, escaped twins among them, with records of every other sort: what
    tests/test_cast_strings.py runs as one column on the device"""
    values = timestamp_corpus() if kind == TIMESTAMP else number_corpus()
    rng = random.Random(19)
    accepted = [v for v in values if v and py_value(v, kind, "ns")[0] == CAST]
    bodies = values + escaped_twins(accepted[::5], rng) + damaged(rng, accepted, 100)
    rng.shuffle(bodies)
    data, records = window_of(bodies)
    extra = tag_records(len(data))
    records = np.concatenate([records, extra])
    order = list(range(len(records)))
    rng.shuffle(order)
    return data, np.ascontiguousarray(records[order])


@pytest.mark.parametrize("kind", [TIMESTAMP, NUMBER])
def test_mixed_corpus(ctw, ctwin, kind):
    data, records = mixed_corpus(kind)
    for flags in (0, KEEP_NUMBERS):
        outcomes = check_column(ctw, ctwin, data, records, kind, "ns" if kind == TIMESTAMP else "s", flags)
        assert all(outcomes.count(x) > 0 for x in (PASSED, CAST, SYNTAX, RANGE, OTHER))
