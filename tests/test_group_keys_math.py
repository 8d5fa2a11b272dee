"""CPU check of the arithmetic of msj_bucket_rows_device and msj_group_keys_device (mojo_simdjson_amd/csrc/group_keys_math.h).

The host twin (tests/group_keys_math_host.cpp: the header's floor, part encoders and decode, the bucket call serially and the
keys call block by block as the kernel goes) runs over hand-made records and codes.  The yardstick is the definition of
include/msj_stage1.h written in Python and knows nothing of the header: a bucket is
``origin + ((floor(Fraction(v)) - origin) // width) * width``; a key is never computed here at all -- what is asserted is
what the header promises of it: ``sorted(rows, key=bytes)`` is ``sorted`` by ``(null, Fraction)`` per part, two keys are equal
iff all their parts are the same real (or null in both), and the decode of a part is the canonical form of the value that
went in.  Exact, so no case and no row is exempt.  Every array at its exact size with the fill behind each capacity.  The
kernels that run the same header on the device are covered by tests/test_group_keys.py (-m gpu); arrays from anywhere by
tests/test_group_keys_sanitizers.py.
"""
import ctypes
import itertools
import math
import os
import random
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import test_aggregate_math as tam
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
FILL = 0xA5
NUMBER, CODE, NULL_IS_GROUP = _lib.KEY_NUMBER, _lib.KEY_CODE, _lib.KEY_NULL_IS_GROUP
PART_BYTES = {NUMBER: 11, CODE: 5}
NUMBER_ERROR, INCORRECT_TYPE = 9, 17
NO_TOKEN = 0xFFFFFFFF
PASSED, BUCKETED, RANGE, SKIPPED, OTHER = range(5)   # group_keys_math.h: what became of one record
L, D = tam.L, tam.D
MASK = tam.MASK
INT64_MAX, INT64_MIN = tam.INT64_MAX, tam.INT64_MIN
Raw, records, record, double_bits, bits_double = tam.Raw, tam.records, tam.record, tam.double_bits, tam.bits_double
HOSTILE = tam.HOSTILE

_twin = None


def load_twin():
    """The host twin of the two calls (g++ build of tests/group_keys_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libgroup_keys_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "group_keys_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, i64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("gkm_floor_of_double", [u64, vp, vp], i32),
                            ("gkm_bucket_floor", [i64, i64, i64, vp], i32),
                            ("gkm_bucket_record", [vp, i64, i64, vp], u32),
                            ("gkm_encode_number", [vp, vp], i32),
                            ("gkm_encode_code", [i32, vp], i32),
                            ("gkm_decode_number", [vp, vp, vp], i32),
                            ("gkm_decode_code", [vp, vp], i32),
                            ("gkm_part_width", [u32], u32),
                            ("gkm_bucket_rows", [vp, vp, i64, i64, u32, vp, u64, vp, vp], i32),
                            ("gkm_group_keys", [vp, u32, u64, vp, vp, vp, vp, u64, u64, vp], i32)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def gtw():
    return load_twin()


# ---- the yardstick: the definition ------------------------------------------------------------------------------------------

def py_real(rec):
    """The value of a record tuple as a Fraction; None: no number value; "skipped": an 'l' / 'd' without usable bits"""
    v = tam.py_value(tuple(int(x) for x in rec))
    return Fraction(v[1]) if isinstance(v, tuple) else v


def py_bucket(rec, width, origin):
    """-> (the output record tuple, the outcome)"""
    rec = tuple(int(x) for x in rec)
    if rec[4] != 0:
        return rec, PASSED
    v = py_real(rec)
    if v is None:
        return (0, NO_TOKEN, 0, 0, INCORRECT_TYPE), OTHER
    error = (0, NO_TOKEN, 0, 0, NUMBER_ERROR)
    if v == "skipped":
        return error, SKIPPED
    f = math.floor(v)
    s = origin + ((f - origin) // width) * width
    if not (INT64_MIN <= f <= INT64_MAX) or s < INT64_MIN:
        return error, RANGE
    assert s <= INT64_MAX
    return (s & MASK, rec[1], L, 0, 0), BUCKETED


def py_canonical(v):
    """What a NUMBER part decodes to: an integer inside int64 is that int, anything else the float"""
    f = Fraction(v)
    if f.denominator == 1 and INT64_MIN <= f.numerator <= INT64_MAX:
        return int(f.numerator)
    return float(v)


def select_result(R, code=0):
    s = _lib.MsjSelectDocumentsResult()
    s.code, s.n_documents, s.n_paths = code, R, 1
    return s


class Bucketed:
    """What one bucket call left: rc, the records with the fill behind them (FIELD_DTYPE), the two results"""

    def __init__(self, rc, out, res, out_sel):
        self.rc, self.out, self.res, self.out_sel = rc, out, res, out_sel


def twin_bucket(gtw, rows, R, width, origin=0, flags=0, capacity=None, sel_code=0, in_place=False):
    rows = np.ascontiguousarray(rows, dtype=FIELD_DTYPE)
    capacity = len(rows) if capacity is None else capacity
    out = rows.copy() if in_place else np.frombuffer(bytes([FILL]) * (16 * capacity), dtype=FIELD_DTYPE).copy()
    src = out if in_place else rows
    sel, res, out_sel = select_result(R, sel_code), _lib.MsjBucketRowsResult(), _lib.MsjSelectDocumentsResult()
    rc = gtw.gkm_bucket_rows(src.ctypes.data if capacity else None, ctypes.addressof(sel), width, origin, flags, out.ctypes.data if capacity else None,
                             capacity, ctypes.addressof(res), ctypes.addressof(out_sel))
    return Bucketed(rc, out, res, out_sel)


def py_bucket_rows(rows, R, width, origin):
    """-> (the R output tuples, (n_bucketed, n_range, n_skipped, n_other), n_no_bits)"""
    out, counts, no_bits = [], [0, 0, 0, 0], 0
    for k in range(R):
        o, outcome = py_bucket(rows[k], width, origin)
        out.append(o)
        if outcome != PASSED:
            counts[outcome - 1] += 1
        no_bits += bool(o[3] & tam.NO_BITS)
    return out, tuple(counts), no_bits


def check_bucket(b, rows, R, width, origin, capacity, in_place=False):
    """A bucket call's outputs, whole, against the definition"""
    assert b.rc == 0 and b.res.code == 0 and b.res.flags == 0 and b.res.n_rows == R
    want, counts, no_bits = py_bucket_rows(rows, R, width, origin)
    got = [tuple(int(x) for x in r) for r in b.out[:R]]
    assert got == want
    assert (b.res.n_bucketed, b.res.n_range, b.res.n_skipped, b.res.n_other) == counts
    s = b.out_sel
    assert (s.code, s.flags, s.n_documents, s.n_paths, s.n_found, s.n_no_bits, s.reserved) == (0, 0, R, 1, counts[0], no_bits, 0)
    behind = b.out[R:capacity].tobytes()
    assert behind == (rows[R:capacity].tobytes() if in_place else bytes([FILL]) * len(behind))


class Part:
    """One column of a key: FIELD_DTYPE records (NUMBER) or int32 codes (CODE), with the part's flags"""

    def __init__(self, column, flags=0):
        column = np.ascontiguousarray(column)
        self.kind = NUMBER if column.dtype == FIELD_DTYPE else CODE
        self.column = column if self.kind == NUMBER else column.astype(np.int32)
        self.flags = flags

    @property
    def width(self):
        return PART_BYTES[self.kind]


def part_array(parts, pointers):
    arr = (_lib.MsjKeyPart * max(len(parts), 1))()
    for j, (p, ptr) in enumerate(zip(parts, pointers)):
        arr[j].d_column, arr[j].kind, arr[j].flags = ptr, p.kind, p.flags
    return arr


class Keys:
    """What one keys call left: rc, the three arrays with the fill behind them, the result"""

    def __init__(self, rc, offsets, valid, data, res):
        self.rc, self.offsets, self.valid, self.bytes, self.res = rc, offsets, valid, data, res


def twin_keys(gtw, parts, R, capacity=None, bytes_capacity=None, sel_code=0):
    stride = len(parts[0].column)
    W = sum(p.width for p in parts)
    capacity = stride if capacity is None else capacity
    bytes_capacity = capacity * W if bytes_capacity is None else bytes_capacity
    offsets = np.full(capacity + 1, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    valid = np.full(capacity, FILL, dtype=np.uint8)
    data = helpers_aligned(bytes_capacity)
    arr = part_array(parts, [p.column.ctypes.data if stride else None for p in parts])
    sel, res = select_result(R, sel_code), _lib.MsjGroupKeysResult()
    rc = gtw.gkm_group_keys(arr, len(parts), stride, ctypes.addressof(sel), offsets.ctypes.data, valid.ctypes.data if capacity else None,
                            data.ctypes.data if capacity else None, capacity, bytes_capacity, ctypes.addressof(res))
    return Keys(rc, offsets, valid, data, res)


def helpers_aligned(n):
    """uint8[n] filled, at a 16-byte aligned address"""
    raw = np.full(n + 16, FILL, dtype=np.uint8)
    at = (-raw.ctypes.data) % 16
    return raw[at:at + n]


def key_rows(k, R, W):
    return [k.bytes[i * W:(i + 1) * W].tobytes() for i in range(R)]


def part_value(p, k):
    """Row k of a part as the definition sees it: (null, the real or the code)"""
    if p.kind == CODE:
        c = int(p.column[k])
        return (1, 0) if c < 0 else (0, c)
    v = py_real(p.column[k])
    return (0, v) if isinstance(v, Fraction) else (1, 0)


def check_keys(k, parts, R, capacity, bytes_capacity):
    """A keys call's outputs, whole, against what the header promises of them"""
    W = sum(p.width for p in parts)
    assert k.rc == 0 and k.res.code == 0 and k.res.flags == 0
    assert (k.res.n_rows, k.res.key_width, k.res.bytes_len) == (R, W, R * W)
    assert k.offsets[:R + 1].tolist() == [i * W for i in range(R + 1)]
    assert (k.offsets[R + 1:] == 0xA5A5A5A5A5A5A5A5).all() and (k.valid[R:] == FILL).all() and (k.bytes[R * W:] == FILL).all()
    assert len(k.bytes) == bytes_capacity and len(k.valid) == capacity
    rows = key_rows(k, R, W)
    values = [tuple(part_value(p, i) for p in parts) for i in range(R)]
    valid = [int(all(not null or (p.flags & NULL_IS_GROUP) for p, (null, _) in zip(parts, v))) for v in values]
    assert k.valid[:R].tolist() == valid
    assert k.res.n_keys == sum(valid) and k.res.n_null_rows == sum(any(null for null, _ in v) for v in values)
    # the order of the bytes is the order of the parts, and equal bytes are equal parts: the two sorts agree on every tie too
    by_bytes = sorted(range(R), key=lambda i: rows[i])
    by_value = sorted(range(R), key=lambda i: values[i])
    assert by_bytes == by_value
    assert [rows[a] == rows[b] for a, b in zip(by_bytes, by_bytes[1:])] == [values[a] == values[b] for a, b in zip(by_value, by_value[1:])]
    return rows


def decode_key(gtw, parts_kinds, key):
    """The parts of one key's bytes: an int / float, a code, or None"""
    out, at = [], 0
    for kind in parts_kinds:
        buf = (ctypes.c_uint8 * PART_BYTES[kind]).from_buffer_copy(key[at:at + PART_BYTES[kind]])
        if kind == NUMBER:
            t, b = ctypes.c_uint32(), ctypes.c_uint64()
            ok = gtw.gkm_decode_number(buf, ctypes.byref(t), ctypes.byref(b))
            out.append(None if not ok else (b.value - (1 << 64) if b.value >> 63 else b.value) if t.value == L else bits_double(b.value))
        else:
            c = ctypes.c_int32()
            out.append(c.value if gtw.gkm_decode_code(buf, ctypes.byref(c)) else None)
        at += PART_BYTES[kind]
    return tuple(out)


# ---- buckets ----------------------------------------------------------------------------------------------------------------

EXTREME_INTS = [INT64_MIN, INT64_MIN + 1, INT64_MIN + 59999, -(2**53) - 1, -(2**53), -(2**53) + 1, -60001, -60000, -59999, -2, -1, 0, 1, 2, 59999, 60000,
                60001, 2**53 - 1, 2**53, 2**53 + 1, INT64_MAX - 1, INT64_MAX]
EXTREME_DOUBLES = [-0.0, 0.0, 0.5, -0.5, 1.5, -1.5, 2.0**63, -(2.0**63), math.nextafter(2.0**63, 0), math.nextafter(-(2.0**63), 0),
                   math.nextafter(-(2.0**63), -math.inf), 2.0**53 - 1, 2.0**53, 2.0**53 + 2, -(2.0**53) - 2, -(2.0**53), -(2.0**53) + 1, 2.0**64, 1e300, -1e300,
                   5e-324, -5e-324, 2.0**-1022, 59999.999, -59999.999, -60000.0, 1e18, -1e18, 9.2e18, -9.2e18]
WIDTHS = [1, 2, 7, 60000, 2**62, 2**63 - 1]
ORIGINS = [INT64_MIN, INT64_MIN + 1, -60001, -1, 0, 1, 30000, INT64_MAX - 1, INT64_MAX]


def test_bucket_extremes(gtw):
    """Every extreme value under every width and origin, through the whole call: int64 extremes, doubles at +-2^63, +-2^53 +- 1
    and +-0.5, -0.0, widths 1, 60 000 and 2^63 - 1, origins at both ends; and every record that is no number value"""
    token = 0
    values = []
    for v in EXTREME_INTS + EXTREME_DOUBLES + HOSTILE + tam.ODD_VALUES:
        token += 3
        r = list(record(v))
        r[1] = token
        values.append(tuple(r))
    rows = np.array(values, dtype=FIELD_DTYPE)
    outcomes = set()
    for width, origin in itertools.product(WIDTHS, ORIGINS):
        b = twin_bucket(gtw, rows, len(rows), width, origin)
        check_bucket(b, rows, len(rows), width, origin, len(rows))
        outcomes |= {py_bucket(r, width, origin)[1] for r in rows}
    assert outcomes == {PASSED, BUCKETED, RANGE, SKIPPED, OTHER}


def test_bucket_pinned(gtw):
    """The floor is no truncation: below the origin the bucket lies to the left"""
    def one(v, width, origin=0):
        b = twin_bucket(gtw, records([v]), 1, width, origin)
        check_bucket(b, records([v]), 1, width, origin, 1)
        bits = int(b.out[0]["bits"])
        return (bits - (1 << 64) if bits >> 63 else bits) if b.out[0]["code"] == 0 else None
    assert one(-1, 60000) == -60000 and one(-60000, 60000) == -60000 and one(-60001, 60000) == -120000
    assert one(59999, 60000) == 0 and one(60000, 60000) == 60000
    assert one(-0.5, 1) == -1 and one(-0.0, 1) == 0 and one(0.5, 1) == 0
    assert one(7, 5, 2) == 7 and one(6, 5, 2) == 2 and one(1, 5, 2) == -3
    assert one(INT64_MIN, 2**63 - 1, 0) is None            # -(2^63 - 1) * 2 lies below int64
    assert one(INT64_MIN, 2**63 - 1, -1) == INT64_MIN      # origin - width
    assert one(INT64_MAX, 2**63 - 1, INT64_MIN) == INT64_MAX - 1
    assert one(INT64_MAX, 1, INT64_MIN) == INT64_MAX
    assert one(2.0**63, 1) is None and one(-(2.0**63), 1) == INT64_MIN and one(-(2.0**63), 3) is None


def test_bucket_random(gtw):
    rng = random.Random(5)

    def any_int():
        return rng.choice([rng.randint(INT64_MIN, INT64_MAX), rng.randint(-10**6, 10**6), INT64_MIN + rng.randint(0, 99), INT64_MAX - rng.randint(0, 99)])
    for _ in range(20000):
        f, origin = any_int(), any_int()
        width = rng.choice([rng.randint(1, INT64_MAX), rng.randint(1, 10**6), INT64_MAX - rng.randint(0, 9)])
        s = ctypes.c_int64()
        ok = gtw.gkm_bucket_floor(f, width, origin, ctypes.byref(s))
        want = origin + ((f - origin) // width) * width
        assert (s.value if ok else None) == (want if want >= INT64_MIN else None), (f, width, origin)
    for _ in range(20000):
        bits = rng.getrandbits(64)
        x = bits_double(bits)
        if not math.isfinite(x):
            continue
        f, whole = ctypes.c_int64(), ctypes.c_int32()
        ok = gtw.gkm_floor_of_double(bits, ctypes.byref(f), ctypes.byref(whole))
        want = math.floor(Fraction(x))
        assert bool(ok) == (INT64_MIN <= want <= INT64_MAX), x
        if ok:
            assert f.value == want and bool(whole.value) == (Fraction(x).denominator == 1), x


def test_bucket_sizes_and_refusals(gtw):
    rows = records([5, -5, 2.5, Raw(1, '"'), Raw(3, "l", code=20)] * 60)
    for R in (0, 1, 255, 256, 257):
        check_bucket(twin_bucket(gtw, rows, R, 3, 1), rows, R, 3, 1, len(rows))
        check_bucket(twin_bucket(gtw, rows, R, 3, 1, in_place=True), rows, R, 3, 1, len(rows), in_place=True)
    b = twin_bucket(gtw, rows, 300, 3, capacity=299)
    assert b.rc == 0 and (b.res.code, b.res.n_rows, b.res.n_bucketed) == (MSJ_CAPACITY, 300, 0) and b.out.tobytes() == bytes([FILL]) * (16 * 299)
    assert (b.out_sel.code, b.out_sel.n_documents, b.out_sel.n_found) == (MSJ_CAPACITY, 0, 0)
    b = twin_bucket(gtw, rows, 300, 3, sel_code=7)
    assert b.rc == 0 and (b.res.code, b.res.n_rows) == (7, 0) and b.out.tobytes() == bytes([FILL]) * (16 * 300)
    assert twin_bucket(gtw, rows, 10, 0).rc == BAD_ARGUMENT and twin_bucket(gtw, rows, 10, -1).rc == BAD_ARGUMENT
    assert twin_bucket(gtw, rows, 10, 1, flags=1).rc == BAD_ARGUMENT


# ---- keys -------------------------------------------------------------------------------------------------------------------

KEY_VALUES = [0, -0.0, 0.0, 3, 3.0, -3, -3.0, 9007199254740992.0, 9007199254740993, 9007199254740994.0, 9007199254740992, -9007199254740993,
              -9007199254740992.0, -9007199254740994.0, INT64_MAX, INT64_MIN, 2.0**63, -(2.0**63), INT64_MAX - 1, INT64_MIN + 1, 0.5, -0.5, 5e-324,
              -5e-324, 1e300, -1e300, 1, 2, 200, 200.0, 2e2, 1.5, 60000, -60000]


def test_number_part_order_equality_decode(gtw):
    """One NUMBER part over every value and every record kind of msj_field: the triple around 2^53, 3 / 3.0, -0.0 / 0, codes 17
    and 20, strings, NO_BITS, NaN bits"""
    col = records(KEY_VALUES + HOSTILE + tam.ODD_VALUES + [Raw(0, 0, code=17), Raw(0, 0, code=20)])
    R = len(col)
    for flags in (0, NULL_IS_GROUP):
        parts = [Part(col, flags)]
        rows = check_keys(twin_keys(gtw, parts, R), parts, R, R, 11 * R)
        for i in range(R):
            v = py_real(col[i])
            got = decode_key(gtw, [NUMBER], rows[i])[0]
            if isinstance(v, Fraction):
                want = py_canonical(v)
                assert type(got) is type(want) and got == want and rows[i][0] == 0, (col[i], got)
            else:
                assert got is None and rows[i] == b"\x01" + bytes(10)
    at = {repr(v): rows[i] for i, v in enumerate(KEY_VALUES)}
    assert at["9007199254740992.0"] < at["9007199254740993"] < at["9007199254740994.0"] and at["9007199254740992.0"] == at["9007199254740992"]
    assert at["3"] == at["3.0"] and at["-0.0"] == at["0"] == at["0.0"] and at["200"] == at["200.0"]


def test_code_part(gtw):
    codes = np.array([0, 1, 255, 256, 65536, 2**31 - 1, -1, -2, -(2**31), 7, 7], dtype=np.int32)
    R = len(codes)
    for flags in (0, NULL_IS_GROUP):
        parts = [Part(codes, flags)]
        rows = check_keys(twin_keys(gtw, parts, R), parts, R, R, 5 * R)
        assert rows[2] == bytes([0, 0, 0, 0, 255]) and rows[5] == bytes([0, 0x7F, 0xFF, 0xFF, 0xFF]) and rows[6] == bytes([1, 0, 0, 0, 0])
        assert [decode_key(gtw, [CODE], r)[0] for r in rows] == [int(c) if c >= 0 else None for c in codes]


def random_parts(rng, kinds, stride, flags=None):
    parts = []
    for j, kind in enumerate(kinds):
        f = rng.choice([0, NULL_IS_GROUP]) if flags is None else flags[j]
        if kind == NUMBER:
            parts.append(Part(records([rng.choice(KEY_VALUES[:12] + HOSTILE[:3]) for _ in range(stride)]), f))
        else:
            parts.append(Part(np.array([rng.choice([-1, 0, 1, 2, 300, 70000]) for _ in range(stride)], dtype=np.int32), f))
    return parts


# W: 5, 10, 11, 16, 21, 55, 88, and every number of parts from 1 to 8
KIND_LISTS = [[CODE], [CODE, CODE], [NUMBER], [NUMBER, CODE], [CODE, NUMBER, CODE], [NUMBER] * 5, [NUMBER] * 8, [CODE] * 4, [CODE, NUMBER] * 3,
              [NUMBER, CODE, CODE, NUMBER, CODE, CODE, CODE]]


def test_kind_lists_cover_the_widths():
    assert [sum(PART_BYTES[k] for k in ks) for ks in KIND_LISTS[:7]] == [5, 10, 11, 16, 21, 55, 88]
    assert sorted({len(ks) for ks in KIND_LISTS}) == [1, 2, 3, 4, 5, 6, 7, 8]


@pytest.mark.parametrize("kinds", KIND_LISTS, ids=lambda ks: "".join("n" if k == NUMBER else "c" for k in ks))
def test_keys_lexicographic(gtw, kinds):
    rng = random.Random(len(kinds) * 31 + sum(kinds))
    W = sum(PART_BYTES[k] for k in kinds)
    for R in (0, 1, 255, 256, 257):
        stride = R + 2
        parts = random_parts(rng, kinds, stride)
        check_keys(twin_keys(gtw, parts, R), parts, R, stride, stride * W)
        # every array at its exact size
        k = twin_keys(gtw, parts, R, capacity=R, bytes_capacity=R * W)
        rows = check_keys(k, parts, R, R, R * W)
        for i in range(0, R, 37):
            got = decode_key(gtw, kinds, rows[i])
            want = tuple(None if null else (py_canonical(v) if p.kind == NUMBER else v) for p, (null, v) in ((p, part_value(p, i)) for p in parts))
            assert got == want and [type(a) for a in got] == [type(b) for b in want]


def test_keys_capacity_and_refusals(gtw):
    rng = random.Random(3)
    parts = random_parts(rng, [CODE, NUMBER], 300)
    W = 16

    def untouched(k):
        return (k.offsets == 0xA5A5A5A5A5A5A5A5).all() and (k.valid == FILL).all() and (k.bytes == FILL).all()
    for kw in (dict(capacity=256), dict(bytes_capacity=257 * W - 1)):
        k = twin_keys(gtw, parts, 257, **kw)
        assert k.rc == 0 and (k.res.code, k.res.n_rows, k.res.n_keys, k.res.n_null_rows, k.res.key_width, k.res.bytes_len) == (MSJ_CAPACITY, 257, 0, 0, W, 0)
        assert untouched(k)
    k = twin_keys(gtw, parts, 301)   # R > stride
    assert k.res.code == MSJ_CAPACITY and untouched(k)
    k = twin_keys(gtw, parts, 10, sel_code=9)
    assert (k.res.code, k.res.n_rows) == (9, 0) and untouched(k)
    sel, res = select_result(1), _lib.MsjGroupKeysResult()
    a = part_array(parts, [p.column.ctypes.data for p in parts])
    call = lambda arr, n, stride=300, cap=0: gtw.gkm_group_keys(arr, n, stride, ctypes.addressof(sel), None, None, None, cap, 0, ctypes.addressof(res))
    assert call(a, 2) == 0 and res.code == MSJ_CAPACITY
    assert call(None, 2) == BAD_ARGUMENT and call(a, 0) == BAD_ARGUMENT and call(a, 9) == BAD_ARGUMENT
    a[1].kind = 3
    assert call(a, 2) == BAD_ARGUMENT
    a[1].kind, a[1].flags = NUMBER, 2
    assert call(a, 2) == BAD_ARGUMENT
    a[1].flags, a[1].d_column = 0, None
    assert call(a, 2) == BAD_ARGUMENT and call(a, 2, stride=0) == 0
    a[1].d_column = parts[1].column.ctypes.data
    assert call(a, 2, cap=1) == BAD_ARGUMENT
    a[1].d_column = parts[1].column.ctypes.data + 8
    assert call(a, 2) == BAD_ARGUMENT
