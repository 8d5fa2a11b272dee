"""CPU check of the arithmetic of msj_aggregate_device (mojo_simdjson_amd/csrc/aggregate_math.h).

The host twin (tests/aggregate_math_host.cpp: the header's value test, exponents, limbs, 128-bit recombination, final rounding
and min / max rule, serially) runs over hand-made records.  The yardstick is the definition of include/msj_stage1.h written
in Python and knows nothing of the header: ``fractions.Fraction`` for every value, ``int`` for t = trunc(v * 2^(95 - E)) and
for S, and Python's correctly rounded ``int / int`` for the one rounding.  Minimum and maximum are ``min`` / ``max`` over
(the value as a Fraction, the tie rank).  Every array at its exact size with the fill behind each capacity.  The kernels that
run the same header on the device are covered by tests/test_aggregate.py (-m gpu); arrays from anywhere by
tests/test_aggregate_sanitizers.py.
"""
import ctypes
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE
from tests import helpers
from tests import test_string_column_math as tcm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
FILL = 0xA5
NO_BITS = 64
INT_OVERFLOW, INFINITE = 1, 2
INT64_MAX, INT64_MIN = 2**63 - 1, -2**63
MASK = (1 << 64) - 1
L, D = ord("l"), ord("d")
AGG_DTYPE = np.dtype([("n_rows", "<u8"), ("n_values", "<u8"), ("sum_bits", "<u8"), ("min_bits", "<u8"), ("max_bits", "<u8"),
                      ("sum_type", "u1"), ("min_type", "u1"), ("max_type", "u1"), ("flags", "u1"), ("reserved", "<u4")])  # msj_aggregate
assert AGG_DTYPE.itemsize == 48

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/aggregate_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libaggregate_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "aggregate_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, i64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("agm_value_kind", [vp], u32),
                            ("agm_exp_key", [u32, u64], u32),
                            ("agm_value_limbs", [u32, u64, u32, vp], None),
                            ("agm_int_limbs", [i64, vp], None),
                            ("agm_recombine", [i64, i64, i64, vp, vp], None),
                            ("agm_round_scaled", [u64, i64, i32, vp], u64),
                            ("agm_replaces", [i32, u32, u64, u32, u64], i32),
                            ("agm_aggregate", [vp, u64, u32, vp, vp, u64, vp, u64, vp, ctypes.c_int], ctypes.c_int)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def atw():
    return load_twin()


# ---- records ----------------------------------------------------------------------------------------------------------------

def double_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def bits_double(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


class Raw:
    """A record spelled out: what is no plain number value"""

    def __init__(self, bits, type, flags=0, code=0):
        self.t = (bits & MASK, 0, type if isinstance(type, int) else ord(type), flags, code)


def record(v):
    """(bits, token, type, flags, code) of an int (an 'l'), a float (a 'd') or a Raw"""
    if isinstance(v, Raw):
        return v.t
    if isinstance(v, int):
        assert INT64_MIN <= v <= INT64_MAX
        return (v & MASK, 0, L, 0, 0)
    return (double_bits(v), 0, D, 0, 0)


def records(values):
    return np.array([record(v) for v in values], dtype=FIELD_DTYPE)


HOSTILE = [Raw(5, '"'), Raw(5, "t"), Raw(7, 0), Raw(7, 0xFF), Raw(3, "l", code=20), Raw(double_bits(2.5), "d", code=9), Raw(9, "l", NO_BITS),
           Raw(double_bits(1.5), "d", NO_BITS), Raw(double_bits(math.inf), "d"), Raw(double_bits(-math.inf), "d"), Raw(0x7FF8000000000001, "d"),
           Raw(0xFFF0000000000001, "d"), Raw(4, "{"), Raw(4, "[", NO_BITS)]
# ... and what looks odd and IS a value: an int64 has no NaN, and MSJ_SPAN_ESCAPED means nothing on a number
ODD_VALUES = [Raw(double_bits(math.inf), "l"), Raw(1, "l", 2)]


# ---- the yardstick: the definition ------------------------------------------------------------------------------------------

def py_value(rec):
    """None, "skipped", or (tag, the value as int / float) of a record tuple"""
    bits, _, type, flags, code = rec
    if code != 0 or type not in (L, D):
        return None
    if flags & NO_BITS:
        return "skipped"
    if type == L:
        return (L, bits - (1 << 64) if bits >> 63 else bits)
    x = bits_double(bits)
    return (D, x) if math.isfinite(x) else "skipped"


def floor_log2(f):
    """floor(log2 f) of a positive Fraction"""
    e = f.numerator.bit_length() - f.denominator.bit_length()
    return e if Fraction(2) ** e <= f else e - 1


def round_once(f):
    """(the pattern of the binary64 nearest to the Fraction f, ties to even; beyond DBL_MAX?)"""
    try:
        x = f.numerator / f.denominator   # int / int: correctly rounded
    except OverflowError:
        return double_bits(math.inf if f > 0 else -math.inf), True
    if f < 0 and x == 0:
        x = -0.0
    return double_bits(x), False


def py_sum(vals):
    """(tag, bits, flags) of a group's values [(tag, value)], at least one"""
    all_int = all(t == L for t, _ in vals)
    if all_int and INT64_MIN <= sum(v for _, v in vals) <= INT64_MAX:
        return L, sum(v for _, v in vals) & MASK, 0
    flags = INT_OVERFLOW if all_int else 0
    fr = [Fraction(v) for _, v in vals if v != 0]
    if not fr:
        return D, 0, flags
    E = max(floor_log2(abs(f)) for f in fr)
    S = sum(math.trunc(f * Fraction(2) ** (95 - E)) for f in fr)
    assert abs(S) < 1 << 127
    if S == 0:
        return D, 0, flags
    bits, infinite = round_once(Fraction(S) * Fraction(2) ** (E - 95))
    return D, bits, flags | (INFINITE if infinite else 0)


def raw_bits(t, v):
    return v & MASK if t == L else double_bits(v)


def py_min_max(vals):
    negative_zero = lambda t, v: t == D and v == 0 and math.copysign(1, v) < 0
    # between equal reals the 'l' wins; among doubles -0.0 lies below +0.0
    lo = min(vals, key=lambda tv: (Fraction(tv[1]), 0 if tv[0] == L else 1 if negative_zero(*tv) else 2))
    hi = max(vals, key=lambda tv: (Fraction(tv[1]), 2 if tv[0] == L else 0 if negative_zero(*tv) else 1))
    return lo[0], raw_bits(*lo), hi[0], raw_bits(*hi)


def py_group(recs):
    """The msj_aggregate of a group's record tuples, as an AGG_DTYPE tuple, and its skipped records"""
    kinds = [py_value(r) for r in recs]
    vals = [k for k in kinds if isinstance(k, tuple)]
    skipped = sum(k == "skipped" for k in kinds)
    if not vals:
        return (len(recs), 0, 0, 0, 0, 0, 0, 0, 0, 0), skipped
    st, sb, flags = py_sum(vals)
    lt, lb, ht, hb = py_min_max(vals)
    return (len(recs), len(vals), sb, lb, hb, st, lt, ht, flags, 0), skipped


def py_aggregate(columns, R, codes, G):
    """columns: FIELD_DTYPE of shape (n_columns, stride).  -> (AGG_DTYPE array of shape (n_columns, G), the result's
    (flags, n_rows, n_groups, n_ungrouped, n_values, n_skipped))"""
    group = [0 if codes is None else int(codes[k]) for k in range(R)]
    rows = [[] for _ in range(G)]
    for k, g in enumerate(group):
        if 0 <= g < G:
            rows[g].append(k)
    out = np.zeros((len(columns), G), dtype=AGG_DTYPE)
    flags = n_values = n_skipped = 0
    for c, col in enumerate(columns):
        for g in range(G):
            rec, skipped = py_group([tuple(int(x) for x in col[k]) for k in rows[g]])
            out[c, g] = rec
            flags |= rec[8]
            n_values += rec[1]
            n_skipped += skipped
    return out, (flags, R, G, R - sum(len(r) for r in rows), n_values, n_skipped)


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Agg:
    """What one call left: rc, the record bytes with the fill (uint8), the 48-byte result"""

    def __init__(self, rc, groups, res, n_columns, capacity):
        self.rc, self.groups, self.res, self.n_columns, self.capacity = rc, groups, res, n_columns, capacity

    def records(self, G):
        return self.groups.view(AGG_DTYPE).reshape(self.n_columns, self.capacity)[:, :G]

    def result(self):
        r = self.res
        return (r.flags, r.n_rows, r.n_groups, r.n_ungrouped, r.n_values, r.n_skipped)


def as_columns(columns):
    columns = np.ascontiguousarray(columns, dtype=FIELD_DTYPE)
    return columns.reshape(1, -1) if columns.ndim == 1 else columns


def twin_aggregate(atw, columns, R, codes, G, capacity=None, sel_code=0, split=0):
    """agm_aggregate over `columns` (FIELD_DTYPE, (n_columns, stride) or one column) -> Agg"""
    columns = as_columns(columns)
    n_columns, stride = columns.shape
    capacity = G if capacity is None else capacity
    groups = np.full(n_columns * capacity * 48, FILL, dtype=np.uint8)
    sel = tcm.select_result(R, sel_code)
    res = _lib.MsjAggregateResult()
    codes = None if codes is None else np.ascontiguousarray(codes, dtype=np.int32)
    assert codes is None or len(codes) == stride
    rc = atw.agm_aggregate(columns.ctypes.data, stride, n_columns, ctypes.addressof(sel), None if codes is None else codes.ctypes.data, G,
                           groups.ctypes.data, capacity, ctypes.addressof(res), split)
    return Agg(rc, groups, res, n_columns, capacity)


def one_group(atw, values, split=0):
    """The record of the values as one ungrouped column, as a tuple"""
    a = twin_aggregate(atw, records(values), len(values), None, 1, split=split)
    assert a.rc == 0 and a.res.code == 0
    return tuple(int(x) for x in a.records(1)[0, 0])


def check_group(atw, values):
    want, _ = py_group([record(v) for v in values])
    for split in (0, 1):
        assert one_group(atw, values, split) == want, (values, split)
    return want


# ---- the pinned cases (tests/test_aggregate.py places them in a block's first and last row) -----------------------------------

CASES = {
    "cancel": [1e308, -1e308, 1.0],
    "tenths": [0.1] * 10,
    "past_2_53": [float(2**53), 1.0, 1.0],
    "int_round_trip": [INT64_MAX, 1, -1],
    "int_overflow": [INT64_MAX, 1],
    "int_min_twice": [INT64_MIN, INT64_MIN],
    "int_cut_by_1e30": [12345678901234567, 1e30],
    "subnormals": [5e-324] * 3,
    "subnormals_less_one": [5e-324] * 3 + [-5e-324],
    "infinite": [1.7e308, 1.7e308],
    "minus_infinite": [-1.7e308, -1.7e308, 3],
    "negative_zero": [-0.0],
    "zeros": [-0.0, 0, 0.0],
    "zeros_doubles": [0.0, -0.0, 0.0],
    "int_beside_double": [9007199254740993, 9007199254740992.0],
    "double_beside_int": [9007199254740992.0, 9007199254740993, 9007199254740992],
    "hostile": HOSTILE,
    "hostile_and_values": HOSTILE[:8] + [3, -2.5] + HOSTILE[8:],
    "nothing": [],
}


def test_pinned_cases(atw):
    d = double_bits
    got = {name: check_group(atw, values) for name, values in CASES.items()}
    # n_rows, n_values, sum, min, max, the three tags, flags, reserved
    # E = 1023: a last place of 2^928 cuts the 1.0 to t = 0, and the two large terms cancel exactly.  (A left-to-right double
    # sum of this order gives 1.0, of another order 0.0; the definition gives +0.0 for every order.)
    assert got["cancel"] == (3, 3, d(0.0), d(-1e308), d(1e308), D, D, D, 0, 0)
    assert got["tenths"] == (10, 10, d(1.0), d(0.1), d(0.1), D, D, D, 0, 0) and sum([0.1] * 10) != 1.0
    assert got["past_2_53"][2] == d(9007199254740994.0) and float(2**53) + 1.0 + 1.0 == float(2**53)
    assert got["int_round_trip"] == (3, 3, INT64_MAX, MASK, INT64_MAX, L, L, L, 0, 0)
    assert got["int_overflow"] == (2, 2, d(9223372036854775808.0), 1, INT64_MAX, D, L, L, INT_OVERFLOW, 0)
    assert got["int_min_twice"] == (2, 2, d(-2.0**64), 1 << 63, 1 << 63, D, L, L, INT_OVERFLOW, 0)
    # E = 99: the int is cut to a multiple of 2^4, 12345678901234560, before it is added
    assert got["int_cut_by_1e30"][2] == round_once(Fraction(1e30) + 12345678901234560)[0] != d(1e30)
    assert got["int_cut_by_1e30"][5] == D and got["int_cut_by_1e30"][8] == 0
    assert got["subnormals"][2] == d(1.5e-323) and got["subnormals_less_one"][2] == d(1e-323)
    assert got["infinite"] == (2, 2, d(math.inf), d(1.7e308), d(1.7e308), D, D, D, INFINITE, 0)
    assert got["minus_infinite"][2] == d(-math.inf) and got["minus_infinite"][8] == INFINITE
    assert got["negative_zero"] == (1, 1, 0, d(-0.0), d(-0.0), D, D, D, 0, 0)
    assert got["zeros"] == (3, 3, 0, 0, 0, D, L, L, 0, 0)
    assert got["zeros_doubles"] == (3, 3, 0, d(-0.0), 0, D, D, D, 0, 0)
    assert got["int_beside_double"] == (2, 2, d(18014398509481984.0), d(9007199254740992.0), 9007199254740993, D, D, L, 0, 0)
    assert got["double_beside_int"][3:8] == (9007199254740992, 9007199254740993, D, L, L)
    assert got["hostile"] == (len(HOSTILE), 0, 0, 0, 0, 0, 0, 0, 0, 0)
    assert got["hostile_and_values"] == (len(HOSTILE) + 2, 2, d(0.5), d(-2.5), 3, D, D, L, 0, 0)
    assert got["nothing"] == (0,) * 10


def test_value_kind_and_counts(atw):
    kinds = [atw.agm_value_kind(records([h]).ctypes.data) for h in HOSTILE]
    # code 0 and a number's tag, but NO_BITS or bits that are not finite: skipped (2); everything else: no number (0)
    assert kinds == [0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2, 0, 0]
    assert [atw.agm_value_kind(records([h]).ctypes.data) for h in ODD_VALUES] == [1, 1]
    assert check_group(atw, ODD_VALUES)[:3] == (2, 2, 0x7FF0000000000001)
    col = records(HOSTILE[:12] + [1, 2.0])
    codes = np.array([0, 1, -1, 2, -(2**31), 0, 1, 0, 1, 5, 0, 1, 1, 0], dtype=np.int32)
    a = twin_aggregate(atw, col, len(col), codes, 2)
    want, res = py_aggregate(as_columns(col), len(col), codes, 2)
    assert a.rc == 0 and a.res.code == 0 and np.array_equal(a.records(2), want) and a.result() == res
    assert res == (0, 14, 2, 4, 2, 5)


def test_exponents_and_limbs(atw):
    rng = random.Random(7)
    for _ in range(4000):
        if rng.random() < 0.5:
            v = rng.choice([1, -1]) * rng.getrandbits(rng.randrange(1, 64))
            v = max(INT64_MIN, min(INT64_MAX, v)) if rng.random() < 0.9 else rng.choice([INT64_MIN, INT64_MAX, 0])
            type, bits, f = L, v & MASK, Fraction(v)
        else:
            bits = rng.getrandbits(64) if rng.random() < 0.8 else rng.getrandbits(52) | (rng.getrandbits(1) << 63)
            if (bits >> 52) & 0x7FF == 0x7FF:
                continue
            type, f = D, Fraction(bits_double(bits))
        key = atw.agm_exp_key(type, bits)
        if f == 0:
            assert key == 0
            continue
        e = floor_log2(abs(f))
        assert key == e + 1075
        E = e + rng.choice([0, 0, 1, 5, 31, 32, 33, 43, 52, 53, 63, 64, 95, 96, 97, 200, rng.randrange(0, 2200)])
        if E > 1023:
            continue
        limbs = (ctypes.c_int64 * 3)()
        atw.agm_value_limbs(type, bits, E + 1075, limbs)
        t = math.trunc(f * Fraction(2) ** (95 - E))
        assert all(abs(x) < 1 << 32 and (x == 0 or (x < 0) == (f < 0)) for x in limbs)
        assert limbs[0] + (limbs[1] << 32) + (limbs[2] << 64) == t, (type, bits, E)
        if type == L:
            two = (ctypes.c_int64 * 2)()
            atw.agm_int_limbs(bits - (1 << 64) if bits >> 63 else bits, two)
            assert 0 <= two[0] < 1 << 32 and -(1 << 31) <= two[1] < 1 << 31 and two[0] + (two[1] << 32) == f


def twin_recombine(atw, a0, a1, a2):
    lo, hi = ctypes.c_uint64(), ctypes.c_int64()
    atw.agm_recombine(a0, a1, a2, ctypes.byref(lo), ctypes.byref(hi))
    return lo.value, hi.value


def test_recombine(atw):
    rng = random.Random(11)
    edge = [0, 1, -1, 2**62, -(2**62), 2**63 - 1, -(2**63) + 1, 2**32, -(2**32), 2**31 * (2**32 - 1), -(2**31) * (2**32 - 1)]
    for _ in range(3000):
        a = [rng.choice(edge) if rng.random() < 0.4 else rng.randrange(-(2**63) + 1, 2**63) for _ in range(3)]
        a[2] = a[2] >> rng.choice([0, 2, 33])    # (|S| < 2^127 where fewer than 2^31 rows made it)
        S = a[0] + (a[1] << 32) + (a[2] << 64)
        if not -(1 << 127) <= S < 1 << 127:
            continue
        lo, hi = twin_recombine(atw, *a)
        assert (hi << 64) + lo == S, a


def twin_round(atw, S, scale):
    inf = ctypes.c_uint32()
    bits = atw.agm_round_scaled(S & MASK, S >> 64, scale, ctypes.byref(inf))
    return bits, bool(inf.value)


def test_rounding_from_S(atw):
    d = double_bits
    # ties to even at the 53rd bit: 2^53 + 1 lies between 2^53 (even) and 2^53 + 2; 2^53 + 3 between + 2 and + 4 (even)
    assert twin_round(atw, 2**53 + 1, 0) == (d(9007199254740992.0), False)
    assert twin_round(atw, 2**53 + 3, 0) == (d(9007199254740996.0), False)
    assert twin_round(atw, -(2**53 + 1), 0) == (d(-9007199254740992.0), False)
    assert twin_round(atw, (2**53 + 1) << 40, -40) == (d(9007199254740992.0), False)
    assert twin_round(atw, ((2**53 + 1) << 40) + 1, -40) == (d(9007199254740994.0), False)   # (above the tie by one part in 2^94)
    assert twin_round(atw, (2**53 + 1) << 70, 0) == (d(2.0**123), False)
    # a carry out of the significand; the largest finite; the first step beyond it
    assert twin_round(atw, 2**54 - 1, 0) == (d(2.0**54), False)
    assert twin_round(atw, (2**53 - 1) << 42, 971 - 42) == (d(1.7976931348623157e308), False)
    assert twin_round(atw, ((2**53 - 1) << 42) + (1 << 41) - 1, 971 - 42) == (d(1.7976931348623157e308), False)
    assert twin_round(atw, ((2**53 - 1) << 42) + (1 << 41), 971 - 42) == (d(math.inf), True)
    assert twin_round(atw, -(1 << 126), 928) == (d(-math.inf), True)
    # subnormals: the last place is 2^-1074 whatever the leading bit; a tie between 0 and the smallest goes to 0 (even)
    assert twin_round(atw, 3, -1074) == (3, False) and twin_round(atw, 3, -1075) == (2, False) and twin_round(atw, 1, -1075) == (0, False)
    assert twin_round(atw, -1, -1075) == (1 << 63, False) and twin_round(atw, 5, -1076) == (1, False) and twin_round(atw, 1, -1169) == (0, False)
    assert twin_round(atw, (1 << 52) - 1, -1074) == ((1 << 52) - 1, False) and twin_round(atw, (1 << 53) - 1, -1075) == (1 << 52, False)
    assert twin_round(atw, 0, 5) == (0, False)
    rng = random.Random(13)
    for _ in range(6000):
        S = rng.choice([1, -1]) * (rng.getrandbits(rng.randrange(1, 128)) | rng.getrandbits(1) << rng.randrange(0, 127))
        if rng.random() < 0.3:    # on and around a tie
            keep = rng.randrange(1, 60)
            S = ((S >> keep) << keep) + rng.choice([-1, 0, 1]) + (1 << (keep - 1))
        if S == 0 or abs(S) >= 1 << 127:
            continue
        scale = rng.randrange(-1169, 929) if rng.random() < 0.5 else rng.choice([-1169, -1100, -1074, -1022, -95, 0, 800, 928])
        assert twin_round(atw, S, scale) == round_once(Fraction(S) * Fraction(2) ** scale), (S, scale)


def random_value(rng, centre):
    """A value of any size; centre: an exponent most of a group's doubles stay near, so that the sums see carries and
    cancellation and not only one large term"""
    r = rng.random()
    if r < 0.30:
        v = rng.choice([1, -1]) * rng.getrandbits(rng.randrange(1, 64))
        return max(INT64_MIN, min(INT64_MAX, v))
    if r < 0.36:
        return rng.choice([0, 0.0, -0.0, INT64_MAX, INT64_MIN, 1, -1, 5e-324, -5e-324, 2.2250738585072014e-308, 1.7976931348623157e308, -1.7976931348623157e308])
    if r < 0.40:
        return rng.choice(HOSTILE)
    e = rng.randrange(1, 2047) if rng.random() < 0.3 else max(0, min(2046, centre + rng.randrange(-60, 4)))
    return bits_double(rng.getrandbits(52) | e << 52 | rng.getrandbits(1) << 63)


def random_groups(seed, n_groups, most=12):
    """(values row by row, their codes): n_groups groups of mixed records, the rows shuffled"""
    rng = random.Random(seed)
    rows = []
    for g in range(n_groups):
        centre = rng.randrange(0, 2047)
        kind = rng.random()
        for _ in range(rng.randrange(1, most + 1)):
            v = random_value(rng, centre)
            if kind < 0.2 and not isinstance(v, Raw):      # a group of ints alone: the int path and its overflow
                v = int(max(INT64_MIN, min(INT64_MAX, v))) if isinstance(v, int) or abs(v) < 1e300 else INT64_MAX
            rows.append((g, v))
    rng.shuffle(rows)
    return [v for _, v in rows], np.array([g for g, _ in rows], dtype=np.int32)


def test_random_groups(atw):
    G = 2000
    values, codes = random_groups(2024, G)
    col = records(values)
    want, res = py_aggregate(as_columns(col), len(col), codes, G)
    tags = want["sum_type"][0]
    assert (tags == L).sum() > 100 and (tags == D).sum() > 1000 and (want["flags"][0] & INT_OVERFLOW).any() and (want["flags"][0] & INFINITE).any()
    for split in (0, 1):
        a = twin_aggregate(atw, col, len(col), codes, G, split=split)
        assert a.rc == 0 and a.res.code == 0
        got = a.records(G)
        bad = np.nonzero(got[0] != want[0])[0]
        assert bad.size == 0, (split, int(bad[0]), got[0][bad[0]], want[0][bad[0]], [v for v, g in zip(values, codes) if g == bad[0]])
        assert a.result() == res


def test_order_does_not_matter(atw):
    values, codes = random_groups(5, 300)
    col = records(values)
    first = twin_aggregate(atw, col, len(col), codes, 300, split=1)
    rng = random.Random(6)
    for _ in range(3):
        perm = list(range(len(col)))
        rng.shuffle(perm)
        again = twin_aggregate(atw, col[perm], len(col), codes[perm], 300, split=1)
        assert np.array_equal(first.groups, again.groups) and first.result() == again.result()


def test_codes_and_capacities(atw):
    values = [1, 2.5, 3, -4, 5.5, 6, Raw(1, "l", NO_BITS), 8]
    col = np.stack([records(values), records(list(reversed(values)))])
    codes = np.array([-1, 0, 2, 3, 2**31 - 1, -(2**31), 1, 2], dtype=np.int32)
    for G in (0, 1, 2, 3, 4):
        a = twin_aggregate(atw, col, 8, codes, G, capacity=5)
        want, res = py_aggregate(col, 8, codes, G)
        assert a.rc == 0 and a.res.code == 0 and np.array_equal(a.records(G), want) and a.result() == res
        assert (a.groups.reshape(2, 5, 48)[:, G:] == FILL).all()     # nothing at or past G
    # rows beyond R are not read as rows; R == 0 leaves zeroed records
    a = twin_aggregate(atw, col, 3, codes, 3)
    want, res = py_aggregate(col, 3, codes, 3)
    assert np.array_equal(a.records(3), want) and a.result() == res == (0, 3, 3, 1, 3, 1)
    a = twin_aggregate(atw, col, 0, codes, 3)
    assert a.res.code == 0 and not a.groups.any() and a.result() == (0, 0, 3, 0, 0, 0)
    # over: the rows, the groups; a code in the select result
    for R, G, cap in ((9, 2, 2), (8, 3, 2)):
        a = twin_aggregate(atw, col, R, codes, G, capacity=cap)
        assert a.rc == 0 and a.res.code == MSJ_CAPACITY and a.result() == (0, R, G, 0, 0, 0) and (a.groups == FILL).all()
    a = twin_aggregate(atw, col, 8, codes, 2, sel_code=7)
    assert a.res.code == 7 and a.result() == (0, 0, 0, 0, 0, 0) and (a.groups == FILL).all()
    assert twin_aggregate(atw, np.zeros((17, 1), dtype=FIELD_DTYPE), 1, None, 1).rc == -1


def test_merge_rule(atw):
    """replaces(want, new, old) against the yardstick's order: (the value as a Fraction, the tie rank)"""
    rng = random.Random(17)
    pool = [0, 0.0, -0.0, 1, 1.0, -1, -1.0, 9007199254740993, 9007199254740992.0, 9007199254740994.0, INT64_MAX, 9223372036854775808.0,
            INT64_MIN, -9223372036854775808.0, -9223372036854777856.0, 0.5, -0.5, 5e-324, -5e-324, 1.7976931348623157e308]
    pool += [rng.choice([1, -1]) * rng.getrandbits(rng.randrange(1, 64)) for _ in range(20)]
    pool += [float(v) for v in pool if isinstance(v, int)] + [bits_double(rng.getrandbits(63) % (0x7FF << 52) | rng.getrandbits(1) << 63) for _ in range(20)]
    tagged = [(L if isinstance(v, int) else D, v) for v in pool]
    for a in tagged:
        for b in tagged:
            lo_first, hi_first = py_min_max([b, a])[:2], py_min_max([b, a])[2:]     # (min and max keep the first of two that are the same)
            takes_min = (a[0], raw_bits(*a)) == lo_first and (a[0], raw_bits(*a)) != (b[0], raw_bits(*b))
            takes_max = (a[0], raw_bits(*a)) == hi_first and (a[0], raw_bits(*a)) != (b[0], raw_bits(*b))
            assert bool(atw.agm_replaces(-1, a[0], raw_bits(*a), b[0], raw_bits(*b))) == takes_min, (a, b)
            assert bool(atw.agm_replaces(1, a[0], raw_bits(*a), b[0], raw_bits(*b))) == takes_max, (a, b)
