"""CPU check of the arithmetic of msj_sort_rows_device (mojo_simdjson_amd/csrc/sort_rows_math.h).

The host twin (tests/sort_rows_math_host.cpp: the header's value test and key, and a serial stable sort of the keys) runs
over hand-made records.  The yardstick is the definition of include/msj_stage1.h written in Python and knows nothing of the
header: ``sorted(range(N), key=lambda j: (no_value(j), +-Fraction(value(j))))`` -- Python's sort is stable -- and then
``[:K]``.  It is exact, so no case and no row is exempt, and every comparison is over all the rows.  Every array at its exact
size with the fill behind each capacity.  The kernels that run the same header on the device are covered by
tests/test_sort_rows.py (-m gpu); arrays from anywhere by tests/test_sort_rows_sanitizers.py.
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
from tests import test_string_column_math as tcm
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
FILL = 0xA5
FILL32 = 0xA5A5A5A5
DESC, VALUES_ONLY = 1, 2
L, D = tam.L, tam.D
INT64_MAX, INT64_MIN = tam.INT64_MAX, tam.INT64_MIN
Raw, records, record, double_bits = tam.Raw, tam.records, tam.record, tam.double_bits
HOSTILE = tam.HOSTILE

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/sort_rows_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libsort_rows_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "sort_rows_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("srm_value_kind", [vp], u32),
                            ("srm_key", [vp, u32, vp], None),
                            ("srm_digit", [u64, u64, u32], u32),
                            ("srm_aux", [u64, u64, u64], u64),
                            ("srm_takes_selection", [u32, u64, u64], i32),
                            ("srm_passes", [vp, u64, u32], u32),
                            ("srm_sort_rows", [vp, u64, vp, vp, vp, u32, u64, vp, u64, vp, vp], i32)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def stw():
    return load_twin()


# ---- the yardstick: the definition ------------------------------------------------------------------------------------------

def py_value(rec):
    """The value of a record tuple as a Fraction, None for a row without one, and whether it counts as skipped"""
    v = tam.py_value(tuple(int(x) for x in rec))
    if isinstance(v, tuple):
        return Fraction(v[1]), False
    return None, v == "skipped"


def py_sort(col, R, rows_in=None, N=None, flags=0, limit=0):
    """-> (the first K row numbers of the order, (n_rows, n_values, n_written, n_skipped, n_out_of_range), the rows compared)"""
    seq = list(range(R)) if rows_in is None else [int(r) for r in rows_in[:N]]
    vals, skipped, out_of_range = [], 0, 0
    for row in seq:
        if row >= R:
            vals.append(None)
            out_of_range += 1
            continue
        v, s = py_value(col[row])
        vals.append(v)
        skipped += s
    sign = -1 if flags & DESC else 1
    order = sorted(range(len(seq)), key=lambda j: (vals[j] is None, 0 if vals[j] is None else sign * vals[j]))
    n_values = sum(v is not None for v in vals)
    M = n_values if flags & VALUES_ONLY else len(seq)
    K = M if limit == 0 else min(limit, M)
    return [seq[j] for j in order[:K]], (len(seq), n_values, K, skipped, out_of_range), len(order)


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Sorted:
    """What one call left: rc, d_order with the fill (uint32), the 48-byte result, d_order_select"""

    def __init__(self, rc, order, res, order_sel):
        self.rc, self.order, self.res, self.order_sel = rc, order, res, order_sel

    def rows(self):
        return [int(x) for x in self.order[:self.res.n_written]]

    def counts(self):
        r = self.res
        return (r.n_rows, r.n_values, r.n_written, r.n_skipped, r.n_out_of_range)

    def untouched(self):
        return bool((self.order[self.res.n_written:] == FILL32).all())


def order_room(capacity, limit):
    return min(capacity, limit) if limit else capacity


def twin_sort(stw, col, R, rows_in=None, N=None, flags=0, limit=0, capacity=None, sel_code=0, in_code=0, order_select=True):
    """srm_sort_rows over `col` (FIELD_DTYPE, one column; its length is the stride) -> Sorted"""
    col = np.ascontiguousarray(col, dtype=FIELD_DTYPE)
    stride = len(col)
    sel = tcm.select_result(R, sel_code)
    in_sel = None
    if rows_in is not None:
        rows_in = np.ascontiguousarray(rows_in, dtype=np.uint32)
        N = len(rows_in) if N is None else N
        in_sel = tcm.select_result(N, in_code)
    if capacity is None:
        capacity = len(rows_in) if rows_in is not None else stride
    order = np.full(order_room(capacity, limit), FILL32, dtype=np.uint32)
    res = _lib.MsjSortRowsResult()
    ctypes.memset(ctypes.addressof(res), FILL, 48)
    order_sel = tcm.select_result(0x5A5A, 0x5A) if order_select else None
    rc = stw.srm_sort_rows(col.ctypes.data if stride else None, stride, ctypes.addressof(sel), None if rows_in is None else rows_in.ctypes.data,
                           None if in_sel is None else ctypes.addressof(in_sel), flags, limit, order.ctypes.data if len(order) else None, capacity,
                           ctypes.addressof(res), None if order_sel is None else ctypes.addressof(order_sel))
    return Sorted(rc, order, res, order_sel)


def check_sort(stw, col, R, rows_in=None, N=None, flags=0, limit=0, capacity=None):
    """The twin against the definition -> the twin's Sorted"""
    got = twin_sort(stw, col, R, rows_in, N, flags, limit, capacity)
    want, counts, compared = py_sort(col, R, rows_in, N, flags, limit)
    assert got.rc == 0 and got.res.code == 0 and got.res.flags == flags
    assert compared == counts[0]     # every row took part
    assert got.counts() == counts, (got.counts(), counts)
    assert got.rows() == want
    assert got.untouched()
    s = got.order_sel
    assert (s.code, s.n_documents, s.n_paths, s.n_found, s.n_no_bits) == (0, counts[2], 1, counts[2], 0)
    return got


# ---- the key ----------------------------------------------------------------------------------------------------------------

def twin_key(stw, v, flags=0):
    out = (ctypes.c_uint64 * 3)()
    stw.srm_key(records([v]).ctypes.data, flags, out)
    return (out[2], out[0], out[1])     # (null, hi, lo): compared as tuples


PINNED = ([0.0, -0.0, 0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 3, 3.0, -3, -3.0]
          + [s * v for s in (1, -1) for v in (2**53, 2**53 + 1)] + [s * float(v) for s in (1, -1) for v in (2**53, 2**53 + 2)]
          + [float(2**62), float(2**62 + 1024), INT64_MIN, INT64_MAX, 2.0**63, -(2.0**63), 9007199254740993, 9007199254740992.0, 9007199254740994.0]
          + [2**62 + k for k in range(2048)])


def check_pairs(stw, values):
    keys = [twin_key(stw, v) for v in values]
    desc = [twin_key(stw, v, DESC) for v in values]
    reals = [Fraction(v) for v in values]
    assert all(k[0] == 0 and k[2] < 1024 for k in keys + desc)
    return keys, desc, reals


def test_key_order_on_the_pinned_list(stw):
    """Key order is Fraction order and key equality is real equality, over ALL pairs, in both directions"""
    keys, desc, reals = check_pairs(stw, PINNED)
    r, n = reals, len(PINNED)
    # all pairs through a sort of each side: the ranks with ties must agree
    rank = lambda xs: {x: i for i, x in enumerate(sorted(set(xs)))}
    rr, rk, rd = rank(r), rank(keys), rank(desc)
    assert len(rr) == len(rk) == len(rd)
    top = len(rr) - 1
    for j in range(n):
        assert rk[keys[j]] == rr[r[j]] and rd[desc[j]] == top - rr[r[j]], PINNED[j]
    # ... and the pairs the header names, spelled out
    key = lambda v: twin_key(stw, v)
    assert key(0.0) == key(-0.0) == key(0) and key(3) == key(3.0)
    assert key(9007199254740992.0) < key(9007199254740993) < key(9007199254740994.0)
    assert key(float(2**62)) == key(2**62) < key(2**62 + 1) < key(2**62 + 1023) < key(float(2**62 + 1024)) == key(2**62 + 1024) < key(2**62 + 2047)
    assert key(INT64_MIN) == key(-(2.0**63)) < key(INT64_MIN + 1) and key(INT64_MAX) < key(2.0**63)
    assert key(-5e-324) < key(0) < key(5e-324)


def random_number(rng):
    r = rng.random()
    if r < 0.25:
        return max(INT64_MIN, min(INT64_MAX, rng.choice([1, -1]) * rng.getrandbits(rng.randrange(1, 65))))
    if r < 0.45:      # an integer next to a double above 2^53, as either
        e = rng.randrange(53, 63)
        v = rng.choice([1, -1]) * ((rng.getrandbits(53) | 1 << 52) << (e - 52)) + rng.randrange(-3, 4)
        v = max(INT64_MIN, min(INT64_MAX, v))
        return v if rng.random() < 0.5 else float(v)
    if r < 0.55:
        return rng.choice([0, 0.0, -0.0, INT64_MAX, INT64_MIN, 2.0**63, -(2.0**63), 5e-324, -5e-324, 2.2250738585072014e-308, 1, -1, 1.0])
    if r < 0.65:
        return tam.bits_double(rng.getrandbits(52) | rng.getrandbits(1) << 63)      # subnormals
    return tam.bits_double(rng.getrandbits(52) | rng.randrange(0, 2047) << 52 | rng.getrandbits(1) << 63)


def test_key_order_on_random_pairs(stw):
    rng = random.Random(41)
    for _ in range(20000):
        a, b = random_number(rng), random_number(rng)
        if rng.random() < 0.1:
            b = float(a) if isinstance(a, int) else (int(a) if abs(a) < 2**62 else a)
        fa, fb = Fraction(a), Fraction(b)
        for flags in (0, DESC):
            ka, kb = twin_key(stw, a, flags), twin_key(stw, b, flags)
            want = (fa > fb) - (fa < fb)
            assert (ka > kb) - (ka < kb) == (-want if flags else want), (a, b, flags)


def test_rows_without_a_value(stw):
    kinds = [stw.srm_value_kind(records([h]).ctypes.data) for h in HOSTILE]
    assert kinds == [0, 0, 0, 0, 0, 0, 2, 2, 2, 2, 2, 2, 0, 0]
    assert all(twin_key(stw, h, f) == (1, 0, 0) for h in HOSTILE for f in (0, DESC))
    assert [stw.srm_value_kind(records([h]).ctypes.data) for h in tam.ODD_VALUES] == [1, 1]
    col = records(HOSTILE[:7] + [5, -2.5] + HOSTILE[7:] + [-7])
    for flags in (0, DESC, VALUES_ONLY, DESC | VALUES_ONLY):
        got = check_sort(stw, col, len(col), flags=flags)
        assert got.counts()[1] == 3 and got.counts()[3] == 6
    got = check_sort(stw, col, len(col))
    assert got.rows()[:3] == [len(col) - 1, 8, 7] and got.rows()[3:] == [j for j in range(len(col)) if j not in (7, 8, len(col) - 1)]


def test_digits(stw):
    """The eleven digits, least significant first, put the key together again: lo, hi byte by byte, the null bit"""
    rng = random.Random(3)
    for _ in range(300):
        hi, lo, null, pos = rng.getrandbits(64), rng.getrandbits(10), rng.getrandbits(1), rng.getrandbits(31)
        aux = stw.srm_aux(lo, null, pos)
        assert aux & 0x7FFFFFFF == pos
        d = [stw.srm_digit(hi, aux, x) for x in range(11)]
        assert d[0] | d[1] << 8 == lo and sum(d[2 + i] << 8 * i for i in range(8)) == hi and d[10] == null and d[1] < 4


def test_passes(stw):
    """srm_passes (scripts/sort_rows_rate.py reports it): the digits that are not the same in every row"""
    def passes(values, flags=0):
        col = records(values)
        digits = []
        for v in values:
            null, hi, lo = twin_key(stw, v, flags)
            digits.append([stw.srm_digit(hi, stw.srm_aux(lo, null, 0), d) for d in range(11)])
        want = sum(len({row[d] for row in digits}) > 1 for d in range(11))
        assert stw.srm_passes(col.ctypes.data, len(col), flags) == want
        return want

    assert passes([5, 5, 5.0]) == 0 and passes([]) == 0 and passes([2**62, 2**62 + 1]) == 1 and passes([2**62, 2**62 + 256]) == 1
    assert passes([1.0, Raw(0, "n")]) >= 2 and passes(list(range(1000, 5000))) <= 3 and passes([0.5 * k for k in range(1, 3000)], DESC) <= 3
    ns = 1714521600000000000      # nanoseconds of 2024: between 2^60 and 2^61, a double's last place there is 2^8 and the low part has 8 bits
    assert passes([ns, ns + 255]) == 1 and passes([ns, ns + 256]) == 1 and passes([ns + 1000003 * k for k in range(3000)]) >= 4
    assert passes(MIXED) == 11


# ---- the whole call ---------------------------------------------------------------------------------------------------------

MIXED = [3, 3.0, -1, 2.5, Raw(0, "n"), 9007199254740993, 9007199254740992.0, 0, -0.0, 0.0, Raw(9, "l", tam.NO_BITS), -5e-324, INT64_MIN, 3, 1e300, Raw(1, '"'), 2.5,
         INT64_MAX, 9223372036854775808.0, -3]


def test_hand_made_columns(stw):
    col = records(MIXED)
    n, n_values = len(MIXED), sum(not isinstance(v, Raw) for v in MIXED)
    for flags in (0, DESC, VALUES_ONLY, DESC | VALUES_ONLY):
        M = n_values if flags & VALUES_ONLY else n
        for limit in sorted({0, 1, M - 1, M, M + 1}):
            check_sort(stw, col, n, flags=flags, limit=limit)
    asc = check_sort(stw, col, n).rows()
    assert asc[:4] == [12, 19, 2, 11] and asc[4:7] == [7, 8, 9] and asc[-3:] == [4, 10, 15]      # equal values and rows without one keep input order
    desc = check_sort(stw, col, n, flags=DESC).rows()
    assert desc[:3] == [14, 18, 17] and desc[-3:] == [4, 10, 15] and desc.index(0) < desc.index(1) < desc.index(13)
    # R below the stride: the records behind R are not rows
    check_sort(stw, col, 7)
    check_sort(stw, col, 0)


def test_rows_in(stw):
    col = records(MIXED)
    R = 15
    rows_in = [14, 3, 3, R, 2**32 - 1, 0, 13, 1, 12, 7, 14, R + 4, 5, 6]
    for flags in (0, DESC, VALUES_ONLY):
        for limit in (0, 1, 5, len(rows_in), 40):
            got = check_sort(stw, col, R, rows_in=rows_in, flags=flags, limit=limit)
            assert got.counts()[4] == 3
    check_sort(stw, col, R, rows_in=rows_in, N=4, capacity=len(rows_in))
    check_sort(stw, col, R, rows_in=rows_in, N=0)


def test_two_keys(stw):
    """The minor key first, its order as d_rows_in of the major key's call: sorted() with a tuple key"""
    rng = random.Random(8)
    n = 400
    major = [rng.choice([1, 2, 2.0, 3, Raw(0, "n"), 9007199254740993, 9007199254740992.0]) for _ in range(n)]
    minor = [rng.choice([rng.randrange(-5, 5), rng.random(), Raw(0, "t")]) for _ in range(n)]
    a, b = records(major), records(minor)
    key = lambda col, j, sign: (lambda v: (v is None, 0 if v is None else sign * v))(py_value(col[j])[0])
    for major_desc, minor_desc in itertools.product((0, DESC), repeat=2):
        first = check_sort(stw, b, n, flags=minor_desc)
        second = check_sort(stw, a, n, rows_in=first.rows(), flags=major_desc)
        want = sorted(range(n), key=lambda j: (key(a, j, -1 if major_desc else 1), key(b, j, -1 if minor_desc else 1)))
        assert second.rows() == want


def test_codes_and_refusals(stw):
    col = records(MIXED)
    n = len(col)
    rows_in = np.arange(n, dtype=np.uint32)[::-1].copy()
    zero = (0, 0, 0, 0, 0)
    for kw, code in ((dict(sel_code=7), 7), (dict(rows_in=rows_in, in_code=9, sel_code=7), 9), (dict(rows_in=rows_in, sel_code=7), 7)):
        got = twin_sort(stw, col, n, **kw)
        assert got.rc == 0 and got.res.code == code and got.res.flags == 0 and got.counts() == zero and (got.order == FILL32).all()
        assert (got.order_sel.code, got.order_sel.n_documents, got.order_sel.n_paths, got.order_sel.n_found) == (code, 0, 1, 0)
    for kw, N in ((dict(R=n + 1), n + 1), (dict(R=n, rows_in=rows_in, capacity=n - 1), n), (dict(R=1 << 31), 1 << 31),
                  (dict(R=n, rows_in=rows_in, N=n + 3), n + 3)):
        R = kw.pop("R")
        got = twin_sort(stw, col, R, flags=DESC, **kw)
        assert got.rc == 0 and got.res.code == MSJ_CAPACITY and got.res.flags == DESC and got.counts() == (N, 0, 0, 0, 0) and (got.order == FILL32).all()
        assert got.order_sel.code == MSJ_CAPACITY and got.order_sel.n_documents == 0
    got = twin_sort(stw, col, 0, flags=VALUES_ONLY)
    assert got.res.code == 0 and got.res.flags == VALUES_ONLY and got.counts() == zero and (got.order == FILL32).all()
    assert twin_sort(stw, col, n, order_select=False).rows() == check_sort(stw, col, n).rows()

    # what the entry point refuses, in the header's order, with nothing written
    sel, in_sel, res, out_sel = tcm.select_result(n), tcm.select_result(n), _lib.MsjSortRowsResult(), tcm.select_result(0)
    order = np.full(n + 2, FILL32, dtype=np.uint32)
    ad = ctypes.addressof

    def call(**kw):
        p = dict(col=col.ctypes.data, stride=n, sel=ad(sel), rows_in=None, in_sel=None, flags=0, limit=0, order=order.ctypes.data, cap=n, res=ad(res),
                 out_sel=ad(out_sel))
        p.update(kw)
        return stw.srm_sort_rows(p["col"], p["stride"], p["sel"], p["rows_in"], p["in_sel"], p["flags"], p["limit"], p["order"], p["cap"], p["res"],
                                 p["out_sel"])

    ctypes.memset(ad(res), FILL, 48)
    assert call(res=None) == BAD_ARGUMENT and call(sel=None) == BAD_ARGUMENT
    assert call(rows_in=rows_in.ctypes.data) == BAD_ARGUMENT and call(in_sel=ad(in_sel)) == BAD_ARGUMENT
    assert call(col=None) == BAD_ARGUMENT and call(order=None) == BAD_ARGUMENT and call(flags=4) == BAD_ARGUMENT
    assert call(stride=1 << 40, col=None) == BAD_ARGUMENT and call(cap=1 << 40, flags=8) == BAD_ARGUMENT
    assert call(stride=1 << 40, res=ad(sel)) == MSJ_CAPACITY and call(cap=1 << 40, col=col.ctypes.data + 8) == MSJ_CAPACITY
    assert call(res=ad(sel)) == BAD_ARGUMENT and call(res=ad(out_sel)) == BAD_ARGUMENT
    assert call(rows_in=rows_in.ctypes.data, in_sel=ad(in_sel), res=ad(in_sel)) == BAD_ARGUMENT
    assert call(out_sel=ad(sel)) == BAD_ARGUMENT and call(rows_in=rows_in.ctypes.data, in_sel=ad(in_sel), out_sel=ad(in_sel)) == BAD_ARGUMENT
    # d_order over d_rows_in: its first entry on the list's last; with a limit the order is shorter
    both = np.concatenate([rows_in, rows_in])
    at = lambda k: both.ctypes.data + 4 * k
    assert call(rows_in=at(0), in_sel=ad(in_sel), order=at(n - 1)) == BAD_ARGUMENT and call(rows_in=at(0), in_sel=ad(in_sel), order=at(n)) == 0
    assert call(rows_in=at(3), in_sel=ad(in_sel), order=at(0), limit=3) == 0 and call(rows_in=at(3), in_sel=ad(in_sel), order=at(0), limit=4) == BAD_ARGUMENT
    for name, base, step in (("col", col.ctypes.data, 8), ("order", order.ctypes.data, 2), ("sel", ad(sel), 4), ("res", ad(res), 4), ("out_sel", ad(out_sel), 4)):
        assert call(**{name: base + step}) == BAD_ARGUMENT, name
    assert call(rows_in=rows_in.ctypes.data + 2, in_sel=ad(in_sel)) == BAD_ARGUMENT
    assert call(rows_in=rows_in.ctypes.data, in_sel=ad(in_sel) + 4) == BAD_ARGUMENT
    assert (order == FILL32).all()
    assert call(stride=0, col=None, cap=0, order=None) == 0 and res.code == MSJ_CAPACITY and res.n_rows == n     # no room for a row
    sel0 = tcm.select_result(0)
    assert call(stride=0, col=None, cap=0, order=None, sel=ad(sel0)) == 0 and res.code == 0 and res.n_rows == 0


def test_which_path(stw):
    """The cut-over the header names: the selection for a limit of at most an eighth of at least 16 384 rows"""
    sel = stw.srm_takes_selection
    assert not sel(0, 0, 1 << 20) and not sel(0, 10, 16383) and sel(0, 10, 16384) and sel(0, 2048, 16384) and not sel(0, 2049, 16384)
    assert not sel(1, 10, 1 << 20) and sel(2, 10, 11) and sel(2, 10, 1) and not sel(2, 0, 100) and not sel(2, 5, 0)


def test_random_columns(stw):
    rng = random.Random(99)
    for round in range(60):
        n = rng.randrange(1, 300)
        vals = [rng.choice(HOSTILE) if rng.random() < 0.15 else random_number(rng) for _ in range(n)]
        if round % 3 == 0:
            vals = [rng.choice(vals[:5]) for _ in range(n)]      # many equal values
        col = records(vals)
        R = rng.choice([n, n, rng.randrange(0, n + 1)])
        rows_in = None if round % 2 else [rng.choice([rng.randrange(0, n + 3), rng.getrandbits(32)]) if rng.random() < 0.1 else rng.randrange(0, n) for _ in range(rng.randrange(0, 2 * n))]
        check_sort(stw, col, R, rows_in=rows_in, flags=rng.randrange(4), limit=rng.choice([0, 0, 1, rng.randrange(1, n + 2)]))
