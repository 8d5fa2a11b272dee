"""CPU check of the arithmetic of msj_join_rows_device (mojo_simdjson_amd/csrc/join_rows_math.h).

The host twin (tests/join_rows_math_host.cpp: the header's key test, digits, pairs per row and pair-to-row search, the call
built serially from them in the kernels' steps) runs over hand-made key columns.  The yardstick is the definition of
include/msj_stage1.h written in Python and knows nothing of the header: ``match`` is a dict of lists of right rows, INNER is
the double loop over it, and LEFT / SEMI / ANTI are derived from ``match`` as the table in the header says.  Every output is
compared over its WHOLE array, each at its exact size and pre-filled, so a write at or past M, pairs_capacity or
d_offsets[L] shows.  ``np_join`` is the same definition with numpy's stable sort for the sizes a Python loop cannot take; it
is held against the dict here and used by the GPU tests (tests/test_join_rows.py, -m gpu); arrays from anywhere are
tests/test_join_rows_sanitizers.py's.
"""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import helpers
from tests import test_string_column_math as tcm
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
INNER, LEFT, SEMI, ANTI = 0, 1, 2, 3
KINDS = (INNER, LEFT, SEMI, ANTI)
NO_ROW = 0xFFFFFFFF
FILL = 0xA5
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5
INT32_MAX, INT32_MIN = 2**31 - 1, -2**31

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/join_rows_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libjoin_rows_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "join_rows_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("jrm_is_key", [i32, u64], i32),
                            ("jrm_key_digits", [u64], u32),
                            ("jrm_key_passes", [u64], u32),
                            ("jrm_digit", [u32, u32], u32),
                            ("jrm_pairs_of_row", [u32, u64], u64),
                            ("jrm_row_of_pair", [vp, u64, u64, u64], u64),
                            ("jrm_join_rows", [i32, vp, u64, vp, vp, u64, vp, u64, vp, u64, u32, vp, vp, u64, vp, vp, vp, vp], i32)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def jtw():
    return load_twin()


# ---- the yardstick: the definition ------------------------------------------------------------------------------------------

def py_match(lk, rk, L, R, G):
    """match(l) for every left row: the right rows with its key, ascending; [] for a row without a key"""
    by_key = {}
    for r in range(R):
        if 0 <= int(rk[r]) < G:
            by_key.setdefault(int(rk[r]), []).append(r)
    return [by_key.get(int(lk[l]), []) if 0 <= int(lk[l]) < G else [] for l in range(L)]


def py_join(lk, rk, L, R, G, kind):
    """-> (left rows, right rows, offsets, (n_pairs, n_left_matched, n_left_null, n_right_null)) of the definition"""
    match = py_match(lk, rk, L, R, G)
    left, right, offsets = [], [], [0]
    for l, m in enumerate(match):
        if kind == INNER:
            pairs = [(l, r) for r in m]
        elif kind == LEFT:
            pairs = [(l, r) for r in m] or [(l, NO_ROW)]
        elif kind == SEMI:
            pairs = [(l, m[0])] if m else []
        else:
            pairs = [] if m else [(l, NO_ROW)]
        left += [p[0] for p in pairs]
        right += [p[1] for p in pairs]
        offsets.append(len(left))
    counters = (len(left), sum(1 for m in match if m), sum(1 for l in range(L) if not 0 <= int(lk[l]) < G),
                sum(1 for r in range(R) if not 0 <= int(rk[r]) < G))
    return left, right, offsets, counters


def np_join(lk, rk, L, R, G, kind):
    """The same definition for large inputs: numpy's stable sort of the right keys, searchsorted for every left key"""
    lk, rk = np.asarray(lk[:L], dtype=np.int64), np.asarray(rk[:R], dtype=np.int64)
    r_ok, l_ok = (rk >= 0) & (rk < G), (lk >= 0) & (lk < G)
    rows = np.nonzero(r_ok)[0]
    order = rows[np.argsort(rk[rows], kind="stable")]
    keys_sorted = rk[order]
    first = np.searchsorted(keys_sorted, lk, "left")
    c = np.where(l_ok, np.searchsorted(keys_sorted, lk, "right") - first, 0)
    n = {INNER: c, LEFT: np.maximum(c, 1), SEMI: (c > 0).astype(np.int64), ANTI: (c == 0).astype(np.int64)}[kind]
    offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
    left = np.repeat(np.arange(L, dtype=np.int64), n)
    within = np.arange(len(left), dtype=np.int64) - offsets[:-1].astype(np.int64)[left]
    if kind == SEMI:
        within[:] = 0
    has = (c[left] > 0) & (kind != ANTI)
    place = np.where(has, first[left] + within, 0)
    right = np.where(has, order[place] if len(order) else 0, NO_ROW)
    counters = (len(left), int((c > 0).sum()), int((~l_ok).sum()), int((~r_ok).sum()))
    return left.astype(np.uint32), right.astype(np.uint32), offsets, counters


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Joined:
    """What one call left: rc, the pair arrays and the offsets with their fill, the 64-byte result, the two select results"""

    def __init__(self, rc, left, right, offsets, res, lsel, rsel):
        self.rc, self.left, self.right, self.offsets, self.res, self.lsel, self.rsel = rc, left, right, offsets, res, lsel, rsel

    def counters(self):
        r = self.res
        return (r.n_pairs, r.n_left_matched, r.n_left_null, r.n_right_null)


def keys_array(keys, room=None):
    a = np.asarray(keys, dtype=np.int64).astype(np.int32)
    if room is not None and room > len(a):
        a = np.concatenate([a, np.full(room - len(a), 0x5A5A5A5A, dtype=np.int32)])
    return np.ascontiguousarray(a)


def _p(a):
    return None if a is None else a.ctypes.data


def twin_join(tw, lk, rk, G, kind, L=None, R=None, G_dev=None, keys_capacity=None, pairs_capacity=None, want_right=True, want_offsets=True,
              want_selects=True):
    """The twin over exact-size arrays.  lk / rk: int32 arrays whose lengths are the rooms; L / R / G_dev: the counts "on the
    device" (None: the rooms / G as the argument)"""
    left_rows, right_rows = len(lk), len(rk)
    n_l = None if L is None else np.array([L], dtype=np.uint64)
    n_r = None if R is None else np.array([R], dtype=np.uint64)
    n_g = None if G_dev is None else np.array([G_dev], dtype=np.uint64)
    keys_capacity = G if keys_capacity is None else keys_capacity
    if pairs_capacity is None:
        eff_L, eff_R = (left_rows if L is None else L), (right_rows if R is None else R)
        pairs_capacity = eff_L * max(eff_R, 1) + eff_L if eff_L <= left_rows and eff_R <= right_rows else 0
    left = np.full(pairs_capacity, FILL32, dtype=np.uint32)
    right = np.full(pairs_capacity, FILL32, dtype=np.uint32) if want_right else None
    offsets = np.full(left_rows + 1, FILL64, dtype=np.uint64) if want_offsets else None
    res = _lib.MsjJoinRowsResult()
    ctypes.memset(ctypes.byref(res), FILL, ctypes.sizeof(res))
    lsel, rsel = (tcm.select_result(0, 0), tcm.select_result(0, 0)) if want_selects else (None, None)
    for s in (lsel, rsel):
        if s is not None:
            ctypes.memset(ctypes.byref(s), FILL, ctypes.sizeof(s))
    rc = tw.jrm_join_rows(1, _p(lk) if left_rows else None, left_rows, _p(n_l), _p(rk) if right_rows else None, right_rows, _p(n_r), G, _p(n_g),
                          keys_capacity, kind, _p(left) if pairs_capacity else None, _p(right) if pairs_capacity and want_right else None,
                          pairs_capacity, _p(offsets), ctypes.addressof(res), None if lsel is None else ctypes.addressof(lsel),
                          None if rsel is None else ctypes.addressof(rsel))
    return Joined(rc, left, right, offsets, res, lsel, rsel)


def expected_arrays(want, pairs_capacity, left_rows, L, clipped=False):
    """The definition laid out as the call's arrays with their fill -> (left, right, offsets)"""
    wl, wr, wo, _ = want
    left, right = np.full(pairs_capacity, FILL32, dtype=np.uint32), np.full(pairs_capacity, FILL32, dtype=np.uint32)
    if not clipped:
        left[:len(wl)], right[:len(wr)] = np.asarray(wl, dtype=np.uint32), np.asarray(wr, dtype=np.uint32)
    offsets = np.full(left_rows + 1, FILL64, dtype=np.uint64)
    offsets[:L + 1] = np.asarray(wo, dtype=np.uint64)
    return left, right, offsets


def check(tw, lkeys, rkeys, G, kind, left_room=None, right_room=None, where=None, definition=py_join, **kw):
    """The twin against the definition over every output -> the twin's Joined"""
    L, R = len(lkeys), len(rkeys)
    lk, rk = keys_array(lkeys, left_room), keys_array(rkeys, right_room)
    if left_room is not None:
        kw["L"] = L
    if right_room is not None:
        kw["R"] = R
    got = twin_join(tw, lk, rk, G, kind, **kw)
    assert got.rc == 0, (where, got.rc)
    want = definition(lk, rk, L, R, G, kind)
    M = want[3][0]
    clipped = M > len(got.left)
    left, right, offsets = expected_arrays(want, len(got.left), len(lk), L, clipped)
    assert got.res.code == (MSJ_CAPACITY if clipped else 0), (where, got.res.code)
    assert (got.res.flags, got.res.n_left, got.res.n_right, got.res.n_keys) == (kind, L, R, kw.get("G_dev", G) if kw.get("G_dev") is not None else G), where
    assert got.counters() == want[3], (where, got.counters(), want[3])
    assert np.array_equal(got.left, left), (where, "left rows")
    if got.right is not None:
        assert np.array_equal(got.right, right), (where, "right rows")
    if got.offsets is not None:
        assert np.array_equal(got.offsets, offsets), (where, "offsets")
    for s in (got.lsel, got.rsel):
        if s is not None:
            assert (s.code, s.n_documents, s.n_found, s.n_paths, s.n_no_bits, s.flags) == (got.res.code, M, M, 1, 0, 0), where
    return got


# ---- the pieces ---------------------------------------------------------------------------------------------------------------

def test_key_test_and_digits(jtw):
    for G in (0, 1, 2, 7, 256, 2**31 - 1, 2**31, 2**33):
        for key in (-2, -1, 0, 1, G - 1, G, G + 1, INT32_MAX, INT32_MIN):
            if INT32_MIN <= key <= INT32_MAX:
                assert bool(jtw.jrm_is_key(key, G)) == (0 <= key < G), (G, key)
    for G, digits in ((0, 0), (1, 0), (2, 1), (256, 1), (257, 2), (65536, 2), (65537, 3), (2**24, 3), (2**24 + 1, 4), (2**31, 4), (2**40, 4)):
        assert jtw.jrm_key_digits(G) == digits, G
        assert jtw.jrm_key_passes(G) == max(digits, 1), G
    for key in (0, 1, 0xFF, 0x100, 0x12345678, 0x7FFFFFFF):
        assert [jtw.jrm_digit(key, p) for p in range(4)] == [(key >> (8 * p)) & 0xFF for p in range(4)]


def test_pairs_per_row(jtw):
    for c in (0, 1, 2, 3000, 2**31 - 1):
        assert [jtw.jrm_pairs_of_row(k, c) for k in KINDS] == [c, max(c, 1), int(c > 0), int(c == 0)]


def test_pair_to_row(jtw):
    rng = random.Random(5)
    for _ in range(200):
        n = [rng.choice((0, 0, 0, 1, 2, 7)) for _ in range(rng.randrange(1, 40))]
        offsets = np.cumsum([0] + n).astype(np.uint64)
        for j in range(int(offsets[-1])):
            want = max(l for l in range(len(n)) if offsets[l] <= j)
            assert n[want] > 0
            assert jtw.jrm_row_of_pair(offsets.ctypes.data, 0, len(n), j) == want


# ---- the call -----------------------------------------------------------------------------------------------------------------

MIXED_L = [3, -1, 0, 3, 5, -2, 1, 1, 6, 0, 2, 9]
MIXED_R = [1, 3, -1, 3, 0, 7, 3, -2, 1, 5, 5]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("want_right,want_offsets,want_selects", [(True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, False, False)])
def test_kinds_and_optional_outputs(jtw, kind, want_right, want_offsets, want_selects):
    check(jtw, MIXED_L, MIXED_R, 7, kind, want_right=want_right, want_offsets=want_offsets, want_selects=want_selects)


@pytest.mark.parametrize("kind", KINDS)
def test_counts_of_zero_and_one(jtw, kind):
    for L in (0, 1):
        for R in (0, 1):
            for G in (0, 1):
                check(jtw, [0] * L, [0] * R, G, kind, where=(L, R, G))
                check(jtw, [0] * L, [0] * R, G, kind, left_room=L + 2, right_room=R + 3, keys_capacity=G + 5, where=(L, R, G, "rooms"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("G", [1, 2, 5, 256, 257, 70000])
def test_keys_at_the_edges(jtw, kind, G):
    edge = [-2, -1, 0, G - 1, G, INT32_MAX, INT32_MIN, G - 1, 0]
    check(jtw, edge + edge[::-1], edge[::2] + edge, G, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_shapes(jtw, kind):
    check(jtw, [-1] * 9, [0, 1, 2], 3, kind, where="left all null")
    check(jtw, [0, 1, 2], [-1, -2, 3, INT32_MIN], 3, kind, where="right all null")
    check(jtw, [-1] * 4, [5] * 3, 3, kind, where="both all null")
    check(jtw, [4] * 13, [4] * 17, 5, kind, where="every key equal: M = L * R")
    check(jtw, [2, 2, 0, 9, 7, 7, 3], list(range(10))[::-1], 10, kind, where="unique right keys")
    check(jtw, list(range(300, -1, -1)), list(range(299, -1, -1)) * 2, 300, kind, where="descending, two digits")
    check(jtw, list(range(300)), [k * 257 % 70001 for k in range(900)], 70001, kind, where="three digits")


@pytest.mark.parametrize("kind", KINDS)
def test_pairs_capacity(jtw, kind):
    M = py_join(MIXED_L, MIXED_R, len(MIXED_L), len(MIXED_R), 7, kind)[3][0]
    for room in (M - 1, M, M + 1, 0):
        got = check(jtw, MIXED_L, MIXED_R, 7, kind, pairs_capacity=room, where=room)
        assert got.res.n_pairs == M and got.res.code == (MSJ_CAPACITY if room < M else 0)


@pytest.mark.parametrize("kind", KINDS)
def test_counts_on_the_device_and_over_the_rooms(jtw, kind):
    lk, rk = keys_array(MIXED_L, 20), keys_array(MIXED_R, 16)
    check(jtw, MIXED_L, MIXED_R, 7, kind, left_room=20, right_room=16, G_dev=7, keys_capacity=9)
    got = check(jtw, MIXED_L, MIXED_R, 99, kind, G_dev=6, keys_capacity=6, definition=lambda a, b, L, R, G, k: py_join(a, b, L, R, 6, k))
    assert got.res.n_keys == 6
    for kw, counts in ((dict(L=21), (21, 16, 7)), (dict(R=17), (20, 17, 7)), (dict(G_dev=10, keys_capacity=9), (20, 16, 10)),
                       (dict(L=20, R=16, keys_capacity=6), (20, 16, 7))):
        got = twin_join(jtw, lk, rk, 7, kind, pairs_capacity=50, **kw)
        r = got.res
        assert got.rc == 0 and (r.code, r.flags, r.n_left, r.n_right, r.n_keys) == (MSJ_CAPACITY, kind) + counts, kw
        assert (r.n_pairs, r.n_left_matched, r.n_left_null, r.n_right_null) == (0, 0, 0, 0)
        assert (got.left == FILL32).all() and (got.right == FILL32).all() and (got.offsets == FILL64).all()
        assert (got.lsel.code, got.lsel.n_documents, got.rsel.code, got.rsel.n_found) == (MSJ_CAPACITY, 0, MSJ_CAPACITY, 0)


def test_rows_of_two_to_the_31(jtw):
    """L or R >= 2^31 on the device: MSJ_CAPACITY, though the room (never touched) would hold them"""
    lk = keys_array([0, 1])
    n = np.array([2**31], dtype=np.uint64)
    res = _lib.MsjJoinRowsResult()
    for side in (0, 1):
        rc = jtw.jrm_join_rows(1, _p(lk), 2**32, _p(n) if side == 0 else None, _p(lk), 2**32 if side else 2, _p(n) if side else None, 2, None, 2, 0,
                               None, None, 0, None, ctypes.addressof(res), None, None)
        assert (rc, res.code, res.n_pairs) == (0, MSJ_CAPACITY, 0)


def test_argument_checks_in_order(jtw):
    lk, rk = keys_array(MIXED_L), keys_array(MIXED_R)
    buf = np.zeros(64, dtype=np.uint64)
    res, sel = _lib.MsjJoinRowsResult(), tcm.select_result(0, 0)
    big = 1 << 40

    def call(ctx=1, left=_p(lk), left_rows=len(lk), n_left=None, right=_p(rk), right_rows=len(rk), flags=0, out_left=_p(buf), out_right=None,
             pairs_capacity=4, offsets=None, result=ctypes.addressof(res), lsel=None, keys_capacity=7):
        return jtw.jrm_join_rows(ctx, left, left_rows, n_left, right, right_rows, None, 7, None, keys_capacity, flags, out_left, out_right,
                                 pairs_capacity, offsets, result, lsel, None)

    assert call(pairs_capacity=100) == 0
    # 1 .. 5, each alone and each in front of the capacity check
    for extra in ({}, dict(keys_capacity=big)):
        assert call(ctx=0, **extra) == BAD_ARGUMENT
        assert call(result=None, **extra) == BAD_ARGUMENT
        assert call(left=None, **extra) == BAD_ARGUMENT
        assert call(right=None, **extra) == BAD_ARGUMENT
        assert call(out_left=None, **extra) == BAD_ARGUMENT
        assert call(flags=4, **extra) == BAD_ARGUMENT
        assert call(flags=1 << 31, **extra) == BAD_ARGUMENT
        assert call(offsets=_p(lk), **extra) == BAD_ARGUMENT                       # over the left keys
        assert call(offsets=_p(rk) - 8 * len(lk), **extra) == BAD_ARGUMENT          # its last word over the right keys
    assert call(left=None, left_rows=0, n_left=_p(buf), offsets=_p(buf)) == BAD_ARGUMENT  # over a count word
    assert call(left=None, left_rows=0, right=None, right_rows=0, out_left=None, pairs_capacity=0) == 0
    # 6: a room of 2^40 wins over what follows it
    for kw in (dict(left_rows=big), dict(right_rows=big), dict(keys_capacity=big), dict(pairs_capacity=big)):
        assert call(**kw) == MSJ_CAPACITY
        assert call(out_right=_p(buf) + 2, **kw) == MSJ_CAPACITY
        assert call(lsel=ctypes.addressof(res), **kw) == MSJ_CAPACITY
    # 7, 8
    assert call(left=_p(lk) + 2) == BAD_ARGUMENT
    assert call(out_left=_p(buf) + 2) == BAD_ARGUMENT
    assert call(out_right=_p(buf) + 1) == BAD_ARGUMENT
    assert call(offsets=_p(buf) + 4) == BAD_ARGUMENT
    assert call(n_left=_p(buf) + 4) == BAD_ARGUMENT
    assert call(result=ctypes.addressof(res) + 4) == BAD_ARGUMENT
    assert call(lsel=ctypes.addressof(sel) + 4) == BAD_ARGUMENT
    assert call(lsel=ctypes.addressof(res)) == BAD_ARGUMENT


@pytest.mark.parametrize("seed", range(6))
def test_random_rounds(jtw, seed):
    rng = random.Random(seed)
    for _ in range(60):
        G = rng.choice((1, 2, 3, 9, 256, 257, 1000, 65537))
        span = rng.choice((G, min(G, 4), G + 3))
        draw = lambda: rng.choice((-2, -1, INT32_MAX)) if rng.random() < 0.15 else rng.randrange(span)
        lkeys, rkeys = [draw() for _ in range(rng.randrange(0, 60))], [draw() for _ in range(rng.randrange(0, 60))]
        kind = rng.choice(KINDS)
        M = py_join(lkeys, rkeys, len(lkeys), len(rkeys), G, kind)[3][0]
        check(jtw, lkeys, rkeys, G, kind, left_room=len(lkeys) + rng.randrange(3), right_room=len(rkeys) + rng.randrange(3),
              keys_capacity=G + rng.randrange(3), pairs_capacity=rng.choice((M, M, M + 5, max(M - 1, 0))), where=(seed, G, kind))


@pytest.mark.parametrize("seed", range(3))
def test_numpy_definition_is_the_definition(seed):
    rng = random.Random(100 + seed)
    for _ in range(40):
        G = rng.choice((1, 3, 300))
        lkeys = [rng.randrange(-2, G + 2) for _ in range(rng.randrange(0, 50))]
        rkeys = [rng.randrange(-2, G + 2) for _ in range(rng.randrange(0, 50))]
        for kind in KINDS:
            a = py_join(lkeys, rkeys, len(lkeys), len(rkeys), G, kind)
            b = np_join(keys_array(lkeys), keys_array(rkeys), len(lkeys), len(rkeys), G, kind)
            assert (a[0], a[1], a[2], a[3]) == (b[0].tolist(), b[1].tolist(), b[2].tolist(), b[3])


@pytest.mark.parametrize("seed", range(3))
def test_identities(jtw, seed):
    rng = random.Random(200 + seed)
    G = rng.choice((4, 40, 400))
    lkeys = [rng.randrange(-1, G + 1) for _ in range(80)]
    rkeys = [rng.randrange(-1, G + 1) for _ in range(90)]
    out = {k: check(jtw, lkeys, rkeys, G, k) for k in KINDS}
    pairs = {k: list(zip(out[k].left[:out[k].res.n_pairs].tolist(), out[k].right[:out[k].res.n_pairs].tolist())) for k in KINDS}
    assert pairs[INNER] == [p for p in pairs[LEFT] if p[1] != NO_ROW]
    semi, anti = [p[0] for p in pairs[SEMI]], [p[0] for p in pairs[ANTI]]
    assert sorted(semi + anti) == list(range(len(lkeys))) and not set(semi) & set(anti)
    swapped = check(jtw, rkeys, lkeys, G, INNER)
    assert sorted((r, l) for l, r in zip(swapped.left[:swapped.res.n_pairs].tolist(), swapped.right[:swapped.res.n_pairs].tolist())) == sorted(pairs[INNER])
    match = py_match(lkeys, rkeys, len(lkeys), len(rkeys), G)
    for k in KINDS:
        n = np.diff(out[k].offsets[:len(lkeys) + 1].astype(np.int64)).tolist()
        c = [len(m) for m in match]
        assert n == [[x, max(x, 1), int(x > 0), int(x == 0)][k] for x in c]
