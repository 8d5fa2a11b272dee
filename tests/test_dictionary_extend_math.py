"""CPU check of msj_dictionary_extend_device's arithmetic (mojo_simdjson_amd/csrc/dictionary_extend_math.h over
dictionary_math.h).

The host twin of the whole call (tests/dictionary_extend_math_host.cpp) runs against the definition written in Python, which
knows nothing of the headers: a dict seeded with the prior entries in ascending code (the lowest code wins among equal
entries), then ``setdefault`` over the rows.  Twin and definition start from the SAME arrays -- the fill, 64 canary bytes
behind each capacity, the prior part in place -- and the whole of every array is compared, so a store into the prior part
or past a capacity shows.  Every form: with room, each capacity one short, no room, layout-only, frozen; both hashes, both
orders of insertion; damaged inputs.  Two identities carry the rest: with P = 0 the call is msj_dictionary_device
(tests/test_dictionary_math.py's twin), and a chain over windows equals that twin over the concatenated column.  The kernels
that run the same headers on the device are covered by tests/test_dictionary_extend.py (-m gpu); arrays from anywhere by
tests/test_dictionary_extend_sanitizers.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import helpers
from tests import test_dictionary_math as tdc
from tests import test_validate_math as tvm
from tests.test_dictionary_math import CANARY, FILL, MSJ_CAPACITY, WEAK, Column, column_of

FROZEN = 2          # MSJ_DICTIONARY_FROZEN
NO_ENTRY = -2       # the code of a row whose value a frozen dictionary does not hold
MAX_ITEMS = 1 << 31  # csrc/string_column_math.h: kMaxRows -- P + R stays below it

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/dictionary_extend_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libdictionary_extend_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "dictionary_extend_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    lib.dxm_dictionary_extend.argtypes = [vp, vp, u64, vp, vp, u64, u64, vp, vp, vp, vp, u64, vp, u64, u32, ctypes.c_int, vp]
    lib.dxm_dictionary_extend.restype = None
    lib.dxm_extend_slots.argtypes, lib.dxm_extend_slots.restype = [u64, u64, u32], u64
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def xtwin():
    return load_twin()


@pytest.fixture(scope="module")
def dtwin():
    return tdc.load_twin()


# ---- the arrays -------------------------------------------------------------------------------------------------------------

class Arrays:
    """The three dictionary arrays as a call finds them, each at its exact size + 64 canary bytes, everything the fill but
    the prior part: offsets[0 .. P] and the bytes below offsets[P].  offsets: the caller's (hostile ones for the damaged
    cases); data: the bytes they speak of."""

    def __init__(self, prior_offsets, data, dict_capacity, dict_bytes_capacity):
        self.dict_capacity, self.dict_bytes_capacity = dict_capacity, dict_bytes_capacity
        self.offsets = np.full(8 * (dict_capacity + 1) + CANARY, FILL, dtype=np.uint8).view(np.uint64)
        self.first = np.full(4 * dict_capacity + CANARY, FILL, dtype=np.uint8).view(np.uint32)
        self.bytes = np.full(dict_bytes_capacity + CANARY, FILL, dtype=np.uint8)
        fit = min(len(prior_offsets), dict_capacity + 1)
        self.offsets[:fit] = np.asarray(prior_offsets[:fit], dtype=np.uint64)
        fit = min(len(data), dict_bytes_capacity)
        self.bytes[:fit] = np.frombuffer(bytes(data[:fit]), dtype=np.uint8)

    def copy(self):
        other = Arrays.__new__(Arrays)
        other.dict_capacity, other.dict_bytes_capacity = self.dict_capacity, self.dict_bytes_capacity
        other.offsets, other.first, other.bytes = self.offsets.copy(), self.first.copy(), self.bytes.copy()
        return other

    def same(self, other):
        return (np.array_equal(self.offsets, other.offsets) and np.array_equal(self.first, other.first)
                and np.array_equal(self.bytes, other.bytes))

    def entries(self, P):
        """The prior entries by the header's entry test, in Python: bytes, or None for an entry without a value"""
        off, cap = self.offsets[:P + 1].tolist(), self.dict_bytes_capacity
        return [self.bytes[off[c]:off[c + 1]].tobytes() if off[c] <= off[c + 1] <= cap else None for c in range(P)]


def arrays_of(prior, dict_capacity=None, dict_bytes_capacity=None, spare=(0, 0)):
    """Prior values (bytes) back to back -> Arrays with room for them and `spare` (entries, bytes) more"""
    offsets, data = [0], bytearray()
    for v in prior:
        data += v
        offsets.append(len(data))
    cap = len(prior) + spare[0] if dict_capacity is None else dict_capacity
    room = len(data) + spare[1] if dict_bytes_capacity is None else dict_bytes_capacity
    return Arrays(offsets, data, cap, room)


def filled_codes(rows):
    return np.full(4 * rows + CANARY, FILL, dtype=np.uint8).view(np.int32)


def twin_extend(xtwin, col, arrays, P, flags=0, order=0, rows=None, n_rows=None, p_word=None):
    """dxm_dictionary_extend over the Column and the Arrays (None: the layout-only form), which it writes in place.
    p_word: P as the word on the device, in place of the argument.  -> (MsjDictionaryExtendResult, codes with canary)"""
    rows = col.rows if rows is None else rows
    codes = filled_codes(rows)
    res = _lib.MsjDictionaryExtendResult()
    word = ctypes.c_uint64(n_rows) if n_rows is not None else None
    pword = ctypes.c_uint64(p_word) if p_word is not None else None
    ref = lambda w: ctypes.addressof(w) if w is not None else None
    a = arrays
    xtwin.dxm_dictionary_extend(col.offsets.ctypes.data, col.valid.ctypes.data, rows, ref(word), col.data.ctypes.data, col.data.size, P, ref(pword),
                                codes.ctypes.data, a.offsets.ctypes.data if a else None, a.first.ctypes.data if a else None,
                                a.dict_capacity if a else 0, a.bytes.ctypes.data if a else None, a.dict_bytes_capacity if a else 0, flags, order,
                                ctypes.byref(res))
    return res, codes


def summary(res):
    """(everything but max_probe, which depends on the order of insertion)"""
    return (res.code, res.flags, res.n_rows, res.n_values, res.n_distinct, res.dict_bytes, res.n_prior, res.n_matched)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------

def definition(entries, values, frozen=False):
    """entries: bytes or None per prior entry; values: bytes or None per row -> (codes, the new values in code order, their
    first rows, the rows that matched a prior entry)"""
    P = len(entries)
    seen = {}
    for c, v in enumerate(entries):
        if v is not None:
            seen.setdefault(v, c)
    codes, new, first, matched = [], [], [], 0
    for k, v in enumerate(values):
        if v is None:
            codes.append(-1)
        elif v in seen:
            codes.append(seen[v])
            matched += seen[v] < P
        elif frozen:
            codes.append(NO_ENTRY)
        else:
            seen[v] = P + len(new)
            codes.append(seen[v])
            new.append(v), first.append(k)
    return codes, new, first, matched


def expected(arrays, P, values, flags=0):
    """What the definition leaves in a copy of the Arrays (None: layout-only) and in the result -> (Arrays, codes, summary)"""
    frozen = bool(flags & FROZEN)
    want = arrays.copy() if arrays is not None else None
    entries = arrays.entries(P) if arrays is not None else []
    base = int(arrays.offsets[P]) if P else 0
    codes, new, first, matched = definition(entries, values, frozen)
    n, total = P + len(new), base + sum(len(v) for v in new)
    clipped = False
    if want is not None and not frozen:
        if P == 0:
            want.offsets[0] = 0
        at = base
        for j, v in enumerate(new):
            c = P + j
            if c < want.dict_capacity:
                want.first[c], want.offsets[c + 1] = first[j], at + len(v)
                fit = max(0, min(len(v), want.dict_bytes_capacity - at))
                want.bytes[at:at + fit] = np.frombuffer(v[:fit], dtype=np.uint8)
            at += len(v)
        clipped = n > want.dict_capacity or total > want.dict_bytes_capacity
    return want, codes, (MSJ_CAPACITY if clipped else 0, flags, len(values), sum(v is not None for v in values), n, total, P, matched)


def check(xtwin, col, arrays, P, flags=0, order=0, R=None):
    """One call of the twin against the definition over the whole of every array -> (result, the Arrays as left)"""
    values = col.values(R)
    got = arrays.copy() if arrays is not None else None
    res, codes = twin_extend(xtwin, col, got, P, flags, order, n_rows=R)
    want, want_codes, want_summary = expected(arrays, P, values, flags)
    assert summary(res) == want_summary, (summary(res), want_summary)
    assert codes[:len(values)].tolist() == want_codes and bool((codes.view(np.uint8)[4 * len(values):] == FILL).all())
    if got is not None:
        assert got.same(want)
    slots = xtwin.dxm_extend_slots(P, len(values), flags)
    assert (res.max_probe == 0) == (res.n_values == 0 and not any(e is not None for e in (arrays.entries(P) if arrays else [])))
    assert res.max_probe <= slots
    return res, got


def every_form(xtwin, prior, values):
    """Prior values and a column under both hashes and both orders: with room, each capacity one short, no room at all,
    frozen, and with P = 0 layout-only"""
    col = column_of(values)
    P, base = len(prior), sum(len(v) for v in prior)
    _, new, _, _ = definition(list(prior), values)
    n_new, new_bytes = len(new), sum(len(v) for v in new)
    for flags in (0, WEAK):
        for order in (0, 1):
            check(xtwin, col, arrays_of(prior, spare=(n_new, new_bytes)), P, flags, order)
            check(xtwin, col, arrays_of(prior, spare=(n_new + 3, new_bytes + 9)), P, flags, order)
            if n_new:
                res, _ = check(xtwin, col, arrays_of(prior, spare=(n_new - 1, new_bytes)), P, flags, order)
                assert res.code == MSJ_CAPACITY
            if new_bytes:
                res, _ = check(xtwin, col, arrays_of(prior, spare=(n_new, new_bytes - 1)), P, flags, order)
                assert res.code == MSJ_CAPACITY
            res, _ = check(xtwin, col, arrays_of(prior), P, flags, order)  # dict_capacity == P, dict_bytes_capacity == base
            assert res.code == (MSJ_CAPACITY if n_new else 0)
            res, _ = check(xtwin, col, arrays_of(prior, spare=(2, 5)), P, flags | FROZEN, order)
            assert res.code == 0 and res.n_distinct == P and res.dict_bytes == base
            if P == 0:
                check(xtwin, col, None, 0, flags, order)


def generated(seed, rows, vocabulary=40):
    """A column of `rows` values drawn from a vocabulary of mixed lengths ("" and a value past 512 bytes among them) with
    null rows between"""
    rng = np.random.default_rng(seed)
    words = [b"", b"a", b"ab", b"abc" * 200] + [bytes(rng.integers(97, 123, int(rng.integers(1, 24)), dtype=np.uint8)) for _ in range(vocabulary)]
    picks = rng.integers(0, len(words) + 3, rows)
    return [words[p] if p < len(words) else None for p in picks]


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_every_form_small(xtwin):
    """No prior and no row up to both; "" and null rows on both sides; prefixes; values that are all prior, all new, mixed."""
    cases = [([], []), ([], [b"a"]), ([b"a"], []), ([b"a"], [b"a"]), ([b"a"], [b"b"]), ([b""], [None, b"", b"x", None, b""]),
             ([b"x", b"y"], [b"", b"y", None, b"", b"z", b"x", b"z"]), ([b"abc", b"ab", b"abcdefgh"], [b"a", b"ab", b"abcdefghi", b"abcdefgh", b"a"]),
             ([b"\0", b"\0\0"], [b"", b"\0" * 8, b"\0", b"\0" * 9, b"\0\0", b"\0" * 8]),
             ([b"red", b"green", b"blue"], [(b"red", b"green", b"blue", b"grey")[k % 4] for k in range(30)]),
             ([b"v%d" % k for k in range(40)], [b"v%d" % (k * 7 % 60) for k in range(90)])]
    for prior, values in cases:
        every_form(xtwin, prior, values)
    col = column_of([b"", b"y", None, b"", b"z", b"x", b"z"])
    res, codes = twin_extend(xtwin, col, arrays_of([b"x", b"y"], spare=(4, 9)), 2)
    assert codes[:7].tolist() == [2, 1, -1, 2, 3, 0, 3] and (res.n_distinct, res.n_matched) == (4, 2)
    res, codes = twin_extend(xtwin, col, arrays_of([b"x", b"y"], spare=(4, 9)), 2, flags=FROZEN)
    assert codes[:7].tolist() == [-2, 1, -1, -2, -2, 0, -2] and (res.n_distinct, res.n_matched, res.n_values) == (2, 2, 6)


def test_chains_that_wrap(xtwin):
    """Under the weak hash prior entries and rows stand in the same four chains that wrap through slot 0."""
    values = tdc.weak_values()
    every_form(xtwin, values[:150:2], values[::-1] + values[::3])
    every_form(xtwin, [b"red", b"blue"], [(b"red", b"green", b"blue")[k % 3] for k in range(300)])
    res, _ = twin_extend(xtwin, column_of(values[150:]), arrays_of(values[:150], spare=(150, 2000)), 150, flags=WEAK)
    assert res.max_probe >= 37 and res.n_distinct == 300


def test_one_byte_differences(xtwin):
    """Prior entries of length 1 .. 33 and rows that differ from them in exactly one byte at every position, then a copy of
    each: the copies match, nothing else does."""
    prior, values = [], []
    for n in range(1, 34):
        base = bytes((7 * n + j) & 0xFF for j in range(n))
        prior.append(base)
        values += [base[:j] + bytes([base[j] ^ 0x40]) + base[j + 1:] for j in range(n)] + [base]
    every_form(xtwin, prior, values)
    res, _ = twin_extend(xtwin, column_of(values), arrays_of(prior, spare=(600, 20000)), 33)
    assert res.n_matched == 33 and res.n_distinct == 33 + sum(range(1, 34))


def test_hostile_rows(xtwin):
    """Row offsets that descend, lie past bytes_len or jump back, valid bytes other than 0 and 1, a row count on the device
    below `rows`: tests/test_dictionary_math.py's cases against prior entries."""
    data = b"abcabcxyz"
    prior = [b"xyz", b"abc", b"q"]
    for offsets, valid in [([9, 6, 3, 0], [1, 1, 1]), ([0, 3, 10, 6, 9], [1, 1, 1, 1]), ([0, 3, 2, 5, 1 << 40, 9], [1] * 5),
                           ([0, 3, 0, 3, 6, 3, 6, 9], [1] * 7), ([3, 3, 3, 9, 9], [2, 0x80, 0, 0xFF]), ([(1 << 64) - 1, 0, 3], [1, 1])]:
        col = Column(offsets, valid, data)
        for flags in (0, WEAK, FROZEN, FROZEN | WEAK):
            for order in (0, 1):
                check(xtwin, col, arrays_of(prior, spare=(4, 12)), 3, flags, order)
                check(xtwin, col, arrays_of(prior), 3, flags, order)
                for R in range(col.rows):
                    check(xtwin, col, arrays_of(prior, spare=(4, 12)), 3, flags, order, R=R)
    col = Column([0, 3, 0, 3, 6, 3, 6, 9], [1] * 7, data)
    _, codes = twin_extend(xtwin, col, arrays_of(prior, spare=(4, 12)), 3)
    assert codes[:7].tolist() == [1, -1, 1, 1, -1, 1, 0]


def test_damaged_prior(xtwin):
    """Prior offsets that descend or exceed dict_bytes_capacity: those entries match nothing and stay where they are, the
    others match.  Duplicate prior entries: the lowest code wins.  Entries that overlap are values like any other."""
    data = b"redgreenblue!"
    rows = [b"red", b"green", b"blue", b"", b"!", b"greenblue", b"dgr", b"red"]
    cases = [[0, 3, 8, 12],                # in order
             [0, 3, 2, 12],                # entry 1 descends (no value), entry 2 = data[2:12]
             [0, 3, 1 << 40, 12],          # entry 1 ends, entry 2 starts out of range
             [3, 0, 3, 8, 8, 12],          # entry 0 descends; "red" at 1, "" at 3
             [0, 3, 0, 3, 0, 3],           # "red" at 0 and 4, the odd ones descend
             [0, 3, 3, 3, 8, 3, 8],        # "" twice (1, 2), "green" twice (3, 5), one that descends
             [2, 5, 3, 12, 12],            # overlapping: "dgr", none, data[3:12], ""
             [(1 << 64) - 1, 0, 12]]       # huge, then the whole
    for offsets in cases:
        P = len(offsets) - 1
        for spare in ((8, 40), (0, 0), (1, 40), (8, 1)):
            a = Arrays(offsets, data, P + spare[0], len(data) + spare[1])
            for flags in (0, WEAK, FROZEN):
                for order in (0, 1):
                    check(xtwin, column_of(rows), a, P, flags, order)
    a = Arrays([0, 3, 3, 3, 8, 3, 8], data, 14, 60)
    assert a.entries(6) == [b"red", b"", b"", b"green", None, b"green"]
    _, codes = twin_extend(xtwin, column_of(rows), a, 6)
    assert codes[:8].tolist() == [0, 3, 6, 1, 7, 8, 9, 0]


def test_nothing_written(xtwin):
    """R > rows, P > dict_capacity, base > dict_bytes_capacity, P + R >= 2^31: MSJ_CAPACITY, and nothing but code, flags,
    n_rows and n_prior is written -- whether P comes as the argument or as the word on the device.  P + R >= 2^31 runs with
    counts alone: no array is read before the counts pass."""
    col = column_of([b"a", b"b", b"a"])
    prior = [b"b", b"c"]
    for flags in (0, WEAK, FROZEN):
        for word in (False, True):
            p_of = lambda P: dict(P=0 if word else P, p_word=P if word else None)
            start = arrays_of(prior, spare=(3, 3))
            for kw, R, P in ((dict(n_rows=4, **p_of(2)), 4, 2), (dict(**p_of(6)), 3, 6), (dict(**p_of(1 << 40)), 3, 1 << 40)):
                got = start.copy()
                res, codes = twin_extend(xtwin, col, got, flags=flags, **kw)
                assert summary(res) == (MSJ_CAPACITY, flags, R, 0, 0, 0, P, 0) and res.max_probe == 0
                assert got.same(start) and bool((codes.view(np.uint8) == FILL).all())
            equal = Arrays([0, 1, 2, 2, 2, 2], b"bc", 5, 5)  # P == dict_capacity exactly is legal
            res, _ = twin_extend(xtwin, col, equal, flags=flags, **p_of(5))
            assert res.n_prior == 5 and res.code == (0 if flags & FROZEN else MSJ_CAPACITY) and res.n_values == 3 and res.n_matched == 1
            short = Arrays([0, 1, 2], b"bc", 5, 1)  # base = 2 above dict_bytes_capacity = 1
            got = short.copy()
            res, codes = twin_extend(xtwin, col, got, flags=flags, **p_of(2))
            assert summary(res) == (MSJ_CAPACITY, flags, 3, 0, 0, 0, 2, 0) and got.same(short) and bool((codes.view(np.uint8) == FILL).all())
            far = Arrays([0, 1, 1 << 50], b"bc", 5, 8)
            got = far.copy()
            res, _ = twin_extend(xtwin, col, got, flags=flags, **p_of(2))
            assert summary(res) == (MSJ_CAPACITY, flags, 3, 0, 0, 0, 2, 0) and got.same(far)
    # counts alone: no array of that size exists
    res = _lib.MsjDictionaryExtendResult()
    for rows, P, cap in ((MAX_ITEMS - 1, 1, 1), (1 << 30, 1 << 30, 1 << 30), (5, MAX_ITEMS - 5, MAX_ITEMS), (0, MAX_ITEMS, MAX_ITEMS),
                         (MAX_ITEMS, 0, 0), ((1 << 64) - 1, 2, 2)):
        stub = np.zeros(4, dtype=np.uint64)
        xtwin.dxm_dictionary_extend(None, None, rows, None, None, 0, P, None, None, stub.ctypes.data, stub.ctypes.data, cap, stub.ctypes.data, 0, 0, 0,
                                    ctypes.byref(res))
        assert summary(res) == (MSJ_CAPACITY, 0, rows, 0, 0, 0, P, 0) and not stub.any()


def test_clipped_then_repeated(xtwin):
    """After a clipped call, the prior part copied into larger arrays and the call repeated with the SAME P gives the
    unclipped answer; repeating a call over its own output with the same P changes no byte."""
    prior = [b"alpha", b"beta"]
    values = generated(3, 200)
    col = column_of(values)
    _, new, _, _ = definition(prior, values)
    full = arrays_of(prior, spare=(len(new), sum(map(len, new))))
    res_full, want = check(xtwin, col, full, 2)
    for spare in ((1, 4), (0, 0), (len(new) - 1, sum(map(len, new))), (len(new), sum(map(len, new)) - 1)):
        small = arrays_of(prior, spare=spare)
        res, left = check(xtwin, col, small, 2)
        assert res.code == MSJ_CAPACITY and (res.n_distinct, res.dict_bytes) == (res_full.n_distinct, res_full.dict_bytes)
        grown = Arrays(left.offsets[:3].tolist(), left.bytes[:9].tobytes(), int(res.n_distinct), int(res.dict_bytes))
        res2, codes2 = twin_extend(xtwin, col, grown, 2)
        assert summary(res2) == summary(res_full) and grown.same(want)
    again = want.copy()
    res3, _ = twin_extend(xtwin, col, again, 2)
    assert summary(res3) == summary(res_full) and again.same(want)


def test_without_prior_it_is_the_dictionary_call(xtwin, dtwin):
    """Identity 1: with P = 0 every output equals msj_dictionary_device's twin, and the extra members are 0."""
    for seed, rows in ((1, 0), (2, 1), (3, 257), (4, 1500)):
        col = column_of(generated(seed, rows))
        for flags in (0, WEAK):
            for layout_only in (False, True):
                for short in (0, 1):
                    base = tdc.twin_dictionary(dtwin, col, flags=flags, layout_only=layout_only)
                    cap, room = (0, 0) if layout_only else (max(int(base.res.n_distinct) - short, 0), max(int(base.res.dict_bytes) - short, 0))
                    base = tdc.twin_dictionary(dtwin, col, flags=flags, layout_only=layout_only, dict_capacity=cap, dict_bytes_capacity=room)
                    a = None if layout_only else Arrays([], b"", cap, room)
                    res, codes = twin_extend(xtwin, col, a, 0, flags=flags)
                    assert summary(res) == base.summary() + (0, 0)
                    assert np.array_equal(codes, base.codes)
                    if a is not None:
                        assert np.array_equal(a.offsets, base.dict_offsets) and np.array_equal(a.first, base.dict_first)
                        assert np.array_equal(a.bytes, base.dict_bytes)


def test_a_chain_is_the_whole_column(xtwin, dtwin):
    """Identity 2: a chain over windows, each call's P the previous n_distinct, equals msj_dictionary_device's twin over the
    concatenated column: the codes concatenated, dict_offsets and dict_bytes, and dict_first[c] less the row base of the
    window that introduced c.  Windows of 0 and 1 rows among them."""
    for seed, sizes in ((5, (300, 1, 0, 513)), (6, (0, 0, 7)), (7, (1, 1, 1, 1, 256, 0, 255)), (8, (64,))):
        values = generated(seed, sum(sizes), vocabulary=90)
        whole = tdc.twin_dictionary(dtwin, column_of(values))
        n, total = int(whole.res.n_distinct), int(whole.res.dict_bytes)
        for flags in (0, WEAK):
            a = Arrays([], b"", n, total)
            P, at, codes, first_base = 0, 0, [], np.zeros(n, dtype=np.int64)
            for size in sizes:
                res, c = twin_extend(xtwin, column_of(values[at:at + size]), a, 0, flags=flags, p_word=P)
                assert res.code == 0 and res.n_prior == P and res.n_rows == size
                codes += c[:size].tolist()
                first_base[P:int(res.n_distinct)] = at
                P, at = int(res.n_distinct), at + size
            assert P == n and codes == whole.codes[:len(values)].tolist()
            assert np.array_equal(a.offsets, whole.dict_offsets) and np.array_equal(a.bytes, whole.dict_bytes)
            assert np.array_equal(a.first[:n].astype(np.int64) + first_base, whole.dict_first[:n].astype(np.int64))
            assert bool((a.first.view(np.uint8)[4 * n:] == FILL).all())
