"""CPU check of msj_dictionary_device's arithmetic (mojo_simdjson_amd/csrc/dictionary_math.h).

The host twin (tests/dictionary_math_host.cpp: the header's row test, hash, byte compare and table walk, serially) runs over
hand-made columns, over the string-column twin's output and over the keys of the object-entries twin.  The yardstick is
Python and knows nothing of the header: ``dict.setdefault(value, len(d))`` over the rows' bytes in order.  Every case runs
with and without MSJ_DICTIONARY_WEAK_HASH, with the rows inserted ascending and descending (the device inserts in any
order), with room, with each capacity one short and layout-only, every array at its exact size with the fill and 64 canary
bytes behind each capacity.  The kernels that run the same header on the device are covered by tests/test_dictionary.py
(-m gpu); arrays from anywhere by tests/test_dictionary_sanitizers.py.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import helpers
from tests import test_number_math as tnm
from tests import test_object_entries_math as tom
from tests import test_select_math as tsm
from tests import test_string_column_math as tcm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
WEAK = 1            # MSJ_DICTIONARY_WEAK_HASH
FILL = 0x77
CANARY = 64         # bytes behind every array
MIN_SLOTS = 1024    # csrc/dictionary_math.h: kMinSlots

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/dictionary_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libdictionary_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "dictionary_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("dcm_dictionary", [vp, vp, u64, vp, vp, u64, vp, vp, vp, u64, vp, u64, u32, ctypes.c_int, vp], None),
                            ("dcm_hash", [ctypes.c_char_p, u64, u32, u64], u64),
                            ("dcm_table_slots", [u64], u64),
                            ("dcm_equal", [ctypes.c_char_p, ctypes.c_char_p, u64, u64], ctypes.c_int)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def dtwin():
    return load_twin()


# ---- the twin ---------------------------------------------------------------------------------------------------------------

class Column:
    """A byte column as the call reads it, every array at its exact size: offsets uint64[rows + 1], valid uint8[rows], data"""

    def __init__(self, offsets, valid, data):
        self.offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self.valid = np.ascontiguousarray(valid, dtype=np.uint8)
        self.data = np.frombuffer(bytes(data), dtype=np.uint8).copy()
        self.rows = int(self.valid.size)
        assert self.offsets.size == self.rows + 1

    def values(self, R=None):
        """The rows by the definition of the header file, in Python: bytes, or None for a null row"""
        off, n = self.offsets.tolist(), int(self.data.size)
        ok = lambda k: self.valid[k] != 0 and off[k] <= off[k + 1] <= n
        return [self.data[off[k]:off[k + 1]].tobytes() if ok(k) else None for k in range(self.rows if R is None else R)]


def column_of(values):
    """Python values (bytes, or None for a null row, whose offsets stand still) -> Column"""
    offsets, data = [0], bytearray()
    for v in values:
        data += v or b""
        offsets.append(len(data))
    return Column(offsets, [v is not None for v in values], data)


class Encoded:
    """What one call left: the result and the four arrays, each with its fill and 64 bytes of canary behind its capacity.
    The dictionary arrays are None in the layout-only form."""

    def __init__(self, res, codes, dict_offsets, dict_first, dict_bytes, rows, dict_capacity, dict_bytes_capacity):
        self.res, self.codes, self.dict_offsets, self.dict_first, self.dict_bytes = res, codes, dict_offsets, dict_first, dict_bytes
        self.rows, self.dict_capacity, self.dict_bytes_capacity = rows, dict_capacity, dict_bytes_capacity

    def summary(self):
        """(everything but max_probe, which depends on the order of insertion)"""
        r = self.res
        return (r.code, r.flags, r.n_rows, r.n_values, r.n_distinct, r.dict_bytes)

    def values(self):
        n = int(self.res.n_distinct)
        off = self.dict_offsets[:n + 1].tolist()
        return [self.dict_bytes[off[c]:off[c + 1]].tobytes() for c in range(n)]

    def untouched(self, R, n_entries, nbytes):
        """Codes at or past R (-1: nothing written at all), dictionary offsets past n_entries, first rows at or past it, bytes
        at or past nbytes, and the canaries, are as they were filled"""
        ok = bool((self.codes.view(np.uint8)[4 * max(R, 0):] == FILL).all())
        if self.dict_offsets is None:
            return ok
        ok = ok and bool((self.dict_offsets.view(np.uint8)[8 * (n_entries + 1 if R >= 0 else 0):] == FILL).all())
        ok = ok and bool((self.dict_first.view(np.uint8)[4 * n_entries:] == FILL).all())
        return ok and bool((self.dict_bytes[nbytes:] == FILL).all())


def filled(rows, dict_capacity, dict_bytes_capacity, layout_only=False):
    """-> (codes int32[rows + 16], dict_offsets uint64[cap + 1 + 8], dict_first uint32[cap + 16], dict_bytes uint8[bytes + 64])"""
    codes = np.full(4 * rows + CANARY, FILL, dtype=np.uint8).view(np.int32)
    if layout_only:
        return codes, None, None, None
    return (codes, np.full(8 * (dict_capacity + 1) + CANARY, FILL, dtype=np.uint8).view(np.uint64),
            np.full(4 * dict_capacity + CANARY, FILL, dtype=np.uint8).view(np.uint32), np.full(dict_bytes_capacity + CANARY, FILL, dtype=np.uint8))


def twin_dictionary(dtwin, col, rows=None, n_rows=None, flags=0, dict_capacity=None, dict_bytes_capacity=None, layout_only=False, order=0):
    """dcm_dictionary over the Column.  Capacities None: what a layout-only first call reports.  -> Encoded"""
    rows = col.rows if rows is None else rows
    if not layout_only and (dict_capacity is None or dict_bytes_capacity is None):
        first = twin_dictionary(dtwin, col, rows, n_rows, flags, layout_only=True, order=order).res
        dict_capacity = int(first.n_distinct) if dict_capacity is None else dict_capacity
        dict_bytes_capacity = int(first.dict_bytes) if dict_bytes_capacity is None else dict_bytes_capacity
    if layout_only:
        dict_capacity = dict_bytes_capacity = 0
    codes, d_off, d_first, d_bytes = filled(rows, dict_capacity, dict_bytes_capacity, layout_only)
    res = _lib.MsjDictionaryResult()
    word = ctypes.c_uint64(n_rows) if n_rows is not None else None
    ptr = lambda a: a.ctypes.data if a is not None else None
    dtwin.dcm_dictionary(col.offsets.ctypes.data, col.valid.ctypes.data, rows, ctypes.addressof(word) if word is not None else None,
                         col.data.ctypes.data, col.data.size, codes.ctypes.data, ptr(d_off), ptr(d_first), dict_capacity, ptr(d_bytes),
                         dict_bytes_capacity, flags, order, ctypes.byref(res))
    return Encoded(res, codes, d_off, d_first, d_bytes, rows, dict_capacity, dict_bytes_capacity)


# ---- the yardstick ----------------------------------------------------------------------------------------------------------

def definition(values):
    """values: bytes or None per row -> (codes, the distinct values in the order of first appearance, their first rows)"""
    seen, codes, first = {}, [], []
    for k, v in enumerate(values):
        if v is None:
            codes.append(-1)
            continue
        if v not in seen:
            first.append(k)
        codes.append(seen.setdefault(v, len(seen)))
    return codes, list(seen), first


def check(got, values, flags=0):
    """An Encoded with room for everything against the yardstick"""
    codes, distinct, first = definition(values)
    R, n, total = len(values), len(distinct), sum(len(v) for v in distinct)
    assert got.summary() == (0, flags, R, sum(v is not None for v in values), n, total), got.summary()
    assert got.codes[:R].tolist() == codes
    if got.dict_offsets is not None:
        assert got.values() == distinct and got.dict_first[:n].tolist() == first and got.dict_offsets[0] == 0
    assert got.untouched(R, n, total)
    longest = int(got.res.max_probe)
    assert (longest == 0) == (got.res.n_values == 0) and longest <= max(MIN_SLOTS, 4 * R)


def every_form(dtwin, col, R=None, **kw):
    """The column under both hashes and both orders of insertion: with room, with each capacity one short, layout-only"""
    values = col.values(R)
    codes, distinct, first = definition(values)
    n, total = len(distinct), sum(len(v) for v in distinct)
    for flags in (0, WEAK):
        for order in (0, 1):
            full = twin_dictionary(dtwin, col, flags=flags, order=order, **kw)
            check(full, values, flags)
            layout = twin_dictionary(dtwin, col, flags=flags, order=order, layout_only=True, **kw)
            check(layout, values, flags)
            roomy = twin_dictionary(dtwin, col, flags=flags, order=order, dict_capacity=n + 3, dict_bytes_capacity=total + 9, **kw)
            check(roomy, values, flags)
            if n:
                short = twin_dictionary(dtwin, col, flags=flags, order=order, dict_capacity=n - 1, dict_bytes_capacity=total, **kw)
                cut = sum(len(v) for v in distinct[:n - 1])
                assert short.summary() == (MSJ_CAPACITY,) + full.summary()[1:] and short.codes[:len(values)].tolist() == codes
                assert short.dict_first[:n - 1].tolist() == first[:n - 1] and short.dict_bytes[:cut].tobytes() == b"".join(distinct[:n - 1])
                assert np.array_equal(short.dict_offsets[:n], full.dict_offsets[:n]) and short.untouched(len(values), n - 1, cut)
            if total:
                short = twin_dictionary(dtwin, col, flags=flags, order=order, dict_capacity=n, dict_bytes_capacity=total - 1, **kw)
                assert short.summary() == (MSJ_CAPACITY,) + full.summary()[1:] and short.codes[:len(values)].tolist() == codes
                assert np.array_equal(short.dict_offsets[:n + 1], full.dict_offsets[:n + 1]) and short.dict_first[:n].tolist() == first
                assert short.dict_bytes[:total - 1].tobytes() == b"".join(distinct)[:total - 1] and short.untouched(len(values), n, total - 1)
    return full


def weak_values():
    """300 distinct values of lengths 0 .. 7, the lengths interleaved: under the weak hash four chains of about 75"""
    values = [b""] + [b"%0*d" % (n, j) if n > 1 else bytes([48 + j]) for j in range(43) for n in range(1, 8)]
    assert len(set(values[:300])) == 300 and {len(v) for v in values[:300]} == set(range(8))
    return values[:300]


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_small_columns(dtwin):
    """No row and one row; all null, all equal, all distinct; "" as a value next to null rows; values that are prefixes of
    each other; a value of zero bytes only, which the padded tail word cannot tell from a shorter one."""
    for values in ([], [b"a"], [None], [b""], [None] * 7, [b"same"] * 9, [b"v%d" % k for k in range(40)],
                   [b"", None, b"", None, b"x", b""], [b"abc", b"ab", b"a", b"", b"abcd", b"ab", b"abcdefgh", b"abcdefghi", b"abcdefgh"],
                   [b"\0", b"", b"\0\0", b"\0" * 8, b"\0" * 9, b"\0", None, b"\0" * 8]):
        every_form(dtwin, column_of(values))
    got = every_form(dtwin, column_of([b"", None, b"", None, b"x", b""]))
    assert got.codes[:6].tolist() == [0, -1, 0, -1, 1, 0] and got.values() == [b"", b"x"]


def test_one_byte_differences(dtwin):
    """Pairs of equal length 1 .. 33 that differ in exactly one byte at every position -- the tail word of the hash and of
    the compare -- with a copy of each original behind them: all distinct, every copy equal to its original."""
    values = []
    for n in range(1, 34):
        base = bytes((7 * n + j) & 0xFF for j in range(n))
        values.append(base)
        values += [base[:j] + bytes([base[j] ^ 0x40]) + base[j + 1:] for j in range(n)]
        values.append(base)
    got = every_form(dtwin, column_of(values))
    assert got.res.n_distinct == sum(n + 1 for n in range(1, 34)) and got.res.n_values == len(values)
    for n in (1, 7, 8, 9, 33):
        a = bytes(range(n))
        for j in range(n):
            b = a[:j] + bytes([a[j] ^ 1]) + a[j + 1:]
            assert not any(dtwin.dcm_equal(a, b, n, pieces) for pieces in (1, 2, 64)) and dtwin.dcm_equal(b, b, n, 3)


def test_hash_in_pieces(dtwin):
    """The hash is a function of the bytes and the length only and can be taken in pieces in any order; the weak hash is
    2^64 - 1 - (length mod 4)."""
    rng = np.random.default_rng(5)
    for n in (0, 1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 4097):
        v = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        whole = dtwin.dcm_hash(v, n, 0, 1)
        assert all(dtwin.dcm_hash(v, n, 0, pieces) == whole for pieces in (2, 3, 64, 256))
        assert dtwin.dcm_hash(v, n, WEAK, 64) == 0xFFFFFFFFFFFFFFFF - (n % 4)
        if n:
            assert dtwin.dcm_hash(v[:-1] + bytes([v[-1] ^ 1]), n, 0, 1) != whole and dtwin.dcm_hash(v + b"\0", n + 1, 0, 1) != whole
    assert [dtwin.dcm_table_slots(r) for r in (0, 1, 512, 513, 1024, 1025, (1 << 31) - 1)] == [1024, 1024, 1024, 2048, 2048, 4096, 1 << 32]


def test_hostile_offsets(dtwin):
    """Offsets that descend, lie past bytes_len or jump back: each such row is null, every other row keeps its value, and
    rows may share or overlap their bytes."""
    data = b"abcabcxyz"
    cases = [([9, 6, 3, 0], [1, 1, 1]), ([0, 3, 10, 6, 9], [1, 1, 1, 1]), ([0, 3, 2, 5, 1 << 40, 9], [1] * 5),
             ([0, 3, 0, 3, 6, 3, 6, 9], [1] * 7), ([3, 3, 3, 9, 9], [1, 1, 1, 1]), ([(1 << 64) - 1, 0, 3], [1, 1])]
    for offsets, valid in cases:
        col = Column(offsets, valid, data)
        every_form(dtwin, col)
    col = Column([0, 3, 0, 3, 6, 3, 6, 9], [1] * 7, data)
    assert col.values() == [b"abc", None, b"abc", b"abc", None, b"abc", b"xyz"]
    assert twin_dictionary(dtwin, col).codes[:7].tolist() == [0, -1, 0, 0, -1, 0, 1]


def test_valid_bytes_and_row_counts(dtwin):
    """A valid byte other than 0 and 1 is a value; the rows on the device equal to, below and above `rows`: below leaves
    the codes past R alone, above is MSJ_CAPACITY with nothing else written."""
    col = column_of([b"a", b"b", b"a", b"c", b"b"])
    col.valid[:] = [2, 0, 0x80, 0xFF, 1]
    assert col.values() == [b"a", None, b"a", b"c", b"b"]
    every_form(dtwin, col)
    for R in (5, 3, 0):
        every_form(dtwin, col, R=R, n_rows=R)
    for flags in (0, WEAK):
        over = twin_dictionary(dtwin, col, n_rows=6, flags=flags, dict_capacity=4, dict_bytes_capacity=4)
        assert over.summary() == (MSJ_CAPACITY, flags, 6, 0, 0, 0) and over.untouched(-1, 0, 0) and over.res.max_probe == 0
        empty = twin_dictionary(dtwin, col, n_rows=0, flags=flags, dict_capacity=2, dict_bytes_capacity=3)
        assert empty.summary() == (0, flags, 0, 0, 0, 0) and empty.dict_offsets[0] == 0 and empty.untouched(0, 0, 0)


def test_chains_that_wrap(dtwin):
    """300 values of lengths 0 .. 7 under the weak hash: four chains that start in the last four slots and wrap through
    slot 0, every slot decided by the byte compare; 300 rows of 3 values the same way."""
    values = weak_values()
    got = every_form(dtwin, column_of(values + values[::-3]))
    assert got.res.n_distinct == 300
    weak = twin_dictionary(dtwin, column_of(values), flags=WEAK)
    assert weak.res.max_probe >= 75
    every_form(dtwin, column_of([(b"red", b"green", b"blue")[k % 3] for k in range(300)]))


def test_escapes_through_the_string_column(dtwin):
    r"""Through the string-column twin: "\u0041" and "A", "a\/b" and "a/b" arrive unescaped, so one value written two ways
    has one code."""
    oracle, nm, stwin, ctwin = helpers.load_oracle(), tnm.load_twin(), tsm.load_twin(), tcm.load_twin()
    lines = [b'{"s":"\\u0041"}', b'{"s":"A"}', b'{"s":"\\u0041\\u0042"}', b'{"s":"AB"}', b'{"s":7}', b'{"s":"a\\/b"}', b'{"s":"a/b"}', b'{"t":1}',
             b'{"s":"\\u0041"}']
    data, w, records, _ = tcm.column_of(oracle, nm, stwin, lines)
    col = tcm.twin_column(ctwin, data, records, w.D)
    total = int(col.res.total_bytes)
    enc = every_form(dtwin, Column(col.offsets[:w.D + 1], col.valid[:w.D], col.data[:total].tobytes()))
    assert enc.codes[:w.D].tolist() == [0, 0, 1, 1, -1, 2, 2, -1, 0] and enc.values() == [b"A", b"AB", b"a/b"]
    want = [json.loads(x).get("s") for x in lines]
    assert definition([v.encode() if isinstance(v, str) else None for v in want])[0] == enc.codes[:w.D].tolist()


def test_keys_give_the_schema(dtwin):
    """The keys of the root objects, through the object-entries and string-column twins: the dictionary's values are the
    fields the documents have, in the order of first appearance, and with the value records' type byte the schema that
    json.loads gives."""
    oracle, nm, ctwin = helpers.load_oracle(), tnm.load_twin(), tcm.load_twin()
    twins = tom.tse.Twins()
    twins.l, twins.o = tom.tae.load_twin(), tom.load_twin()
    lines = [b'{"a":1,"b":2}', b'{"b":3,"c":4}', b'{"a":"x","c":[1],"d":null,"a":2.5}', b'[1]', b'{}']
    data = tdk.join(lines, b"\n")
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    rows, rows_select = tom.document_rows(twins, w, "")
    maps = tom.twin_maps(twins.o, w, rows, rows_select=rows_select)
    n = int(maps.res.n_entries)
    keys = tcm.twin_column(ctwin, data, maps.keys[:n], n)
    enc = every_form(dtwin, Column(keys.offsets[:n + 1], keys.valid[:n], keys.data[:int(keys.res.total_bytes)].tobytes()))
    pairs = [kv for text in lines if text.startswith(b"{") for kv in json.loads(text, object_pairs_hook=list)]
    assert n == len(pairs) == 8
    codes, distinct, _ = definition([k.encode() for k, _ in pairs])
    assert enc.codes[:n].tolist() == codes and enc.values() == distinct == [b"a", b"b", b"c", b"d"]
    tag = lambda v: "n" if v is None else "t" if v is True else "f" if v is False else "l" if isinstance(v, int) else \
        "d" if isinstance(v, float) else '"' if isinstance(v, str) else "[" if isinstance(v, list) else "{"
    want = {}
    for k, v in pairs:
        want.setdefault(k, [0, set()])
        want[k][0] += 1
        want[k][1].add(tag(v))
    got = {}
    for j in range(n):
        entry = got.setdefault(distinct[enc.codes[j]].decode(), [0, set()])
        entry[0] += 1
        entry[1].add(chr(int(maps.values[j]["type"])))
    assert got == want and want["a"] == [3, {"l", '"', "d"}] and list(got) == list(want)
