"""CPU check of the arithmetic of msj_dictionary_order_device and msj_rank_rows_device
(mojo_simdjson_amd/csrc/dictionary_order_math.h).

The host twin (tests/dictionary_order_math_host.cpp: the header's entry test, word fetch, key, digits and tied test, the
call built serially from them in the kernels' steps, both paths' sorts) runs over hand-made dictionaries.  The yardstick is
the definition of include/msj_stage1.h written in Python and knows nothing of the header: ``sorted`` over ``(v[:B], entry)``
and ``bisect`` for the ranks.  Every output is compared over its WHOLE array, each at its exact size and pre-filled, so a
write at or past V shows.  ``Dict`` and ``py_order`` are also what the GPU tests use (tests/test_dictionary_order.py, -m gpu);
arrays from anywhere are tests/test_dictionary_order_sanitizers.py's.
"""
import bisect
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import test_validate_math as tvm

MSJ_CAPACITY, BAD_ARGUMENT = 1, -1
CONTINUE = 1
NO_RANK = 0xFFFFFFFF
FILL32 = 0xA5A5A5A5
AUTO, GRID, GROUP = 0, 1, 2
GROUP_ENTRIES = 1024
ALPHABET = (0x00, ord("a"), ord("b"), 0x7F, 0x80, 0xFF)
PREFIXES = (0, 7, 8, 9, 15, 16, 17, 63, 64, 65)
LENGTHS = tuple(range(18)) + tuple(range(62, 67))
RADIX_SIZES = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2 * 1024 + 1)  # a wave, a round of 256, a tile of 1 024


class OrderResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_entries", ctypes.c_uint64), ("n_values", ctypes.c_uint64),
                ("n_tied", ctypes.c_uint64), ("depth", ctypes.c_uint64), ("n_equal", ctypes.c_uint64)]


class RankRowsResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_rows", ctypes.c_uint64), ("n_ranked", ctypes.c_uint64),
                ("n_null", ctypes.c_uint64), ("n_unknown", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


class SelectResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("n_documents", ctypes.c_uint64), ("n_paths", ctypes.c_uint64),
                ("n_found", ctypes.c_uint64), ("n_no_bits", ctypes.c_uint64), ("reserved", ctypes.c_uint64)]


FIELD = np.dtype([("bits", "<u8"), ("token", "<u4"), ("type", "u1"), ("flags", "u1"), ("code", "<u2")])

_twin = None


def load_twin():
    """The host twin of the two calls (g++ build of tests/dictionary_order_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libdictionary_order_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "dictionary_order_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int32
    for name, args, res in (("dom_fetch_word", [vp, u64, u64, u64, u64, vp, vp], None),
                            ("dom_key_digits", [u64], u32),
                            ("dom_digit", [u64, u32, u32, u32], u32),
                            ("dom_use_group_path", [u64, u32], i32),
                            ("dom_rounds_of", [u32, i32], u32),
                            ("dom_dictionary_order", [i32, vp, vp, u64, u64, vp, u64, u64, u32, u32, u32, vp, vp, vp, vp], i32),
                            ("dom_rank_rows", [i32, vp, u64, vp, vp, u64, vp, vp, u64, vp, vp], i32)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def tw():
    return load_twin()


def ptr(a):
    return None if a is None else a.ctypes.data


# ---- a dictionary from a list of values ---------------------------------------------------------------------------------------

class Dict:
    """(offsets, bytes) of ``values``; None is an entry without a value.  Runs of values stand at descending places of the
    byte array, a byte apart, so that the offsets around an entry without a value fail the entry test: offsets[c] >
    offsets[c + 1], or offsets[c + 1] past the capacity.  ``extra``: live-looking offsets behind V."""

    def __init__(self, values, extra=0):
        self.values = list(values)
        V = len(self.values)
        runs, run = [], []
        for c, v in enumerate(self.values):
            if v is None:
                if run:
                    runs.append(run)
                run = []
            else:
                run.append(c)
        if run:
            runs.append(run)
        total = sum(len(v) for v in self.values if v is not None) + len(runs)
        self.cap = total
        data = bytearray(b"\xEE" * total)
        start = {}
        at = total
        for run in runs:
            at -= sum(len(self.values[c]) for c in run) + 1
            q = at
            for c in run:
                start[c] = q
                data[q:q + len(self.values[c])] = self.values[c]
                q += len(self.values[c])
        offsets = [0] * (V + 1 + extra)
        for c in range(V + 1):
            if c < V and self.values[c] is not None:
                offsets[c] = start[c]
            elif c > 0 and self.values[c - 1] is not None:
                offsets[c] = start[c - 1] + len(self.values[c - 1])
            else:
                offsets[c] = self.cap + 7 + c
        for c in range(V + 1, V + 1 + extra):
            offsets[c] = min(offsets[V], self.cap)  # (entry V and on would pass the entry test: empty values)
        self.offsets = np.array(offsets, dtype=np.uint64)
        self.bytes = np.frombuffer(bytes(data), dtype=np.uint8).copy() if total else np.zeros(0, dtype=np.uint8)
        self.V = V
        for c, v in enumerate(self.values):  # the layout says what was meant
            a, b = int(self.offsets[c]), int(self.offsets[c + 1])
            has = a <= b <= self.cap
            assert has == (v is not None) and (not has or bytes(data[a:b]) == v), (c, v, a, b)


# ---- the yardstick: the definition --------------------------------------------------------------------------------------------

def py_order(values, B=None):
    """-> (sorted, rank, n_values, n_tied, n_equal) of the order by depth B (None: the whole values)"""
    V = len(values)
    have = [e for e in range(V) if values[e] is not None]
    v = {e: (values[e] if B is None else values[e][:B]) for e in have}
    order = sorted(have, key=lambda e: (v[e], e)) + [e for e in range(V) if values[e] is None]
    keys = sorted(v[e] for e in have)
    rank = [NO_RANK] * V
    n_tied = n_equal = 0
    first = {}
    for e in have:
        lo = bisect.bisect_left(keys, v[e])
        rank[e] = lo
        shared = bisect.bisect_right(keys, v[e]) - lo > 1
        tied = shared and B is not None and len(values[e]) >= B
        n_tied += tied
        if not tied and lo in first:
            n_equal += 1
        first.setdefault(lo, e)
    return order, rank, len(have), n_tied, n_equal


def run_twin(tw, d, capacity=None, depth=0, max_rounds=0, flags=0, mode=AUTO, state=None, on_device=False, ctx_ok=1):
    """One call of the twin over exact-size pre-filled arrays -> (rc, result, sorted, rank, passes)"""
    capacity = d.V if capacity is None else capacity
    if state is None:
        srt, rnk = np.full(capacity, FILL32, dtype=np.uint32), np.full(capacity, FILL32, dtype=np.uint32)
    else:
        srt, rnk = state[0].copy(), state[1].copy()
    res = OrderResult()
    ctypes.memset(ctypes.byref(res), 0xA5, ctypes.sizeof(res))
    passes = ctypes.c_uint64(0)
    n = np.array([d.V], dtype=np.uint64)
    rc = tw.dom_dictionary_order(ctx_ok, ptr(d.offsets), ptr(d.bytes) if d.cap else None, d.cap, 0 if on_device else d.V,
                                 ptr(n) if on_device else None, capacity, depth, max_rounds, flags, mode, ptr(srt), ptr(rnk),
                                 ctypes.addressof(res), ctypes.addressof(passes))
    return rc, res, srt, rnk, passes.value


def check_against(values, res, srt, rnk, B, capacity):
    order, rank, n_values, n_tied, n_equal = py_order(values, B)
    V = len(values)
    assert list(srt[:V]) == order, (B, list(srt[:V]), order)
    assert list(rnk[:V]) == rank, (B, list(rnk[:V]), rank)
    assert (srt[V:] == FILL32).all() and (rnk[V:] == FILL32).all()
    assert (res.n_entries, res.n_values, res.n_tied, res.n_equal) == (V, n_values, n_tied, n_equal)
    assert res.code == (MSJ_CAPACITY if n_tied else 0)


# ---- the corpus -------------------------------------------------------------------------------------------------------------

def word(rng, n):
    return bytes(rng.choice(ALPHABET) for _ in range(n))


def corpus():
    """Named lists of values: the alphabet orders NUL against the padding and 0x80 / 0xff against signed compares"""
    rng = random.Random(20261021)
    out = {"empty": [], "one": [b"a"], "one-none": [None], "two": [b"b", b"a"], "two-equal": [b"a", b"a"],
           "nul-against-padding": [b"a\x00", b"a", b"a\x00\x00", b"", b"\x00", b"a" * 8 + b"\x00", b"a" * 8, b"a" * 7, b"a" * 7 + b"\x00"],
           "signed": [b"\x80", b"\x7f", b"\xff", b"\x00", b"a", b"\xff\x00", b"\x7f\xff", b"\x80\x00"],
           "equal-multiples-of-8": [b"b" * 16, b"a" * 8, b"b" * 16, b"a" * 8, b"a" * 16, b"b" * 8, b"a" * 8, b"", b""],
           "lengths": [word(rng, n) for n in LENGTHS]}
    for shared in PREFIXES:
        prefix = word(rng, shared)
        vals = [prefix + word(rng, rng.choice((0, 1, 2, 7, 8, 9))) for _ in range(24)] + [prefix, prefix + b"\x00", prefix + b"\xff"]
        vals += [vals[3], vals[5], prefix]  # duplicates
        rng.shuffle(vals)
        out[f"prefix-{shared}"] = vals
        holes = list(vals)
        for c in (0, 1, len(holes) // 2, len(holes) - 1):
            holes[c] = None
        out[f"prefix-{shared}-holes"] = holes
    for V in (GROUP_ENTRIES - 1, GROUP_ENTRIES, GROUP_ENTRIES + 1):
        pre = word(rng, 9)
        out[f"border-{V}"] = [None if rng.random() < 0.02 else (pre if rng.random() < 0.7 else b"") + word(rng, rng.choice((0, 1, 3, 8, 11))) for _ in range(V)]
    # The grid path's radix pass (radix_block.h) at its borders: N entries, every one with a value, so that round 0 sorts a tied
    # set of exactly N.  Byte 0 takes every bucket inside a tile; byte 2 is the same over 64 neighbours (a wave adds to the
    # histogram once); byte 1 between them is constant: its pass is skipped, and the pass behind it reads the buffer that the
    # NUMBER of passes in front says.  Equal values on both sides of a wave, a round and a tile border; entries 768 apart tie
    # again in round 1
    for N in RADIX_SIZES:
        vals = [bytes([i % 256, 0x40, 1 + (i // 64) % 3]) + b"-----%04d" % (N - i) for i in range(N)]
        for a in (63, 255, 1023):
            if a + 1 < N:
                vals[a + 1] = vals[a]
        out[f"radix-{N}"] = vals
    return out


CORPUS = corpus()


@pytest.mark.parametrize("name", sorted(CORPUS))
@pytest.mark.parametrize("mode", (GRID, GROUP))
def test_one_call_is_the_definition(tw, name, mode):
    values = CORPUS[name]
    d = Dict(values)
    rc, res, srt, rnk, _ = run_twin(tw, d, max_rounds=64, mode=mode, on_device=True)
    assert rc == 0
    check_against(values, res, srt, rnk, None, d.V)
    assert res.n_tied == 0 and res.depth % 8 == 0
    if all(v is not None for v in values) and len(set(values)) == len(values):
        assert all(srt[rnk[c]] == c for c in range(d.V))


@pytest.mark.parametrize("name", sorted(n for n in CORPUS if not n.startswith("border") or n == "border-1025"))
@pytest.mark.parametrize("budget", (1, 2, 3))
def test_continued_chains(tw, name, budget):
    """After every call the arrays are the order by the call's depth; the chain ends in one unbounded call's bytes; the two
    paths take turns along the chain"""
    values = CORPUS[name]
    d = Dict(values)
    _, want, want_s, want_r, _ = run_twin(tw, d, max_rounds=64, mode=GRID)
    state, depth, calls = None, 0, 0
    while True:
        mode = (GRID, GROUP)[calls & 1]
        rc, res, srt, rnk, _ = run_twin(tw, d, depth=depth, max_rounds=budget, flags=CONTINUE if calls else 0, mode=mode, state=state)
        assert rc == 0
        check_against(values, res, srt, rnk, res.depth, d.V)
        calls += 1
        if res.code == 0:
            break
        assert res.depth == depth + 8 * budget and res.n_tied > 0
        state, depth = (srt, rnk), res.depth
        assert calls < 40
    assert (srt == want_s).all() and (rnk == want_r).all()
    assert (res.n_values, res.n_equal, res.depth) == (want.n_values, want.n_equal, want.depth)


def test_random_dictionaries(tw):
    rng = random.Random(7)
    for _ in range(300):
        shared = word(rng, rng.choice((0, 0, 3, 8, 12, 24)))
        vals = [None if rng.random() < 0.05 else (shared if rng.random() < 0.8 else b"") + word(rng, rng.randrange(0, 12)) for _ in range(rng.randrange(0, 40))]
        d = Dict(vals)
        for mode in (GRID, GROUP):
            rc, res, srt, rnk, _ = run_twin(tw, d, capacity=d.V + rng.randrange(3), max_rounds=64, mode=mode)
            assert rc == 0
            check_against(vals, res, srt, rnk, None, d.V)


def test_constant_digits_cost_no_pass(tw):
    """id%07d below 100 000: two rounds.  Round 0's word is 'id00' and four decimal digits: four passes, the rank 0
    everywhere; round 1's is the last decimal digit, nvalid 1 everywhere: one pass and the two digits of a rank below 3 000"""
    vals = [b"id%07d" % i for i in random.Random(3).sample(range(100000), 3000)]
    d = Dict(vals)
    rc, res, srt, rnk, passes = run_twin(tw, d, max_rounds=64, mode=GRID)
    check_against(vals, res, srt, rnk, None, d.V)
    assert res.depth == 16 and passes == 4 + 1 + 2


def test_a_constant_digit_between_two_that_differ(tw):
    """radix-257, round 0: bytes 0 and 2 of the word differ (digits 8 and 6), byte 1 between them does not: two passes, the
    second of which reads what ONE pass in front of it wrote"""
    rc, res, _, _, passes = run_twin(tw, Dict(CORPUS["radix-257"]), max_rounds=1, mode=GRID)
    assert rc == 0 and res.depth == 8 and passes == 2


def test_capacity_and_empty(tw):
    d = Dict([b"b", b"a", b"c"])
    rc, res, srt, rnk, _ = run_twin(tw, d, capacity=2, flags=0)
    assert (rc, res.code, res.n_entries, res.depth, res.n_tied, res.n_values) == (0, MSJ_CAPACITY, 3, 0, 0, 0)
    assert (srt == FILL32).all() and (rnk == FILL32).all()
    e = Dict([])
    rc, res, srt, rnk, _ = run_twin(tw, e, capacity=4)
    assert (rc, res.code, res.flags, res.n_entries, res.depth) == (0, 0, 0, 0, 0) and (srt == FILL32).all()


def test_argument_checks(tw):
    d = Dict([b"b", b"a"])
    assert run_twin(tw, d, ctx_ok=0)[0] == BAD_ARGUMENT
    assert run_twin(tw, d, flags=2)[0] == BAD_ARGUMENT
    assert run_twin(tw, d, max_rounds=65)[0] == BAD_ARGUMENT
    assert run_twin(tw, d, depth=4, flags=CONTINUE)[0] == BAD_ARGUMENT
    assert run_twin(tw, d, depth=8)[0] == BAD_ARGUMENT  # a depth without CONTINUE
    rc, res, srt, rnk, _ = run_twin(tw, d, flags=2)
    assert (srt == FILL32).all() and (rnk == FILL32).all() and res.code != 0  # nothing written: the fill


def test_garbage_state_stays_inside(tw):
    """CONTINUE over arrays from anywhere: in bounds (the arrays are exact and the sanitizer program repeats this), and it
    terminates within the budget"""
    rng = random.Random(11)
    for _ in range(200):
        vals = [None if rng.random() < 0.1 else word(rng, rng.randrange(0, 20)) for _ in range(rng.randrange(1, 30))]
        d = Dict(vals)
        srt = np.array([rng.choice((rng.randrange(d.V), rng.randrange(1 << 32), d.V)) for _ in range(d.V)], dtype=np.uint32)
        rnk = np.array([rng.choice((rng.randrange(d.V), rng.randrange(1 << 32), 0, NO_RANK)) for _ in range(d.V)], dtype=np.uint32)
        for mode in (GRID, GROUP):
            rc, res, s2, r2, _ = run_twin(tw, d, depth=8 * rng.randrange(3), max_rounds=rng.choice((1, 3, 64)), flags=CONTINUE, mode=mode, state=(srt, rnk))
            assert rc == 0 and res.n_entries == d.V and res.depth <= 16 + 8 * 64


def test_word_fetch_everywhere(tw):
    """Every start offset mod 8, every value end at capacity - 0 .. 8, every misalignment of the base, every depth phase"""
    rng = random.Random(5)
    for mis in range(8):
        for cap in range(0, 34):
            raw = np.array([rng.randrange(256) for _ in range(cap + mis + 8)], dtype=np.uint8)
            base = raw.ctypes.data
            shift = (-base) % 8 + mis
            data = raw[shift:shift + cap]
            for end_back in range(0, 9):
                end = cap - end_back
                if end < 0:
                    continue
                for begin in range(max(0, end - 19), end + 1):
                    for depth in (0, 8, 16):
                        w, nv = ctypes.c_uint64(0), ctypes.c_uint32(0)
                        tw.dom_fetch_word(base + shift, cap, begin, end - begin, depth, ctypes.addressof(w), ctypes.addressof(nv))
                        have = bytes(data[begin:end])[depth:depth + 8]
                        assert nv.value == len(have)
                        assert w.value == int.from_bytes(have.ljust(8, b"\x00"), "big"), (mis, cap, begin, end, depth)


def test_digits_and_paths(tw):
    assert [tw.dom_key_digits(c) for c in (0, 1, 2, 256, 257, 65536, 65537, 1 << 20, 1 << 31, 1 << 40)] == [9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
    assert tw.dom_digit(0x0102030405060708, 0x0A0B0C, 5, 0) == 5
    assert [tw.dom_digit(0x0102030405060708, 0x0A0B0C, 5, d) for d in range(1, 9)] == [8, 7, 6, 5, 4, 3, 2, 1]
    assert [tw.dom_digit(0x0102030405060708, 0x0A0B0C, 5, d) for d in range(9, 13)] == [0x0C, 0x0B, 0x0A, 0]
    assert [tw.dom_use_group_path(c, m) for c, m in ((1024, AUTO), (1025, AUTO), (1024, GRID), (1025, GROUP), (0, GROUP))] == [1, 0, 0, 0, 1]
    assert tw.dom_rounds_of(0, 1) == 64 and tw.dom_rounds_of(0, 0) == 4 and tw.dom_rounds_of(7, 0) == 7


# ---- msj_rank_rows_device ---------------------------------------------------------------------------------------------------

def py_rank_records(codes, R, rank, V):
    out = np.zeros(R, dtype=FIELD)
    counts = [0, 0, 0]
    for k in range(R):
        c = int(codes[k])
        if 0 <= c < V and rank[c] != NO_RANK:
            out[k] = (rank[c], 0xFFFFFFFF, ord("l"), 0, 0)
            counts[0] += 1
        else:
            out[k] = (0, 0xFFFFFFFF, 0, 0, 20)
            counts[1 if c == -1 else 2] += 1
    return out, counts


def run_rank_rows(tw, codes, rank, order, rows=None, capacity=None, n_rows=None, rank_capacity=None):
    rows = len(codes) if rows is None else rows
    capacity = rows if capacity is None else capacity
    fields = np.frombuffer(b"\xA5" * (16 * capacity), dtype=FIELD).copy()
    res, sel = RankRowsResult(), SelectResult()
    ctypes.memset(ctypes.byref(res), 0xA5, ctypes.sizeof(res))
    ctypes.memset(ctypes.byref(sel), 0xA5, ctypes.sizeof(sel))
    n = None if n_rows is None else np.array([n_rows], dtype=np.uint64)
    rc = tw.dom_rank_rows(1, ptr(codes), rows, ptr(n), ptr(rank), len(rank) if rank_capacity is None else rank_capacity,
                          ctypes.addressof(order), ptr(fields), capacity, ctypes.addressof(res), ctypes.addressof(sel))
    return rc, res, sel, fields


def test_rank_rows(tw):
    vals = [b"pear", None, b"apple", b"fig", b"apple"]
    d = Dict(vals)
    _, order, srt, rnk, _ = run_twin(tw, d, max_rounds=64)
    codes = np.array([0, 2, -1, -2, 5, 1, 3, 4, 2, 1 << 30, -(1 << 31)], dtype=np.int32)
    rc, res, sel, fields = run_rank_rows(tw, codes, rnk, order, capacity=len(codes) + 2, n_rows=len(codes) - 1)
    want, counts = py_rank_records(codes, len(codes) - 1, list(rnk), d.V)
    assert rc == 0 and res.code == 0 and sel.code == 0
    assert fields[:len(want)].tobytes() == want.tobytes() and fields[len(want):].tobytes() == b"\xA5" * (16 * 3)
    assert [res.n_rows, res.n_ranked, res.n_null, res.n_unknown] == [len(want)] + counts
    assert (sel.n_documents, sel.n_paths, sel.n_found, sel.n_no_bits) == (len(want), 1, counts[0], 0)
    # a code in the order result passes through, the tied MSJ_CAPACITY included
    _, tied, _, rnk1, _ = run_twin(tw, Dict([b"a" * 9, b"a" * 10]), max_rounds=1)
    assert tied.code == MSJ_CAPACITY and tied.n_tied == 2
    rc, res, sel, fields = run_rank_rows(tw, codes, rnk1, tied)
    assert (rc, res.code, sel.code, res.n_rows, sel.n_documents) == (0, MSJ_CAPACITY, MSJ_CAPACITY, 0, 0)
    assert fields.tobytes() == b"\xA5" * (16 * len(codes))
    # the rooms
    for kw in (dict(n_rows=len(codes) + 1), dict(capacity=len(codes) - 1), dict(rank_capacity=d.V - 1), dict(n_rows=1 << 31)):
        rc, res, sel, fields = run_rank_rows(tw, codes, rnk, order, **kw)
        assert (rc, res.code, sel.code) == (0, MSJ_CAPACITY, MSJ_CAPACITY) and set(fields.tobytes()) <= {0xA5}
