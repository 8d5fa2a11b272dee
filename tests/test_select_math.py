"""CPU check of the lookup of msj_select_documents_device (mojo_simdjson_amd/csrc/select_math.h).

The definition in include/msj_stage1.h is restated in Python from its text alone (tests/select_reference.py: json with a
hook that keeps the first of duplicate keys, then a walk over the keys -- no tokens, depths or partners).  The host twin
(tests/select_math_host.cpp: the state words, the member test, the key compare and the record of select_math.h, one serial
lookup per (path, document)) runs over the oracles' arrays of a window; for every (path, document) its code must be the
reference's, and its record decoded back to a Python value -- as Window.values does it -- must be the reference's value.
The kernels that run the same header on the device are covered by tests/test_select_documents.py (-m gpu).
"""
import ctypes
import functools
import os
import random
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document_stream import FIELD_DTYPE, field_value
from tests import helpers
from tests import select_reference as ref
from tests import test_number_math as tnm
from tests import test_tape_documents_math as tdk
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

MSJ_CAPACITY = 1
FILL = 0x77
CANARY = 4          # records behind n_paths * capacity: 64 bytes
NO_TOKEN = 0xFFFFFFFF
PINS = [b'{"a":1,"a":2}', b'{"x":{"a":1},"a":2}', b'{"x":"a","a":3}', b'{"a\\u0062":1}', b'{"a\\/b":1}', b'{"":5}',
        b'{"a":1,"a":{"b":2}}', b'[{"a":1}]', b'{"a":[{"b":1}]}', b"7", b'"s\\n"', b"null", b'{"0":7}', b"[7]",
        b'{"a":{"b":{"a":-2.5e3}},"ab":[1,{"a":2}]}', b"{}"]
PIN_PATHS = ["/a", "/ab", "/a~1b", "/", "/a/b", "", "/0", "/a/b/a"]

_twin = None


def load_twin():
    """The host twin of the call (g++ build of tests/select_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libselect_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "select_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    vp, u64, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32
    for name, args, res in (("sm_paths_bytes", [], u64),
                            ("sm_compile_paths", [ctypes.POINTER(ctypes.c_char_p), u32, vp, vp], ctypes.c_int),
                            ("sm_segment", [vp, u32, u32, vp], ctypes.c_int),
                            ("sm_select_documents", [vp, ctypes.c_char_p, u64, vp, u64] + [vp] * 8 + [u64, vp, vp, vp, u64, vp], None),
                            ("sm_state_code", [u32], u32), ("sm_state_to_code", [u32], u32),
                            ("sm_length_may_match", [u64, ctypes.c_int, u32], ctypes.c_int),
                            ("sm_key_equals", [ctypes.c_char_p, u64, u64, u64, ctypes.c_int, ctypes.c_char_p, u32], ctypes.c_int),
                            ("sm_find_number", [vp, u64, u32], ctypes.c_int64)):
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
    return load_twin()


# ---- the twin ---------------------------------------------------------------------------------------------------------------

def compile_paths(stwin, pointers):
    """-> (0 / 22 / -1, the compiled blob, segments per path)"""
    raw = [p.encode("utf-8") if isinstance(p, str) else p for p in pointers]
    table = (ctypes.c_char_p * max(len(raw), 1))(*raw)
    blob = np.zeros(stwin.sm_paths_bytes(), dtype=np.uint8)
    levels = np.zeros(16, dtype=np.uint32)
    rc = stwin.sm_compile_paths(table, len(raw), blob.ctypes.data, levels.ctypes.data)
    return rc, blob, levels[:len(raw)].tolist()


class Selected:
    """What one call left: the result, every record with the canary behind them, the capacity it was given."""

    def __init__(self, res, fields, n_paths, capacity):
        self.res, self.fields, self.n_paths, self.capacity = res, fields, n_paths, capacity

    def column(self, p):
        return self.fields[p * self.capacity:(p + 1) * self.capacity]

    def summary(self):
        r = self.res
        return (r.code, r.flags, r.n_documents, r.n_paths, r.n_found, r.n_no_bits, r.reserved)

    def untouched(self, lo_k):
        """Records k >= lo_k of every path, and the canary, are as they were filled"""
        raw = self.fields.view(np.uint8).reshape(-1, 16)
        rows = [raw[p * self.capacity + lo_k:(p + 1) * self.capacity] for p in range(self.n_paths)] + [raw[self.n_paths * self.capacity:]]
        return all(bool((r == FILL).all()) for r in rows)


def filled_fields(n_paths, capacity):
    return np.frombuffer(bytes([FILL]) * (16 * (n_paths * capacity + CANARY)), dtype=FIELD_DTYPE).copy()


def twin_select(stwin, w, pointers, verdicts=None, numbers=True, numbers_result=True, capacity=None, numbers_capacity=None):
    """sm_select_documents over the window's arrays.  verdicts: [(code, token)] per document or None (d_verdicts NULL);
    numbers False: d_numbers NULL with capacity 0; numbers_result False: d_numbers_result NULL.  -> Selected"""
    rc, blob, _ = compile_paths(stwin, pointers)
    assert rc == 0, (rc, pointers)
    capacity = max(w.D, 1) if capacity is None else capacity
    fields = filled_fields(len(pointers), capacity)
    docs = _lib.MsjDocumentsResult(*w.docs)
    res = _lib.MsjSelectDocumentsResult()
    ncap = (int(w.records.size) if numbers_capacity is None else numbers_capacity) if numbers else 0
    recs = np.ascontiguousarray(w.records[:ncap])
    nr = w.numbers_result()
    rows = tdk.verdict_rows(verdicts) if verdicts is not None else None
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags, w.first)]
    stwin.sm_select_documents(blob.ctypes.data, w.data, len(w.data), arrs[0].ctypes.data, w.n, *[a.ctypes.data for a in arrs[1:]],
                              ctypes.byref(docs), recs.ctypes.data if ncap else None, ncap, ctypes.byref(nr) if numbers_result else None,
                              rows.ctypes.data if rows is not None else None, fields.ctypes.data, capacity, ctypes.byref(res))
    return Selected(res, fields, len(pointers), capacity)


# ---- against the definition ---------------------------------------------------------------------------------------------------

def same_value(a, b):
    """Equal, and of the same kind: True is not 1 and 1 is not 1.0"""
    if isinstance(a, dict) and isinstance(b, dict):
        return list(a) == list(b) and all(same_value(a[k], b[k]) for k in a)
    if isinstance(a, list) and isinstance(b, list):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return type(a) is type(b) and a == b


def check_against_reference(w, got, pointers, texts, codes=None, bits=True):
    """Every record of `got` (a Selected with room for every document) against tests/select_reference.py on the documents'
    texts.  codes: the verdict's code per document (None: all 0).  -> {(p, k): (code, value)}"""
    codes = [0] * w.D if codes is None else list(codes)
    assert len(texts) >= w.D
    data = np.frombuffer(w.data, dtype=np.uint8)
    decoded = [None if codes[k] else ref.decode(texts[k]) for k in range(w.D)]
    starts = w.first[:w.D].tolist()
    ends = starts[1:] + [w.T]
    out, found, no_bits = {}, 0, 0
    for p, pointer in enumerate(pointers):
        # the column's records as Python values, read once: a window of 260 000 documents is walked here too
        col = {name: got.column(p)[name][:w.D].tolist() for name in FIELD_DTYPE.names}
        for k in range(w.D):
            r = {name: col[name][k] for name in FIELD_DTYPE.names}
            where = (pointer, k, texts[k][:100], r)
            f, e = starts[k], ends[k]
            if codes[k]:
                want = (codes[k], None)
            else:
                want = ref.lookup(decoded[k], pointer)
            assert r["code"] == want[0], where
            if want[0]:
                assert (r["bits"], r["token"], r["type"], r["flags"]) == (0, NO_TOKEN, 0, 0), where
                value = None
            else:
                assert f <= r["token"] < e and chr(r["type"]) in '{["ldtfn', where
                if bits:
                    assert not r["flags"] & _lib.FIELD_NO_BITS, where
                value = field_value(r, data, w.idx, w.end)
                assert same_value(value, want[1]), where + (value, want[1])
                found += 1
                no_bits += bool(r["flags"] & _lib.FIELD_NO_BITS)
            out[(p, k)] = (want[0], value)
    assert got.summary() == (0, 0, w.D, len(pointers), found, no_bits, 0), got.summary()
    assert got.untouched(w.D)
    return out


def usable(keys):
    """Can this chain of keys be named by a pointer of the call: its limits, and no NUL byte in a C string"""
    if not 0 < len(keys) <= ref.MAX_SEGMENTS:
        return False
    try:
        return all(len(k.encode("utf-8")) <= ref.MAX_SEGMENT_BYTES and "\0" not in k for k in keys)
    except UnicodeEncodeError:
        return False


def draw_paths(rng, texts):
    """Up to 16 pointers for a stream: some of its documents' own chains of keys, the root, an absent key, and prefixes and
    extensions of present keys (`ab` against `abc`), as a last segment and as one on the way"""
    chains = set()
    for t in texts:
        chains |= {c for c in ref.key_paths(ref.decode(t)) if usable(c)}
    chains = sorted(chains)
    own = rng.sample(chains, min(8, len(chains)))
    deep = sorted(chains, key=len)[-2:]   # the longest ones always
    out = [""] + [ref.pointer_of(c) for c in own + deep] + ["/no such key"]
    for c in own[:3]:
        out.append(ref.pointer_of(c[:-1] + (c[-1] + "x",)))           # an extension
        if c[-1]:
            out.append(ref.pointer_of(c[:-1] + (c[-1][:-1],)))        # a prefix
        out.append(ref.pointer_of(c + ("zz",)))                        # one level too far
    seen, uniq = set(), []
    for p in out:
        if p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq[:ref.MAX_PATHS]


@functools.lru_cache(maxsize=None)
def corpus():
    """[(stream, its documents, pointers)]: the tape tests' corpus (fixtures, escape cases and 2 048 seeded documents in
    streams of 64, joined by each of the four separators) with the pointers drawn for each stream"""
    rng = random.Random(20270)
    return [(data, docs, draw_paths(rng, docs)) for data, docs in tdk.corpus_streams()]


def pin_stream():
    return tdk.join(PINS, b"\n"), PINS, PIN_PATHS


# ---- tests ------------------------------------------------------------------------------------------------------------------

def test_corpus_equals_reference(oracle, nm, stwin):
    """Every (path, document) of every stream: the code and the decoded value are the reference's; with d_verdicts NULL
    and with all-zero verdicts."""
    n_docs, hist = 0, {}
    for j, (data, docs, pointers) in enumerate(corpus()):
        w = tdm.WindowArrays(oracle, nm, data, is_final=True)
        assert w.D == len(docs), (j, w.D, len(docs))
        got = twin_select(stwin, w, pointers, verdicts=[(0, tvm.UINT64_MAX)] * w.D if j % 2 else None)
        for (c, _) in check_against_reference(w, got, pointers, docs).values():
            hist[c] = hist.get(c, 0) + 1
        n_docs += w.D
    assert n_docs >= 2048 + 4 * 44
    assert all(hist.get(c, 0) > 500 for c in (0, 17, 20)), hist


def test_pins(oracle, nm, stwin):
    """The cases read from the definition, one window."""
    data, docs, pointers = pin_stream()
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    assert w.D == len(docs)
    got = check_against_reference(w, twin_select(stwin, w, pointers), pointers, docs)
    at = lambda text, pointer: got[(pointers.index(pointer), docs.index(text))]
    assert at(b'{"a":1,"a":2}', "/a") == (0, 1)                      # the first duplicate wins
    assert at(b'{"x":{"a":1},"a":2}', "/a") == (0, 2)                # a deeper key must not match
    assert at(b'{"x":"a","a":3}', "/a") == (0, 3)                    # a value string is no key
    assert at(b'{"a\\u0062":1}', "/ab") == (0, 1)
    assert at(b'{"a\\/b":1}', "/a~1b") == (0, 1)
    assert at(b'{"":5}', "/") == (0, 5)
    assert at(b'{"a":1,"a":{"b":2}}', "/a/b") == (17, None)          # ... also when a later duplicate would do
    assert at(b'[{"a":1}]', "/a") == (17, None)
    assert at(b'{"a":[{"b":1}]}', "/a/b") == (17, None)
    assert at(b"7", "") == (0, 7) and at(b'"s\\n"', "") == (0, "s\n") and at(b"null", "") == (0, None)
    assert at(b"7", "/a") == (17, None) and at(b"{}", "/a") == (20, None) and at(b"{}", "") == (0, {})
    assert at(b'{"0":7}', "/0") == (0, 7) and at(b"[7]", "/0") == (17, None)
    assert at(PINS[14], "/a/b/a") == (0, -2500.0) and at(PINS[14], "/ab") == (0, [1, {"a": 2}]) and at(PINS[14], "/a/b") == (0, {"a": -2500.0})


def test_invalid_documents_report_their_code(oracle, nm, vtwin, stwin):
    """One document of every verdict code between valid ones: every path's record of it has that code and nothing else;
    its neighbours are exact.  Without verdicts every document is looked up and the valid ones give the same records."""
    valid = [doc for doc, _ in tvm.seeded_documents(20260, 64)]
    data, docs, bad = tdk.mixed_stream(valid)
    pointers = draw_paths(random.Random(5), [d for k, d in enumerate(docs) if k not in bad])
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    verdicts, _ = tdm.twin_documents(vtwin, w, 3)
    codes = [c for c, _ in verdicts]
    assert all(codes[k] == c for k, c in bad.items()) and set(codes) >= set(tdk.CODES) | {0}
    got = twin_select(stwin, w, pointers, verdicts=verdicts)
    check_against_reference(w, got, pointers, docs, codes=codes)
    free = twin_select(stwin, w, pointers)
    assert free.untouched(w.D)
    for p in range(len(pointers)):
        for k in range(w.D):
            if not codes[k]:
                assert free.column(p)[k] == got.column(p)[k]


def test_cut_window_no_document_and_capacity(oracle, nm, stwin):
    """A cut last document (not final): it has no record.  A window without a complete document, and one without a token:
    a zero result.  A capacity one short: MSJ_CAPACITY, n_documents = D, no record written."""
    docs = [b'{"a":[1,2,{"b":"x\\ny"}],"cut":1}', b"[1.5,true]", b'{"cut":"s"}']
    pointers = ["/cut", "/a", ""]
    w = tdm.WindowArrays(oracle, nm, b" ".join(docs) + b' {"cut":[1,"abc', is_final=False)
    assert (w.docs[0], w.D) == (4, 3) and w.T < w.n
    got = twin_select(stwin, w, pointers, capacity=5)
    out = check_against_reference(w, got, pointers, docs)
    assert [out[(0, k)] for k in range(3)] == [(0, 1), (17, None), (0, "s")]
    for data in (b'{"cut":[1,"abc', b"  \n "):
        w0 = tdm.WindowArrays(oracle, nm, data, is_final=False)
        assert w0.D == 0
        got = twin_select(stwin, w0, pointers)
        assert got.summary() == (0, 0, 0, 3, 0, 0, 0) and got.untouched(0)
    short = twin_select(stwin, w, pointers, capacity=w.D - 1)
    assert short.summary() == (MSJ_CAPACITY, 0, w.D, 3, 0, 0, 0) and short.untouched(0)


def test_numbers_without_records(oracle, nm, stwin):
    """d_numbers NULL, d_numbers_result NULL, or fewer records than the field's: MSJ_FIELD_NO_BITS, bits 0 and the right
    tag; the value comes from the text.  With the records: the bits."""
    docs = [b'{"i":-12,"f":1.5e2,"s":"x","z":0.0}', b'{"f":3,"i":4.25}', b'{"i":9223372036854775807,"f":-0}']
    pointers = ["/i", "/f", "/s", "/z"]
    w = tdm.WindowArrays(oracle, nm, tdk.join(docs, b"\n"), is_final=True)
    full = twin_select(stwin, w, pointers)
    check_against_reference(w, full, pointers, docs)
    assert [chr(int(t)) for t in full.column(0)[:3]["type"]] == ["l", "d", "l"] and int(full.column(0)[2]["bits"]) == (1 << 63) - 1
    for kw in (dict(numbers=False), dict(numbers_result=False)):
        got = twin_select(stwin, w, pointers, **kw)
        check_against_reference(w, got, pointers, docs, bits=False)
        assert got.res.n_no_bits == 7 and got.res.n_found == full.res.n_found
        for p in range(4):
            for k in range(3):
                a, b = got.column(p)[k], full.column(p)[k]
                assert (a["type"], a["token"], a["code"]) == (b["type"], b["token"], b["code"])
                if chr(int(b["type"])) in "ld" and not b["code"]:
                    assert (int(a["bits"]), int(a["flags"])) == (0, _lib.FIELD_NO_BITS)
                else:
                    assert a == b
    part = twin_select(stwin, w, pointers, numbers_capacity=3)    # the first document's records only
    check_against_reference(w, part, pointers, docs, bits=False)
    assert part.res.n_no_bits == 4 and np.array_equal(part.column(0)[:1], full.column(0)[:1])
    recs = np.ascontiguousarray(w.records)
    for j, t in enumerate(recs["token"].tolist()):
        assert stwin.sm_find_number(recs.ctypes.data, recs.size, t) == j
        assert stwin.sm_find_number(recs.ctypes.data, j, t) == -1 and stwin.sm_find_number(recs.ctypes.data, recs.size, t + 1) == -1


def test_escaped_key_lengths(oracle, nm, stwin):
    """An escaped key can only match a segment s when its raw length lies in [len(s), 6 * len(s)]: one of exactly 6 * len(s)
    bytes matches, one byte more cannot; the longest key the call can name, 255 x \\u0061."""
    assert [stwin.sm_length_may_match(raw, 1, 2) for raw in (1, 2, 12, 13)] == [0, 1, 1, 0]
    assert [stwin.sm_length_may_match(raw, 0, 2) for raw in (1, 2, 3)] == [0, 1, 0]
    assert stwin.sm_length_may_match(0, 0, 0) == 1 and stwin.sm_length_may_match(2, 1, 0) == 0
    body = b"\\u0061\\u0062"
    assert stwin.sm_key_equals(body, len(body), 0, 12, 1, b"ab", 2) == 1 and stwin.sm_key_equals(body + b"c", 13, 0, 13, 1, b"ab", 2) == 0
    assert stwin.sm_key_equals(body + b"c", 13, 0, 13, 1, b"abc", 3) == 1 and stwin.sm_key_equals(body, 12, 0, 12, 1, b"ac", 2) == 0
    assert stwin.sm_key_equals(body, 12, 0, 13, 1, b"ab", 2) == 0   # an end past the buffer: never read
    long_key = b"\\u0061" * 255
    docs = [b'{"\\u0061\\u0062c":2,"\\u0061\\u0062":1}', b'{"' + long_key + b'":1,"' + long_key[:-1] + b'2":2}', b'{"\\ud83d\\ude00":"\\ud83d\\ude00"}']
    pointers = ["/ab", "/abc", "/" + "a" * 255, "/" + "a" * 254 + "b", "/\U0001F600", "/a"]
    w = tdm.WindowArrays(oracle, nm, tdk.join(docs, b"\n"), is_final=True)
    out = check_against_reference(w, twin_select(stwin, w, pointers), pointers, docs)
    assert out[(0, 0)] == (0, 1) and out[(1, 0)] == (0, 2) and out[(2, 1)] == (0, 1) and out[(3, 1)] == (0, 2)
    assert out[(4, 2)] == (0, "\U0001F600") and out[(2, 0)] == (20, None)


def test_pointer_parser(stwin):
    """RFC 6901's examples; ~01 is ~1; a bad ~ and a missing leading / are 22; beyond the limits is -1."""
    rfc = ["", "/foo", "/foo/0", "/", "/a~1b", "/c%d", "/e^f", "/g|h", "/i\\j", '/k"l', "/ ", "/m~0n", "/~01", "/a//b/", "/€/~0~1"]
    buf = np.zeros(256, dtype=np.uint8)
    for lo in range(0, len(rfc), 16):
        chunk = rfc[lo:lo + 16]
        rc, blob, levels = compile_paths(stwin, chunk)
        assert rc == 0
        for p, pointer in enumerate(chunk):
            want = ref.segments(pointer)
            assert levels[p] == len(want), pointer
            for l in range(8):
                n = stwin.sm_segment(blob.ctypes.data, p, l, buf.ctypes.data)
                assert (n, bytes(buf[:max(n, 0)])) == ((len(want[l].encode()), want[l].encode()) if l < len(want) else (-1, b"")), (pointer, l)
    assert ref.segments("/~01") == ["~1"] and ref.segments("/a~1b") == ["a/b"] and ref.segments("/") == [""]
    for bad in ("a", "a/b", "~0", "/a~", "/~2", "/a/~/b", " /a"):
        assert compile_paths(stwin, ["/ok", bad])[0] == ref.INVALID_JSON_POINTER, bad
        with pytest.raises(ValueError):
            ref.segments(bad)
    ok = ["/" + "/".join("s%d" % k for k in range(8)), "/" + "k" * 255, "/" + "~0" * 255]
    assert compile_paths(stwin, ok)[:1] + (compile_paths(stwin, ok)[2],) == (0, [8, 1, 1])
    assert compile_paths(stwin, ["/a"] * 16)[0] == 0
    for beyond in (["/a"] * 17, [], ["/" + "/".join("s%d" % k for k in range(9))], ["/" + "k" * 256], ["/a/" + "~1" * 256]):
        assert compile_paths(stwin, beyond)[0] == -1, beyond[:1]
    assert stwin.sm_state_to_code(0xFFFFFFFF) == 20 and stwin.sm_state_to_code(stwin.sm_state_code(17)) == 17
    assert stwin.sm_state_code(9) > 0x7FFFFFFF
