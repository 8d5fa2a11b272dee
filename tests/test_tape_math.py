"""CPU check of the arithmetic of msj_tape_device (mojo_simdjson_amd/csrc/tape_math.h).

The header is compiled for the host with g++ (tests/tape_math_host.cpp).  Two steps: tests/tape_reference.py, a plain serial
tape builder written from the definition in include/msj_stage1.h, is pinned against Python's json (decode the tape back to
a value, floats by bit pattern); then the twin -- words per token, the word encoders, the count rule over d_match / d_depth,
the unescape serially and 64 bytes per step -- gives the same words and bytes as that builder on the same corpus.  The
kernels that run the same header on the device are covered by tests/test_tape.py (-m gpu).
"""
import ctypes
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import helpers
from tests import tape_reference as ref
from tests import test_number_math as tnm
from tests import test_validate_math as tvm

BUILD = os.path.join(helpers.ROOT, "tests", "_build")
CAPACITY = 1
STAGE2_FIXTURES = ("simple_json", "simple_strings", "escaping", "escaping_very_long")  # the reference's tests/test_stage_2.mojo


class TapeResult(ctypes.Structure):
    _fields_ = [("code", ctypes.c_int32), ("flags", ctypes.c_uint32), ("tape_words", ctypes.c_uint64),
                ("string_bytes", ctypes.c_uint64), ("n_strings", ctypes.c_uint64)]


_twin = None


def load_twin():
    """The host twin (g++ build of tests/tape_math_host.cpp), also what tests/test_tape.py compares the GPU with."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libtape_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "tape_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.tm_build.restype = None
    lib.tm_build.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 7 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 4
    lib.tm_unescape.restype = ctypes.c_uint64
    lib.tm_unescape.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_int32, ctypes.c_uint64,
                                ctypes.c_void_p, ctypes.c_uint64]
    lib.tm_words_per_token.restype = ctypes.c_uint32
    lib.tm_words_per_token.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    for name, args in (("tm_open_word", [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64]), ("tm_close_word", [ctypes.c_uint32, ctypes.c_uint64]),
                       ("tm_string_word", [ctypes.c_uint64]), ("tm_atom_word", [ctypes.c_uint32]), ("tm_number_tag_word", [ctypes.c_uint32]),
                       ("tm_root_word", [ctypes.c_int32, ctypes.c_uint64])):
        getattr(lib, name).restype = ctypes.c_uint64
        getattr(lib, name).argtypes = args
    lib.tm_is_direct_comma.restype = ctypes.c_int32
    lib.tm_is_direct_comma.argtypes = [ctypes.c_uint32, ctypes.c_int32, ctypes.c_int32]
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def tm():
    return load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


def number_records(nm, data, idx, flags):
    """(bits uint64[k], kinds uint32[k]) of the number tokens in token order, from the host twin of the number call."""
    num = np.nonzero(flags & 4)[0]
    bits = np.zeros(max(num.size, 1), dtype=np.uint64)
    kinds = np.zeros(max(num.size, 1), dtype=np.uint32)
    if num.size:
        starts = np.ascontiguousarray(idx[num], dtype=np.uint64)
        paths = np.zeros(3, dtype=np.uint64)
        nm.nm_convert_batch(data, len(data), starts.ctypes.data, num.size, bits.ctypes.data, kinds.ctypes.data, paths.ctypes.data)
    return bits[:num.size], kinds[:num.size], num


def host_arrays(oracle, nm, data):
    """What stage 1 + msj_stage2_prep_device(match) + msj_number_values_device leave for `data`, from the oracles: a dict,
    or the stage-1 code when that is not 0."""
    rc, n, idx = helpers.run_oracle(oracle.msj_oracle_stage1, data)
    if rc != 0:
        return rc
    idx = idx[:n].copy()
    typ, depth, _ = helpers.oracle_tokens(data, idx)
    match = helpers.oracle_match(typ)
    end, flags = helpers.oracle_token_spans(data, idx)
    bits, kinds, tokens = number_records(nm, data, idx, flags)
    return dict(idx=idx, typ=typ, depth=depth, match=match, end=end, flags=flags, bits=bits, kinds=kinds, num_tokens=tokens)


def twin_build(tm, data, a, tape_capacity=None, string_capacity=None, numbers_capacity=None, strings=True, extras=False, canary=0):
    """tm_build on host arrays.  Capacities default to the reference's bounds.  -> (TapeResult, tape uint64[cap + canary],
    string buffer uint8[cap + canary] or None[, pos, counts, ulen])"""
    n = len(a["idx"])
    tcap = n + a["bits"].size + 2 if tape_capacity is None else tape_capacity
    scap = 5 * len(data) // 3 + 64 if string_capacity is None else string_capacity
    ncap = a["bits"].size if numbers_capacity is None else numbers_capacity
    tape = np.full(tcap + canary, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    sbuf = np.full(scap + canary, 0xA5, dtype=np.uint8) if strings else None
    res = TapeResult()
    ex = [np.zeros(max(n, 1), dtype=np.uint32) for _ in range(3)] if extras else [None] * 3
    arrs = [np.ascontiguousarray(a["typ"], dtype=np.uint8), np.ascontiguousarray(a["depth"], dtype=np.int32),
            np.ascontiguousarray(a["match"], dtype=np.uint32), np.ascontiguousarray(a["end"], dtype=np.uint32),
            np.ascontiguousarray(a["flags"], dtype=np.uint8)]
    idx = np.ascontiguousarray(a["idx"], dtype=np.uint32)
    bits = np.ascontiguousarray(np.concatenate([a["bits"], np.zeros(1, np.uint64)]))
    kinds = np.ascontiguousarray(np.concatenate([a["kinds"], np.zeros(1, np.uint32)]))
    tm.tm_build(bytes(data), len(data), idx.ctypes.data, n, *[x.ctypes.data for x in arrs], bits.ctypes.data, kinds.ctypes.data, ncap,
                tape.ctypes.data, tcap, sbuf.ctypes.data if strings else None, scap, ctypes.byref(res),
                *[(x.ctypes.data if x is not None else None) for x in ex])
    if extras:
        return res, tape, sbuf, ex[0][:n], ex[1][:n], ex[2][:n]
    return res, tape, sbuf


def fixture_documents():
    out = []
    for name in STAGE2_FIXTURES:
        js, _ = helpers.read_fixture(os.path.join(helpers.GOLDEN, "valid", name + ".json"))
        out.append(bytes(js))
    return out


def valid_corpus(oracle, seeded=200000):
    """(kind, document) of every valid document of the corpus: the four stage-2 fixtures, every valid text of
    tvm.seeded_documents(20260, seeded), every body of tvm.escape_cases() whose document the serial walker accepts."""
    for js in fixture_documents():
        yield "fixture", js
    for doc, _ in tvm.seeded_documents(20260, seeded):
        yield "seeded", doc
    for body in tvm.escape_cases():
        doc = tvm._string_doc(body)
        idx = tvm.stage1(oracle, doc)
        if idx is not None and tvm.walk(doc, idx.tolist()) == (tvm.SUCCESS, None):
            yield "escape", doc


def check_twin_equals_reference(tm, data, a, want_tape, want_sbuf):
    res, tape, sbuf = twin_build(tm, data, a, canary=8)
    assert (res.code, res.flags, res.tape_words, res.string_bytes) == (0, 0, len(want_tape), len(want_sbuf)), data[:200]
    assert tape[:len(want_tape)].tolist() == want_tape, data[:200]
    assert sbuf[:len(want_sbuf)].tobytes() == want_sbuf, data[:200]
    assert res.n_strings == int(np.count_nonzero(a["typ"] == 0x22))
    cap_t, cap_s = len(tape) - 8, len(sbuf) - 8
    assert (tape[cap_t:] == 0xA5A5A5A5A5A5A5A5).all() and (sbuf[cap_s:] == 0xA5).all()


def test_corpus_reference_against_json_and_twin_against_reference(oracle, tm, nm):
    """tape_reference.build decoded back equals json.loads (objects as lists of pairs, floats by bit pattern); the twin's
    words and bytes equal tape_reference's.  Every seeded text must be valid: a generator change fails here, it does not
    thin the corpus."""
    compared = {"fixture": 0, "seeded": 0, "escape": 0}
    for kind, doc in valid_corpus(oracle):
        a = host_arrays(oracle, nm, doc)
        assert not isinstance(a, int), doc
        idx = a["idx"]
        assert tvm.walk(doc, idx.tolist()) == (tvm.SUCCESS, None), doc
        tape, sbuf = ref.build(doc, idx)
        want = json.loads(doc.decode("utf-8"), object_pairs_hook=list)
        got = ref.decode(tape, sbuf)
        assert ref.same(got, want), (doc[:200], got, want)
        check_twin_equals_reference(tm, doc, a, tape, sbuf)
        compared[kind] += 1
    assert compared["fixture"] == 4 and compared["seeded"] == 200000 and compared["escape"] >= 40, compared
    assert sum(compared.values()) >= 200000


def test_words_and_encoders(tm):
    for t in range(256):
        for fl in (0, 1, 2, 3, 4, 12, 36):
            want = 2 if fl & 4 else (1 if t in b'{}[]"tfn' else 0)
            assert tm.tm_words_per_token(t, fl) == want, (t, fl)
    assert tm.tm_root_word(0, 7) == (ord("r") << 56) | 7 and tm.tm_root_word(1, 7) == ord("r") << 56
    assert tm.tm_open_word(ord("["), 3, 9) == (ord("[") << 56) | (3 << 32) | 10
    assert tm.tm_open_word(ord("{"), 0, 4) == (ord("{") << 56) | 5
    assert tm.tm_open_word(ord("["), 0xFFFFFF, 1) == (ord("[") << 56) | (0xFFFFFF << 32) | 2
    assert tm.tm_open_word(ord("["), 0x1000000, 1) == (ord("[") << 56) | (0xFFFFFF << 32) | 2  # deviation 3: saturates
    assert tm.tm_open_word(ord("["), 1 << 40, 1) == (ord("[") << 56) | (0xFFFFFF << 32) | 2
    assert tm.tm_close_word(ord("]"), 5) == (ord("]") << 56) | 5
    assert tm.tm_string_word(1 << 33) == (0x22 << 56) | (1 << 33)
    assert tm.tm_atom_word(ord("n")) == ord("n") << 56
    assert tm.tm_number_tag_word(tnm.INT64) == ord("l") << 56 and tm.tm_number_tag_word(tnm.DOUBLE) == ord("d") << 56
    assert tm.tm_is_direct_comma(ord(","), 3, 2) == 1 and tm.tm_is_direct_comma(ord(","), 4, 2) == 0
    assert tm.tm_is_direct_comma(ord(":"), 3, 2) == 0 and tm.tm_is_direct_comma(ord(","), 2, 2) == 0


def test_words_by_hand(oracle, tm, nm):
    """The layout of the issue's examples, word for word, without the reference builder."""
    doc = b'{"a":[1,-2.5,true],"b\\n":null,"c":{},"d":[]}'
    a = host_arrays(oracle, nm, doc)
    res, tape, sbuf = twin_build(tm, doc, a)
    W = lambda c, p=0: (ord(c) << 56) | p
    dbl = struct.unpack("<Q", struct.pack("<d", -2.5))[0]
    # positions: '{' 1, "a" 2, '[' 3, 1 -> 4 5, -2.5 -> 6 7, true 8, ']' 9, "b\n" 10, null 11, "c" 12, '{' 13, '}' 14, "d" 15,
    # '[' 16, ']' 17, '}' 18, root 19: 20 words
    want = [W("r", 20), W("{", (4 << 32) | 19), W('"', 0), W("[", (3 << 32) | 10), W("l"), 1, W("d"), dbl, W("t"), W("]", 3),
            W('"', 5), W("n"), W('"', 11), W("{", 15), W("}", 13), W('"', 16), W("[", 18), W("]", 16), W("}", 1), W("r")]
    assert tape[:res.tape_words].tolist() == want
    assert sbuf[:res.string_bytes].tobytes() == b"\x01\0\0\0a\x02\0\0\0b\n\x01\0\0\0c\x01\0\0\0d"
    assert (res.code, res.tape_words, res.string_bytes, res.n_strings) == (0, 20, 21, 4)


def test_counts(oracle, tm, nm):
    doc = b'[[1,2],[3,4,5],[],{"a":1,"b":[]}]'
    a = host_arrays(oracle, nm, doc)
    _, tape, _, pos, counts, _ = twin_build(tm, doc, a, extras=True)
    opens = [i for i, t in enumerate(a["typ"]) if t in b"[{"]
    assert [int(counts[i]) for i in opens] == [3, 1, 2, 0, 1, 0]  # direct commas: siblings do not leak into each other
    assert [(int(tape[pos[i]]) >> 32) & 0xFFFFFF for i in opens] == [4, 2, 3, 0, 2, 0]
    deep = b"[" * 300 + b"1,2" + b"]" * 300
    a = host_arrays(oracle, nm, deep)
    _, tape, _, pos, counts, _ = twin_build(tm, deep, a, extras=True)
    assert [(int(tape[pos[i]]) >> 32) & 0xFFFFFF for i in range(300)] == [1] * 299 + [2]


def unescape(tm, body, which, cut=0):
    buf = b'"' + body + b'"'
    out = np.full(len(body) + 8, 0xA5, dtype=np.uint8)
    n = tm.tm_unescape(buf, len(buf), 1, 1 + len(body), which, 1 + cut, out.ctypes.data, len(body))
    assert (out[len(body):] == 0xA5).all()
    return out[:n].tobytes()


def test_unescape_cut_at_every_position(tm):
    """The 64-bytes-per-step walk, whole and with a step cut short at every position of the body, gives the serial walk's
    bytes -- where the body is one run of backslashes, and with surrogate pairs at every phase of a 64-byte step."""
    bodies = [(body, bad) for body, bad in tvm.backslash_run_bodies(1025)]
    pair = b"\\ud83d\\ude00"
    for phase in range(64):
        bodies.append((b"a" * phase + pair * 7 + b"\\u00e9\\u20ac\\n\\\\" + b"z" * 3, False))
    checked = 0
    for body, bad in bodies:
        want = unescape(tm, body, 0)
        if not bad:
            assert want == ref.unescape(b'"' + body + b'"', 0), body[-40:]
            checked += 1
        assert unescape(tm, body, 1) == want, body[-40:]
        for cut in range(1, len(body)):
            assert unescape(tm, body, 2, cut) == want, (body[-40:], cut)
    assert checked > 64


def test_unescape_against_reference_on_escape_cases(oracle, tm):
    n = 0
    for body in tvm.escape_cases():
        doc = tvm._string_doc(body)
        idx = tvm.stage1(oracle, doc)
        if idx is None or tvm.walk(doc, idx.tolist()) != (tvm.SUCCESS, None):
            continue
        want = ref.unescape(doc, 1)
        assert unescape(tm, body, 0) == want and unescape(tm, body, 1) == want, body
        for cut in range(1, len(body)):
            assert unescape(tm, body, 2, cut) == want, (body, cut)
        n += 1
    assert n >= 40  # 8 simple escapes, 12 forms of a \u escape outside the surrogates, 4 pairs, the even runs of backslashes
    for body, want in ((b"\\u0041", b"A"), (b"\\u00e9", b"\xc3\xa9"), (b"\\u20ac", b"\xe2\x82\xac"), (b"\\ud83d\\ude00", b"\xf0\x9f\x98\x80"),
                       (b'\\"\\\\\\/\\b\\f\\n\\r\\t', b'"\\/\b\f\n\r\t'), (b"\\u0000", b"\0")):
        assert unescape(tm, body, 0) == want and unescape(tm, body, 1) == want


def test_capacities_clip(oracle, tm, nm):
    doc = b'{"k":["abc",1.5,"\\u20ac"],"z":-7}'
    a = host_arrays(oracle, nm, doc)
    full, tape, sbuf = twin_build(tm, doc, a)
    for kw in (dict(tape_capacity=full.tape_words - 1), dict(string_capacity=full.string_bytes - 1), dict(numbers_capacity=1)):
        res, t2, s2 = twin_build(tm, doc, a, canary=8, **kw)
        assert (res.code, res.tape_words, res.string_bytes, res.n_strings) == (CAPACITY, full.tape_words, full.string_bytes, full.n_strings)
        assert (t2[len(t2) - 8:] == 0xA5A5A5A5A5A5A5A5).all() and (s2[len(s2) - 8:] == 0xA5).all()
    res, t3, _ = twin_build(tm, doc, a, strings=False)
    assert res.code == 0 and res.string_bytes == full.string_bytes and t3[:full.tape_words].tolist() == tape[:full.tape_words].tolist()
