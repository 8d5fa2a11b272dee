"""CPU check of the per-document form of the verdict's rule (mojo_simdjson_amd/csrc/validate_docs_math.h).

msj_validate_documents_device (include/msj_stage1.h) is DEFINED as msj_validate_device's verdict on every document's token
sub-arrays.  The one-document twin (tests/validate_math_host.cpp, held against a serial walker by
tests/test_validate_math.py) run on those sub-arrays -- the whole stream as the buffer, partners rebased, the number
twin's first error over the slice -- is therefore the expected value, and the new twin (tests/validate_docs_math_host.cpp:
one loop over the window, every token behind the accessor that shows it its own document) must give the same (code, token)
for every document.  The kernels that run the same header on the device are covered by tests/test_validate_documents.py.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from tests import helpers
from tests import test_number_math as tnm
from tests import test_validate_math as tvm

UINT64_MAX = tvm.UINT64_MAX
NO_PARTNER = 0xFFFFFFFF
NUMBER_DTYPE = np.dtype([("bits", "<u8"), ("token", "<u4"), ("kind", "<u4")])    # msj_number
VERDICT_DTYPE = np.dtype([("code", "<i4"), ("reserved", "<u4"), ("error_token", "<u8")])  # msj_document_verdict
SEPARATORS = (b"\n", b" ", b"\r\n")
STREAM_DOCS = 64

_twin = None


def load_twin():
    """The host twin of the window call (g++ build of tests/validate_docs_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libvalidate_docs_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "validate_docs_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.vdm_validate_documents.restype = None
    lib.vdm_validate_documents.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    lib.vdm_docs_starting_up_to.restype = ctypes.c_uint64
    lib.vdm_docs_starting_up_to.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint64]
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def oracle():
    return helpers.load_oracle()


@pytest.fixture(scope="module")
def twin():
    return tvm.load_twin()


@pytest.fixture(scope="module")
def dtwin():
    return load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


# ---- a window's arrays, from the oracles -----------------------------------------------------------------------------

class WindowArrays:
    """What shard(is_final=False) + stage2_prep(match) + documents + number_values leave for `data`, from the oracles."""

    def __init__(self, oracle, nm, data, is_final=True):
        self.data = data = bytes(data)
        self.idx, open_string = helpers.oracle_window(oracle.msj_oracle_stage1, data)
        idx = self.idx
        self.n = int(idx.size)
        if self.n:
            self.typ, self.depth, _ = helpers.oracle_tokens(data, idx)
            self.match = helpers.oracle_match(self.typ)
            self.end, self.flags = helpers.oracle_token_spans(data, idx)
        else:
            self.typ = self.flags = np.zeros(0, dtype=np.uint8)
            self.depth = np.zeros(0, dtype=np.int32)
            self.match = self.end = np.zeros(0, dtype=np.uint32)
        self.first, self.docs = helpers.oracle_documents(data, idx, self.typ, self.depth, open_string, is_final=is_final)
        self.D, self.T = self.docs[1], self.docs[2]
        # msj_number_values_device: a record per number token, and the result
        num = np.nonzero(self.flags & 4)[0]
        self.records = np.zeros(num.size, dtype=NUMBER_DTYPE)
        self.first_error = UINT64_MAX
        self.n_errors = 0
        if num.size:
            starts = np.ascontiguousarray(idx[num], dtype=np.uint64)
            bits = np.zeros(num.size, dtype=np.uint64)
            kinds = np.zeros(num.size, dtype=np.uint32)
            paths = np.zeros(3, dtype=np.uint64)
            nm.nm_convert_batch(data, len(data), starts.ctypes.data, num.size, bits.ctypes.data, kinds.ctypes.data, paths.ctypes.data)
            bad = kinds >= tnm.ERR_SYNTAX
            self.records["bits"], self.records["token"], self.records["kind"] = np.where(bad, np.uint64(0), bits), num, kinds
            self.n_errors = int(bad.sum())
            if self.n_errors:
                self.first_error = int(num[np.nonzero(bad)[0][0]])

    def bounds(self, k):
        return int(self.first[k]), int(self.first[k + 1]) if k + 1 < self.D else self.T

    def numbers_result(self):
        return _lib.MsjNumbersResult(self.records.size, self.n_errors, self.first_error, 0)


def expected_documents(twin, nm, w, max_depths=(100,)):
    """The definition: the one-document twin on every document's sub-arrays.  -> {max_depth: [(code, window token or
    UINT64_MAX)] per document}"""
    out = {md: [] for md in max_depths}
    for k in range(w.D):
        f, e = w.bounds(k)
        m = w.match[f:e].astype(np.int64)
        inside = (m != NO_PARTNER) & (m >= f) & (m < e)
        rebased = np.where(inside, m - f, NO_PARTNER).astype(np.uint32)
        fe = tvm.numbers_first_error(nm, w.data, w.idx[f:e], w.flags[f:e])
        for md in max_depths:
            r = tvm.twin_validate(twin, w.data, w.idx[f:e], w.typ[f:e], w.depth[f:e], rebased, w.end[f:e], w.flags[f:e], fe, md)
            assert r.flags == 0
            out[md].append((r.code, UINT64_MAX if r.code == 0 else r.error_token + f))
    return out


def twin_documents(dtwin, w, max_depth=100, numbers="all", capacity=None):
    """vdm_validate_documents over the window.  numbers: "all" (every record), "none" (d_numbers_result NULL), or a
    capacity (the first so many records).  -> ([(code, token)] per document, MsjValidateDocumentsResult)"""
    cap = w.D if capacity is None else capacity
    verdicts = np.zeros(max(cap, 1), dtype=VERDICT_DTYPE)
    verdicts["code"], verdicts["error_token"] = -77, 77
    docs = _lib.MsjDocumentsResult(*w.docs)
    res = _lib.MsjValidateDocumentsResult()
    nr = None if numbers == "none" else w.numbers_result()
    ncap = w.records.size if numbers in ("all", "none") else int(numbers)
    recs = np.ascontiguousarray(w.records[:ncap])
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags, w.first)]
    idx, rest = arrs[0], arrs[1:]
    dtwin.vdm_validate_documents(w.data, len(w.data), idx.ctypes.data, w.n, *[a.ctypes.data for a in rest], ctypes.byref(docs),
                                 recs.ctypes.data if ncap else None, ncap, ctypes.byref(nr) if nr is not None else None, max_depth,
                                 verdicts.ctypes.data, cap, ctypes.byref(res))
    written = w.D if res.code == 0 else 0
    assert (verdicts["code"][written:] == -77).all() and (verdicts["error_token"][written:] == 77).all()  # nothing past D
    return [(int(c), int(t)) for c, t in zip(verdicts["code"][:written], verdicts["error_token"][:written])], res


def check_summary(res, verdicts, flags=0):
    bad = [k for k, (c, _) in enumerate(verdicts) if c != 0]
    assert (res.code, res.flags, res.n_documents, res.n_invalid) == (0, flags, len(verdicts), len(bad))
    assert res.first_invalid == (bad[0] if bad else UINT64_MAX)
    assert res.reserved == 0


# ---- the corpus (shared with the GPU test) -----------------------------------------------------------------------------

def self_contained(oracle, text):
    """Would `text` keep to itself between other texts?  Stage 1 takes it, and its brackets never go below depth 0 and
    end at depth 0 (anything else would swallow its neighbours)."""
    idx = tvm.stage1(oracle, text)
    if idx is None:
        return False
    d = 0
    for c in np.frombuffer(text, dtype=np.uint8)[idx].tolist():
        if c == 0x7B or c == 0x5B:
            d += 1
        elif c == 0x7D or c == 0x5D:
            d -= 1
            if d < 0:
                return False
    return d == 0


@functools.lru_cache(maxsize=None)
def corpus_streams():
    """(streams of 64 self-contained mutated texts of tvm.seeded_documents(20260, 20000), how many texts were kept)"""
    oracle = helpers.load_oracle()
    kept = [mut for _, mut in tvm.seeded_documents(20260, 20000) if self_contained(oracle, mut)]
    streams = []
    for s in range(0, len(kept), STREAM_DOCS):
        streams.append(SEPARATORS[(s // STREAM_DOCS) % 3].join(kept[s:s + STREAM_DOCS]))
    return streams, len(kept)


@functools.lru_cache(maxsize=None)
def corpus_expected():
    """[(WindowArrays, {100: verdicts, 3: verdicts})] per stream of the corpus: computed once, shared, never changed"""
    oracle, twin, nm = helpers.load_oracle(), tvm.load_twin(), tnm.load_twin()
    out = []
    for data in corpus_streams()[0]:
        w = WindowArrays(oracle, nm, data, is_final=True)
        out.append((w, expected_documents(twin, nm, w, (100, 3))))
    return out


def test_corpus_equals_single_document_twin(dtwin):
    """Every document of every stream: the window twin's (code, token) is the one-document twin's on the sub-arrays, at
    max_depth 100 and 3.  The one-document twin's histograms here, codes 0 / 3 / 4 / 5 / 6 / 7 / 8 / 9:
    100: 7 905 / 3 609 / 0 / 1 544 / 438 / 560 / 439 / 1 285;  3: 6 144 / 2 993 / 3 108 / 1 110 / 395 / 503 / 397 / 1 130."""
    streams, kept = corpus_streams()
    print("kept", kept, "of 20000 in", len(streams), "streams")
    assert 10000 <= kept <= 20000  # (the cap: the filter cannot hide a failure by dropping most of the corpus)
    hist = {100: {}, 3: {}}
    for w, want in corpus_expected():
        assert w.D == w.docs[0] >= 1 and w.T == w.n  # is_final: nothing is cut
        for md in (100, 3):
            got, res = twin_documents(dtwin, w, md)
            assert got == want[md], (w.data[:200], md, [(k, g, x) for k, (g, x) in enumerate(zip(got, want[md])) if g != x][:5])
            check_summary(res, got)
            for c, _ in want[md]:
                hist[md][c] = hist[md].get(c, 0) + 1
    print("codes", {md: sorted(h.items()) for md, h in hist.items()})
    for c in (0, 3, 5, 6, 7, 8, 9):
        assert hist[100].get(c, 0) > 0 and hist[3].get(c, 0) > 0, (c, hist)
    assert hist[3].get(4, 0) > 0 and hist[100].get(4, 0) == 0, hist  # DEPTH_ERROR needs the low limit on this corpus
    assert sum(hist[100].values()) == sum(hist[3].values()) >= kept


def test_valid_streams(oracle, nm, dtwin):
    """Streams of valid texts only, one per line: every document 0, as many documents as lines."""
    valid = [doc for doc, _ in tvm.seeded_documents(20260, 2000)]
    for s in range(0, len(valid), STREAM_DOCS):
        lines = valid[s:s + STREAM_DOCS]
        w = WindowArrays(oracle, nm, b"\n".join(lines), is_final=True)
        got, res = twin_documents(dtwin, w)
        assert w.D == len(lines)
        assert got == [(0, UINT64_MAX)] * len(lines)
        check_summary(res, got)


def codes(dtwin, w, **kw):
    got, res = twin_documents(dtwin, w, **kw)
    return [c for c, _ in got], got, res


def test_pins(oracle, twin, nm, dtwin):
    """Expected values from reading the definition in include/msj_stage1.h."""
    # Content checks see the window's bytes: the atom / number runs into the quote behind it.  Stage 1 starts no token at
    # a quote glued to a scalar (the index holds token 0 alone), so the split sees ONE document here, not the two a
    # reader of the bytes might expect: its verdict is the atom / number error, and there is no document 1 to be valid.
    w = WindowArrays(oracle, nm, b'true"a"')
    assert (w.n, w.D) == (1, 1)
    c, got, res = codes(dtwin, w)
    assert got == [(tvm.T_ATOM, 0)] and (res.n_invalid, res.first_invalid) == (1, 0)
    w = WindowArrays(oracle, nm, b'12"a"')
    assert (w.n, w.D) == (1, 1)
    assert codes(dtwin, w)[1] == [(tvm.NUMBER, 0)]
    # ... where the quote does start a token the scalar in front of it is closed, and both documents are valid
    w = WindowArrays(oracle, nm, b'"a"true "b"12')
    assert w.D == 4 and codes(dtwin, w)[0] == [0, 0, 0, 0]
    # a depth-0 ':' is a document of its own, and no value
    w = WindowArrays(oracle, nm, b'"a":1')
    c, got, res = codes(dtwin, w)
    assert c == [0, tvm.TAPE, 0] and got[1][1] == 1 and (res.n_invalid, res.first_invalid) == (1, 1)
    # the stray bracket starts no document: it follows the root value of the one in front
    w = WindowArrays(oracle, nm, b"[1,2]]")
    assert w.D == 1 and w.n == 6
    c, got, _ = codes(dtwin, w)
    assert got == [(tvm.TAPE, 5)]
    # the cut document is not judged
    w = WindowArrays(oracle, nm, b'{"a":1} {"b":tru', is_final=False)
    assert (w.docs[0], w.D, w.T) == (2, 1, 5)
    c, got, res = codes(dtwin, w)
    assert got == [(0, UINT64_MAX)] and res.n_documents == 1 and res.n_invalid == 0
    # every pin also equals the definition
    for data, fin in ((b'true"a"', True), (b'12"a"', True), (b'"a":1', True), (b"[1,2]]", True), (b'{"a":1} {"b":tru', False),
                      (b'{"a":[1,2,{"b":null}]}\n[[[[1]]]] "\\ud800" [1 2] {"a" 1} nul', True)):
        w = WindowArrays(oracle, nm, data, is_final=fin)
        for md in (100, 3):
            assert twin_documents(dtwin, w, md)[0] == expected_documents(twin, nm, w, (md,))[md], (data, md)


def test_numbers_capacity_and_scope(oracle, nm, dtwin):
    """The number records: all of them, too few (the flag, and the documents read 0), none asked for; more documents than
    verdicts; a window without a document."""
    w = WindowArrays(oracle, nm, b"1 01 [2,1e999] 3")
    assert w.D == 4 and w.n_errors == 2
    c, got, res = codes(dtwin, w)
    assert c == [0, tvm.NUMBER, tvm.NUMBER, 0] and res.flags == 0 and got[2][1] == 5
    c, _, res = codes(dtwin, w, numbers=1)
    assert c == [0] * 4 and res.flags == tvm.NUMBERS_UNCHECKED
    c, _, res = codes(dtwin, w, numbers="none")
    assert c == [0] * 4 and res.flags == tvm.NUMBERS_UNCHECKED
    ok = WindowArrays(oracle, nm, b"1 2 [3]")
    c, _, res = codes(dtwin, ok, numbers=0)
    assert c == [0, 0, 0] and res.flags == 0   # no error: no record is needed
    _, res = twin_documents(dtwin, w, capacity=w.D - 1)
    assert res.code == 1 and res.n_documents == w.D
    blank = WindowArrays(oracle, nm, b"  \n ")
    got, res = twin_documents(dtwin, blank)
    assert got == [] and (res.code, res.flags, res.n_documents, res.n_invalid, res.first_invalid) == (0, 0, 0, 0, UINT64_MAX)


def test_document_lookup(dtwin):
    first = np.array([2, 3, 10, 11, 500], dtype=np.uint32)
    for tok, want in ((0, 0), (1, 0), (2, 1), (3, 2), (9, 2), (10, 3), (11, 4), (499, 4), (500, 5), (1 << 31, 5)):
        assert dtwin.vdm_docs_starting_up_to(first.ctypes.data, first.size, tok) == want
    assert dtwin.vdm_docs_starting_up_to(first.ctypes.data, 0, 7) == 0
