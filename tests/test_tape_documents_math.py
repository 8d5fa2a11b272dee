"""CPU check of the window form of the tape (mojo_simdjson_amd/csrc/tape_docs_math.h).

msj_tape_documents_device (include/msj_stage1.h) is DEFINED as msj_tape_device's tape and string buffer on every document's
token sub-arrays, laid out in the window's arrays by a closed form.  The one-document twin (tests/tape_math_host.cpp, held
against a serial builder and Python's json by tests/test_tape_math.py) run on those sub-arrays -- the whole window as the
buffer, partners and record tokens rebased, the records of the slice -- is therefore the expected value, and the new twin
(tests/tape_docs_math_host.cpp: prefix sums and one loop over the window through tape_docs_math.h) must give the same
records, the same words at tape_first[k] and the same bytes at string_first[k].  Each document's decoded tape also equals
json.loads of its text, and every container's element count equals the one-document twin's: the claim that "every comma
credits its container" needs no change for a window.  The kernels that run the same headers on the device are covered by
tests/test_tape_documents.py (-m gpu).
"""
import ctypes
import functools
import json
import os
import subprocess

import numpy as np
import pytest

from mojo_simdjson_amd import _lib
from mojo_simdjson_amd.document import Document
from tests import helpers
from tests import test_number_math as tnm
from tests import test_tape_math as ttm
from tests import test_validate_documents_math as tdm
from tests import test_validate_math as tvm

NO_PARTNER = 0xFFFFFFFF
MSJ_CAPACITY = 1
DOC_TAPE_DTYPE = np.dtype([("tape_first", "<u8"), ("string_first", "<u8"), ("tape_words", "<u4"), ("code", "<i4"),
                           ("string_bytes", "<u8")])   # msj_document_tape
TAPE_FILL, BYTE_FILL, REC_FILL = 0xA5A5A5A5A5A5A5A5, 0xA5, 0x77
SEPARATORS = (b"\n", b" ", b"\r\n", b"")
STREAM_DOCS = 64
# an invalid document of a few tokens per code (DEPTH: at max_depth 3), as in tests/test_validate_documents.py
CODES = {tvm.TAPE: b'{"a" 1}', tvm.DEPTH: b"[[[1]]]", tvm.STRING: b'["\\ud800x"]', tvm.T_ATOM: b"[tru]", tvm.F_ATOM: b"[fals]",
         tvm.N_ATOM: b"[nul,1]", tvm.NUMBER: b"[1,01]"}

_twin = None


def load_twin():
    """The host twin of the window call (g++ build of tests/tape_docs_math_host.cpp)."""
    global _twin
    if _twin is not None:
        return _twin
    os.makedirs(tvm.BUILD, exist_ok=True)
    so = os.path.join(tvm.BUILD, "libtape_docs_math_host.so")
    src = os.path.join(helpers.ROOT, "tests", "tape_docs_math_host.cpp")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, src])
    lib = ctypes.CDLL(so)
    lib.tdm_tape_documents.restype = None
    lib.tdm_tape_documents.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p,
         ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    for name, args, res in (("tdm_token_word_at", [ctypes.c_uint64] * 2, ctypes.c_uint64), ("tdm_tape_first", [ctypes.c_uint64] * 2, ctypes.c_uint64),
                            ("tdm_rebased_partner", [ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64], ctypes.c_uint32),
                            ("tdm_block_origin", [ctypes.c_uint64] * 2, ctypes.c_int64),
                            ("tdm_block_slot", [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32], ctypes.c_uint32),
                            ("tdm_window", [ctypes.c_uint64] * 5 + [ctypes.c_void_p], None)):
        getattr(lib, name).argtypes, getattr(lib, name).restype = args, res
    _twin = lib
    return lib


@pytest.fixture(scope="module")
def oracle():
    return helpers.load_oracle()


@pytest.fixture(scope="module")
def tm():
    return ttm.load_twin()


@pytest.fixture(scope="module")
def nm():
    return tnm.load_twin()


@pytest.fixture(scope="module")
def vtwin():
    return tdm.load_twin()


@pytest.fixture(scope="module")
def dtwin():
    return load_twin()


# ---- the window twin ----------------------------------------------------------------------------------------------------

def default_capacities(w):
    """Always enough: two words per token and two root words per document; every body and a length prefix per string."""
    return dict(tape_capacity=3 * w.n + 2, string_capacity=len(w.data) + 4 * w.n + 64, numbers_capacity=int(w.records.size),
                capacity=max(w.D, 1))


def verdict_rows(verdicts):
    """[(code, token)] per document (tdm.twin_documents) -> msj_document_verdict rows"""
    rows = np.zeros(max(len(verdicts), 1), dtype=tdm.VERDICT_DTYPE)
    for k, (c, t) in enumerate(verdicts):
        rows[k] = (c, 0, t)
    return rows


class Built:
    """What one call left: the result, the three arrays with their canaries, the capacities they were given."""

    def __init__(self, res, tape, sbuf, recs, caps, counts=None):
        self.res, self.tape, self.sbuf, self.recs, self.caps, self.counts = res, tape, sbuf, recs, caps, counts

    def canaries_intact(self):
        c = self.caps
        ok = bool((self.tape[c["tape_capacity"]:] == TAPE_FILL).all()) and bool((self.recs.view(np.uint8).reshape(-1, 32)[c["capacity"]:] == REC_FILL).all())
        return ok and (self.sbuf is None or bool((self.sbuf[c["string_capacity"]:] == BYTE_FILL).all()))

    def summary(self):
        r = self.res
        return (r.code, r.flags, r.n_documents, r.n_built, r.tape_words, r.string_bytes, r.n_strings, r.n_numbers, r.reserved)


def twin_window(dtwin, w, verdicts=None, strings=True, canary=8, **caps):
    """tdm_tape_documents over the window's arrays.  verdicts: [(code, token)] per document or None (d_verdicts NULL).
    Capacities default to default_capacities(w).  -> Built (with the direct commas credited to every token)"""
    c = default_capacities(w)
    c.update(caps)
    tape = np.full(c["tape_capacity"] + canary, TAPE_FILL, dtype=np.uint64)
    sbuf = np.full(c["string_capacity"] + 8 * canary, BYTE_FILL, dtype=np.uint8) if strings else None
    recs = np.frombuffer(bytes([REC_FILL]) * (32 * (c["capacity"] + canary)), dtype=DOC_TAPE_DTYPE).copy()
    counts = np.zeros(max(w.n, 1), dtype=np.uint32)
    docs = _lib.MsjDocumentsResult(*w.docs)
    res = _lib.MsjTapeDocumentsResult()
    numbers = np.ascontiguousarray(w.records[:c["numbers_capacity"]])
    rows = verdict_rows(verdicts) if verdicts is not None else None
    arrs = [np.ascontiguousarray(a) for a in (w.idx, w.typ, w.depth, w.match, w.end, w.flags, w.first)]
    dtwin.tdm_tape_documents(w.data, len(w.data), arrs[0].ctypes.data, w.n, *[a.ctypes.data for a in arrs[1:]], ctypes.byref(docs),
                             numbers.ctypes.data if numbers.size else None, c["numbers_capacity"],
                             rows.ctypes.data if rows is not None else None, tape.ctypes.data, c["tape_capacity"],
                             sbuf.ctypes.data if strings else None, c["string_capacity"] if strings else 0, recs.ctypes.data, c["capacity"],
                             ctypes.byref(res), counts.ctypes.data)
    return Built(res, tape, sbuf, recs, c, counts[:w.n])


# ---- the definition -----------------------------------------------------------------------------------------------------

def words_prefix(w):
    """W(i) - W(f_0) for i in [0, n] from the definition's words per token (tokens outside [f_0, T) count nothing)"""
    per = np.where(w.flags & 4, 2, np.isin(w.typ, np.frombuffer(b'{}[]"tfn', dtype=np.uint8)).astype(np.int64))
    if w.D:
        per[:int(w.first[0])] = 0
        per[w.T:] = 0
    else:
        per[:] = 0
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def document_arrays(w, k):
    """The token sub-arrays [f_k, e_k) as the one-document call takes them: partners rebased, the records of the slice"""
    f, e = w.bounds(k)
    m = w.match[f:e].astype(np.int64)
    inside = (m != NO_PARTNER) & (m >= f) & (m < e)
    rec = w.records[(w.records["token"] >= f) & (w.records["token"] < e)]
    return dict(idx=w.idx[f:e], typ=w.typ[f:e], depth=w.depth[f:e], match=np.where(inside, m - f, NO_PARTNER).astype(np.uint32),
                end=w.end[f:e], flags=w.flags[f:e], bits=rec["bits"].copy(), kinds=rec["kind"].copy(),
                num_tokens=(rec["token"] - f).astype(np.uint32))


def check_against_definition(tm, w, got, codes=None, texts=None, counts=True):
    """`got` (a Built with room for everything) against the one-document twin on every document's sub-arrays, the closed
    form of the layout and, given the documents' texts, json.loads.  codes: the verdict's code per document (None: all 0)."""
    res, recs = got.res, got.recs
    codes = [0] * w.D if codes is None else list(codes)
    W = words_prefix(w)
    assert (res.code, res.flags, res.n_documents, res.reserved) == (0, 0, w.D, 0)
    assert res.n_built == sum(1 for c in codes if c == 0)
    assert res.tape_words == (int(W[w.T]) + 2 * w.D if w.D else 0)
    assert got.canaries_intact()
    sfirst = 0
    for k in range(w.D):
        f, e = w.bounds(k)
        r = recs[k]
        assert int(r["tape_first"]) == int(W[f]) + 2 * k, (k, r)
        assert int(r["code"]) == codes[k], (k, r, codes[k])
        if k and codes[k - 1] == 0:
            assert int(r["string_first"]) == sfirst, (k, r)
        if codes[k]:
            assert (int(r["tape_words"]), int(r["string_bytes"])) == (0, 0), (k, r)
            continue
        a = document_arrays(w, k)
        want, w_tape, w_sbuf, _, w_counts, _ = ttm.twin_build(tm, w.data, a, extras=True)
        assert want.code == 0
        assert (int(r["tape_words"]), int(r["string_bytes"])) == (want.tape_words, want.string_bytes), (k, r, w.data[:120])
        t0, s0 = int(r["tape_first"]), int(r["string_first"])
        tape = got.tape[t0:t0 + want.tape_words]
        assert np.array_equal(tape, w_tape[:want.tape_words]), (k, w.data[:120], [hex(int(x)) for x in tape[:8]])
        sfirst = s0 + want.string_bytes
        if got.sbuf is not None:
            sbuf = got.sbuf[s0:s0 + want.string_bytes]
            assert np.array_equal(sbuf, w_sbuf[:want.string_bytes]), (k, w.data[:120])
            if texts is not None:
                assert Document(tape, sbuf).to_python() == json.loads(texts[k].decode("utf-8")), (k, texts[k][:120])
        if counts and got.counts is not None:
            opens = np.isin(a["typ"], np.frombuffer(b"[{", dtype=np.uint8))
            assert np.array_equal(got.counts[f:e][opens], w_counts[opens]), (k, w.data[:120])
    if w.D and codes[-1] == 0:
        assert res.string_bytes == sfirst
    assert (recs.view(np.uint8).reshape(-1, 32)[w.D:] == REC_FILL).all()   # nothing past D


# ---- the corpus (shared with the GPU test) ------------------------------------------------------------------------------

def may_touch(left, right):
    """May `right` follow `left` with nothing in between?  Where a bracket stands on either side of the border."""
    return left[-1:] in (b"]", b"}") or right[:1] in (b"[", b"{")


def join(docs, sep):
    """The documents joined by `sep`; a blank where nothing would glue two scalars together -> bytes"""
    out = [docs[0]]
    for prev, d in zip(docs, docs[1:]):
        out.append(sep if sep or may_touch(prev, d) else b" ")
        out.append(d)
    return b"".join(out) + (sep or b"\n")


@functools.lru_cache(maxsize=None)
def corpus_streams():
    """[(stream, its documents)]: the four stage-2 fixtures and the valid escape cases of the tape tests' corpus, and 2 048
    seeded documents, in streams of 64, each kind joined by each of the four separators in turn."""
    oracle = helpers.load_oracle()
    small = ttm.fixture_documents()
    for body in tvm.escape_cases():
        doc = tvm._string_doc(body)
        idx = tvm.stage1(oracle, doc)
        if idx is not None and tvm.walk(doc, idx.tolist()) == (tvm.SUCCESS, None):
            small.append(doc)
    assert len(small) >= 44
    seeded = [doc for doc, _ in tvm.seeded_documents(20260, 2048)]
    out = []
    for sep in SEPARATORS:
        out.append((join(small, sep), small))
    for s in range(0, len(seeded), STREAM_DOCS):
        docs = seeded[s:s + STREAM_DOCS]
        out.append((join(docs, SEPARATORS[(s // STREAM_DOCS) % 4]), docs))
    return out


def mixed_stream(valid):
    """One invalid document of every code between valid ones -> (bytes, documents, {document number: code})"""
    docs, bad = [], {}
    for k, (code, text) in enumerate(sorted(CODES.items())):
        docs += [valid[2 * k], valid[2 * k + 1]]
        bad[len(docs)] = code
        docs.append(text)
    docs += valid[2 * len(CODES):2 * len(CODES) + 3]
    return join(docs, b"\n"), docs, bad


# ---- tests ----------------------------------------------------------------------------------------------------------------

def test_corpus_equals_single_document_twin(oracle, tm, nm, dtwin):
    """Every document of every stream: record, words, bytes and element counts are the one-document twin's on the
    sub-arrays, and the decoded tape is json.loads of the document's text; with d_verdicts NULL and with all-zero verdicts."""
    n_docs = 0
    for j, (data, docs) in enumerate(corpus_streams()):
        w = tdm.WindowArrays(oracle, nm, data, is_final=True)
        assert w.D == len(docs) and w.T == w.n, (j, w.D, len(docs))
        got = twin_window(dtwin, w, verdicts=[(0, tvm.UINT64_MAX)] * w.D if j % 2 else None)
        check_against_definition(tm, w, got, texts=docs)
        n_docs += w.D
    assert n_docs >= 2048 + 4 * 44


def test_invalid_documents_keep_their_slot(oracle, tm, nm, vtwin, dtwin):
    """One document of every error code between valid ones: its record has the code and zero sizes, its neighbours are
    exact, and the layout is the closed form whatever the verdicts say.  At max_depth 100 and 3."""
    valid = [doc for doc, _ in tvm.seeded_documents(20260, 64)]
    data, docs, bad = mixed_stream(valid)
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    assert w.D == len(docs)
    seen = set()
    for md in (100, 3):
        verdicts, _ = tdm.twin_documents(vtwin, w, md)
        codes = [c for c, _ in verdicts]
        for k, code in bad.items():
            if code != tvm.DEPTH or md == 3:
                assert codes[k] == code, (k, code, codes[k])
        seen |= set(codes)
        got = twin_window(dtwin, w, verdicts=verdicts)
        check_against_definition(tm, w, got, codes=codes, texts=docs)
        # without verdicts every slot is built: the valid documents and the layout are the same
        free = twin_window(dtwin, w)
        assert free.res.n_built == w.D and (free.res.tape_words, free.res.string_bytes) == (got.res.tape_words, got.res.string_bytes)
        for k in range(w.D):
            assert (int(free.recs[k]["tape_first"]), int(free.recs[k]["string_first"])) == \
                (int(got.recs[k]["tape_first"]), int(got.recs[k]["string_first"]))
    assert seen >= set(CODES) | {0}


def test_cut_window_and_no_document(oracle, tm, nm, dtwin):
    """A cut last document (not final): nothing at or past T is counted or written.  A window without a complete document,
    and one without a token: a zero result."""
    docs = [b'{"a":[1,2,{"b":"x\\ny"}]}', b"[1.5,true]", b'"s"']
    w = tdm.WindowArrays(oracle, nm, b" ".join(docs) + b' {"cut":[1,"abc', is_final=False)
    assert (w.docs[0], w.D) == (4, 3) and w.T < w.n
    got = twin_window(dtwin, w)
    check_against_definition(tm, w, got, texts=docs)
    used = int(got.res.tape_words)
    assert (got.tape[used:] == TAPE_FILL).all() and (got.sbuf[int(got.res.string_bytes):] == BYTE_FILL).all()
    assert got.res.n_numbers == 3   # 1, 2 and 1.5: the cut document's number is not one of them
    for data in (b'{"cut":[1,"abc', b"  \n "):
        w = tdm.WindowArrays(oracle, nm, data, is_final=False)
        assert w.D == 0
        got = twin_window(dtwin, w)
        assert got.summary() == (0,) * 9 and got.canaries_intact() and (got.tape == TAPE_FILL).all()


BELOW_ZERO = b'] [ "a" , 1 ] [2] 7\n'   # the split starts 4 documents at tokens 2, 3, 4 and 7; the first is the valid "a"


def test_tokens_below_depth_zero_in_front(oracle, tm, nm, vtwin, dtwin):
    """A window whose first tokens sit below depth 0 in front of d_doc_first[0]: they write nothing and count nothing, the
    valid document behind them is exact and starts at word 0."""
    w = tdm.WindowArrays(oracle, nm, BELOW_ZERO, is_final=True)
    assert w.first[:w.D].tolist() == [2, 3, 4, 7] and w.depth[:2].tolist() == [-1, -1]
    verdicts, _ = tdm.twin_documents(vtwin, w)
    codes = [c for c, _ in verdicts]
    assert codes[0] == 0 and codes[1] != 0
    got = twin_window(dtwin, w, verdicts=verdicts)
    check_against_definition(tm, w, got, codes=codes)
    assert int(got.recs[0]["tape_first"]) == 0 and int(got.recs[0]["string_first"]) == 0
    w = tdm.WindowArrays(oracle, nm, b"]] [1,2] 3\n", is_final=True)   # never back at depth 0: no document at all
    assert w.D == 0 and twin_window(dtwin, w).summary() == (0,) * 9


def test_capacities_clip(oracle, tm, nm, dtwin):
    """Each of tape, string buffer, records and number records one short: MSJ_CAPACITY with the true sizes, nothing behind a
    capacity written; the layout-only form gives the same tape."""
    data, docs = corpus_streams()[5]
    w = tdm.WindowArrays(oracle, nm, data, is_final=True)
    full = twin_window(dtwin, w)
    check_against_definition(tm, w, full, texts=docs)
    exact = dict(tape_capacity=int(full.res.tape_words), string_capacity=int(full.res.string_bytes), numbers_capacity=int(full.res.n_numbers),
                 capacity=w.D)
    assert full.res.n_numbers == w.records.size > 0
    check_against_definition(tm, w, twin_window(dtwin, w, **exact), texts=docs)
    for name in exact:
        short = dict(exact)
        short[name] -= 1
        got = twin_window(dtwin, w, **short)
        assert got.res.code == MSJ_CAPACITY and got.canaries_intact(), name
        assert got.summary()[2:] == (w.D, 0 if name == "capacity" else w.D) + full.summary()[4:], name
    lay = twin_window(dtwin, w, strings=False)
    assert lay.summary() == full.summary() and np.array_equal(lay.tape, full.tape)


def test_layout_pieces(dtwin):
    """Word addresses are 64-bit; the partner rebase; a block's slots (the densest block: kBlock one-token number documents
    stage 4 * kBlock words); the window clipped to n."""
    assert dtwin.tdm_token_word_at((1 << 32) - 2, 1 << 31) == (1 << 32) - 2 + (1 << 32) + 1
    assert dtwin.tdm_tape_first(10, 3) == 16 and dtwin.tdm_token_word_at(10, 3) == 17
    for m, f, e, want in ((7, 5, 9, 2), (5, 5, 9, 0), (9, 5, 9, NO_PARTNER), (4, 5, 9, NO_PARTNER), (NO_PARTNER, 0, 1 << 31, NO_PARTNER)):
        assert dtwin.tdm_rebased_partner(m, f, e) == want
    assert dtwin.tdm_block_origin(0, 0) == -1 and dtwin.tdm_block_origin(2048, 1024) == 4095
    assert [dtwin.tdm_block_slot(2 * t, 0, t + 1) for t in (0, 1, 1023)] == [2, 6, 4094]   # + 1 for the number's second word
    out = np.zeros(4, dtype=np.uint64)
    for args, want in (((3, 10, 8, 5, 2), (3, 8, 2, 0)), ((9, 10, 8, 5, 0), (8, 8, 0, 1)), ((0, 0, 8, 5, 0), (0, 0, 0, 0)),
                       ((2, 6, 8, 5, 6), (0, 6, 6, 0))):
        dtwin.tdm_window(*args, out.ctypes.data)
        assert tuple(int(x) for x in out) == want, (args, tuple(out))
